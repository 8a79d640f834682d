// activations.hip -- the parameter activations between the optimizer's raw tensors and the
// rasterizer (GaussianModel.get_scaling / get_rotation / get_opacity, gaussian_model.py:102-135):
//     scales = exp(scaling),  opacities = sigmoid(opacity),  rotations = normalize(rotation)
// and the chain rule torch's autograd applies to them, each as ONE launch over all three groups
// where the torch chain is about five launches forward and ten backward plus three AccumulateGrad
// passes.  normalize is torch.nn.functional.normalize's x / max(|x|_2, eps) with its default eps
// 1e-12; its backward carries clamp_min's mask, so a quaternion shorter than eps (the zero one too)
// gets g / eps.  The backward reads the saved OUTPUTS of exp and sigmoid, as torch does, and has no
// transcendental.
//
// Indexing: one thread per Gaussian (as densify_stats_kernel), size_t indices, 256-thread
// workgroups, no LDS, no atomics: every output element is written by exactly one thread from that
// Gaussian's inputs alone, so results are bitwise reproducible.  Streaming: 32 B in and 32 B out per
// Gaussian forward; 64 B in and 32 B out backward (96 B), 128 B when every destination is
// accumulated into (its 32 B are read as well).  Plain fp32 (expf, sqrtf, IEEE division) under the
// library's -ffp-contract=off.  The (P,4) arrays move as 16-byte accesses only when the host found
// every one of them 16-byte aligned (gradient destinations are views of a flat buffer at any
// 4-byte-aligned offset); everything else is dword accesses.
#include "gsr_kernels.h"

namespace gsr {

constexpr float ACT_NORM_EPS = 1e-12f;  // torch.nn.functional.normalize's default eps

template <bool VEC>
__device__ __forceinline__ void load_quad(const float* p, size_t i, float v[4])
{
    if (VEC) {
        const float4 t = reinterpret_cast<const float4*>(p)[i];
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = p[4 * i + k];
    }
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float* p, size_t i, const float v[4])
{
    if (VEC) {
        reinterpret_cast<float4*>(p)[i] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) p[4 * i + k] = v[k];
    }
}

// n = |q|_2 (summed in component order), d = max(n, eps)
__device__ __forceinline__ void quat_norm(const float q[4], float& n, float& d)
{
    float s = q[0] * q[0];
#pragma unroll
    for (int k = 1; k < 4; k++) s += q[k] * q[k];
    n = sqrtf(s);
    d = fmaxf(n, ACT_NORM_EPS);
}

template <bool VEC>
__global__ void __launch_bounds__(256) activate_fwd_kernel(ActivateFwdArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.P) return;
#pragma unroll
    for (int k = 0; k < 3; k++) a.scales[3 * i + k] = expf(a.scaling[3 * i + k]);
    a.opacities[i] = 1.0f / (1.0f + expf(-a.opacity[i]));
    float q[4], n, d;
    load_quad<VEC>(a.rotation, i, q);
    quat_norm(q, n, d);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = q[k] / d;
    store_quad<VEC>(a.rotations, i, q);
}

template <bool VEC>
__global__ void __launch_bounds__(256) activate_bwd_kernel(ActivateBwdArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.P) return;
    if (a.dL_dscales) {  // exp: g * y
        const bool acc = a.acc & ACT_ACC_SCALING;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const size_t e = 3 * i + k;
            const float v = a.dL_dscales[e] * a.scales[e];
            a.dL_dscaling[e] = acc ? a.dL_dscaling[e] + v : v;
        }
    }
    if (a.dL_dopacities) {  // sigmoid: g (1 - y) y
        const float y = a.opacities[i];
        const float v = a.dL_dopacities[i] * (1.0f - y) * y;
        a.dL_dopacity[i] = (a.acc & ACT_ACC_OPACITY) ? a.dL_dopacity[i] + v : v;
    }
    if (a.dL_drotations) {  // normalize: (g - m r (r . g)) / d, m = clamp_min's mask
        float q[4], g[4], n, d;
        load_quad<VEC>(a.rotation, i, q);
        load_quad<VEC>(a.dL_drotations, i, g);
        quat_norm(q, n, d);
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = q[k] / d;
        float rg = r[0] * g[0];
#pragma unroll
        for (int k = 1; k < 4; k++) rg += r[k] * g[k];
        const float m = n >= ACT_NORM_EPS ? 1.0f : 0.0f;
        float out[4];
#pragma unroll
        for (int k = 0; k < 4; k++) out[k] = (g[k] - m * r[k] * rg) / d;
        if (a.acc & ACT_ACC_ROTATION) {
            float old[4];
            load_quad<VEC>(a.dL_drotation, i, old);
#pragma unroll
            for (int k = 0; k < 4; k++) out[k] = old[k] + out[k];
        }
        store_quad<VEC>(a.dL_drotation, i, out);
    }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

hipError_t launch_activate_fwd(const ActivateFwdArgs& a, hipStream_t s)
{
    if (a.P <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((size_t)a.P + 255) / 256);
    if (aligned16(a.rotation) && aligned16(a.rotations))
        hipLaunchKernelGGL(activate_fwd_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(activate_fwd_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_activate_bwd(const ActivateBwdArgs& a, hipStream_t s)
{
    if (a.P <= 0 || (!a.dL_dscales && !a.dL_drotations && !a.dL_dopacities)) return hipSuccess;
    const unsigned blocks = (unsigned)(((size_t)a.P + 255) / 256);
    // (a skipped rotation group has null pointers, which count as aligned: either kernel will do)
    if (aligned16(a.rotation) && aligned16(a.dL_drotations) && aligned16(a.dL_drotation))
        hipLaunchKernelGGL(activate_bwd_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(activate_bwd_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace gsr
