// densify.hip -- GaussianModel.densify_and_prune (gaussian_model.py:402-469) as a plan and an apply.
// The reference clones the small high-gradient Gaussians, splits the large ones into N samples,
// drops the split originals and prunes the transparent / world-space large rows with two torch.cat
// appends and two boolean-mask selections over the six parameter tensors and both Adam moments:
// every array is read and written four times and every mask is a nonzero(), i.e. a host
// synchronisation.  Here every source row's fate is decided once and every output element is
// written once.
//
// Plan (three small launches over the P source rows, one wave per DENSIFY_ROWS_PER_WAVE rows, four
// waves per workgroup):
//   decide   24 B in per row (accum, denom, 3 scales, opacity), 1 B out (the decision code), and per
//            wave five counts (ballot + popcount, no LDS, no atomics);
//   offsets  ONE workgroup turns the per-wave counts into exclusive offsets (20 B per 1024 rows) and
//            stores the five totals in the workspace header and in pinned host memory;
//   scatter  1 B in per row; writes the source row of every kept original, kept clone and kept split
//            parent (the latter with its rank among ALL split rows, which picks its samples) in output
//            order: 4 B per kept original / clone, 8 B per kept split parent.
// No inter-workgroup waiting anywhere: the launches are the barriers.  The host reads the totals after
// one stream synchronisation, allocates the P_after output rows and draws the N * n_split samples.
//
// Apply (one launch over every group): one thread per OUTPUT element e = row * M + c of a group,
// which writes the parameter and, where the group has optimizer state, both moments.  The output
// row's source comes from the three lists (a 4-B read shared by the M threads of a row).  Per output
// element: 4 B in + 4 B out for the parameter, and for a group with moments 8 B out plus 8 B in for
// kept originals (clones and children get zero moments without a read).  Stores are consecutive
// dwords; loads run along the source rows in order, so they come in long runs too.  Only a split
// child's xyz and scaling are computed (another 40 B / 4 B of cached reads per element): plain fp32,
// no contraction (the library's -ffp-contract=off).  At SH degree 3 that is 236 B in + 236 B out per
// output row, 3 x that with moments.
#include "gsr_common.h"
#include "gsr_kernels.h"

namespace gsr {

namespace {

enum : uint32_t {
    DC_KEEP_ORIG = 1u,   // the row itself survives
    DC_KEEP_CLONE = 2u,  // its clone survives
    DC_SPLIT = 4u,       // split-selected (pruned or not: the rank among these indexes the samples)
    DC_KEEP_SPLIT = 8u,  // its N children survive
    DC_CLONE = 16u       // clone-selected (counted only)
};
constexpr int N_COUNTS = 5;  // totals, in the order of the bits above
// header words behind the five totals
constexpr int HDR_P = 5, HDR_N = 6, HDR_WORDS = 64;

struct Workspace {
    uint32_t* hdr;         // HDR_WORDS
    uint32_t* wave_count;  // N_COUNTS per wave: counts, then (offsets kernel) exclusive offsets
    uint8_t* code;         // P
    uint32_t* orig;        // P: source rows of the kept originals, in order
    uint32_t* clone;       // P: ... of the kept clones
    uint32_t* split;       // P: ... of the kept split parents
    uint32_t* split_rank;  // P: their ranks among all split-selected rows
};

__host__ __device__ inline size_t ws_align(size_t x) { return (x + 255) & ~(size_t)255; }
__host__ __device__ inline uint32_t n_waves(int P)
{
    return (uint32_t)(((size_t)P + DENSIFY_ROWS_PER_WAVE - 1) / DENSIFY_ROWS_PER_WAVE);
}
// byte offsets of the seven arrays, and the total behind them
inline size_t layout(int P, size_t off[7])
{
    const size_t sizes[7] = {4 * (size_t)HDR_WORDS, 4 * (size_t)N_COUNTS * n_waves(P), (size_t)P,
                             4 * (size_t)P, 4 * (size_t)P, 4 * (size_t)P, 4 * (size_t)P};
    size_t at = 0;
    for (int k = 0; k < 7; k++) {
        off[k] = at;
        at += ws_align(sizes[k]);
    }
    return at;
}
inline Workspace carve(char* w, int P)
{
    size_t off[7];
    layout(P, off);
    Workspace s;
    s.hdr = reinterpret_cast<uint32_t*>(w + off[0]);
    s.wave_count = reinterpret_cast<uint32_t*>(w + off[1]);
    s.code = reinterpret_cast<uint8_t*>(w + off[2]);
    s.orig = reinterpret_cast<uint32_t*>(w + off[3]);
    s.clone = reinterpret_cast<uint32_t*>(w + off[4]);
    s.split = reinterpret_cast<uint32_t*>(w + off[5]);
    s.split_rank = reinterpret_cast<uint32_t*>(w + off[6]);
    return s;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot)
{
    const uint32_t lane = threadIdx.x & 63;
    return (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
}

}  // namespace

// ---- plan -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) densify_decide_kernel(DensifyPlanArgs a, uint8_t* code, uint32_t* wave_count)
{
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (gw >= n_waves(a.P)) return;  // wave-uniform
    const size_t row0 = (size_t)gw * DENSIFY_ROWS_PER_WAVE;
    uint32_t cnt[N_COUNTS] = {0, 0, 0, 0, 0};
    for (int it = 0; it < DENSIFY_ROWS_PER_WAVE / 64; it++) {
        const size_t i = row0 + (size_t)it * 64 + lane;
        uint32_t c = 0;
        if (i < (size_t)a.P) {
            float g = a.accum[i * a.accum_stride] / a.denom[i * a.denom_stride];
            if (g != g) g = 0.f;  // 0/0: never seen
            const float e0 = expf(a.scaling[3 * i]), e1 = expf(a.scaling[3 * i + 1]), e2 = expf(a.scaling[3 * i + 2]);
            const float smax = fmaxf(e0, fmaxf(e1, e2));
            const bool hot = g >= a.max_grad;
            const bool clone = hot && smax <= a.dense_extent, split = hot && smax > a.dense_extent;
            const bool low = 1.0f / (1.0f + expf(-a.opacity[i])) < a.min_opacity;
            bool big = false, bigchild = false;
            if (a.big_extent >= 0.f) {
                big = smax > a.big_extent;
                const float c0 = expf(logf(e0 / a.shrink)), c1 = expf(logf(e1 / a.shrink)),
                            c2 = expf(logf(e2 / a.shrink));
                bigchild = fmaxf(c0, fmaxf(c1, c2)) > a.big_extent;
            }
            const bool keep = !(low || big);
            if (!split && keep) c |= DC_KEEP_ORIG;
            if (clone && keep) c |= DC_KEEP_CLONE;
            if (split) c |= DC_SPLIT;
            if (split && !(low || bigchild)) c |= DC_KEEP_SPLIT;
            if (clone) c |= DC_CLONE;
            code[i] = (uint8_t)c;
        }
#pragma unroll
        for (int f = 0; f < N_COUNTS; f++) cnt[f] += (uint32_t)__popcll(__ballot((c >> f) & 1u));
    }
    if (lane < N_COUNTS) {
        uint32_t v = cnt[0];
#pragma unroll
        for (int f = 1; f < N_COUNTS; f++) v = lane == (uint32_t)f ? cnt[f] : v;
        wave_count[(size_t)gw * N_COUNTS + lane] = v;
    }
}

// One workgroup: the per-wave counts become exclusive offsets in place; the totals go to the header
// and (system-scope stores) to the host's pinned words.  Thread t owns a contiguous run of waves.
__global__ void __launch_bounds__(256) densify_offsets_kernel(uint32_t nw, uint32_t* wave_count, uint32_t* hdr,
                                                              uint32_t* host_out, int P, int N)
{
    __shared__ uint32_t part[256][N_COUNTS];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nw + 255) / 256;
    const uint32_t w0 = t * per < nw ? t * per : nw, w1 = w0 + per < nw ? w0 + per : nw;
    uint32_t sum[N_COUNTS] = {0, 0, 0, 0, 0};
    for (uint32_t w = w0; w < w1; w++)
        for (int f = 0; f < N_COUNTS; f++) sum[f] += wave_count[(size_t)w * N_COUNTS + f];
    for (int f = 0; f < N_COUNTS; f++) part[t][f] = sum[f];
    __syncthreads();
    if (t < N_COUNTS) {  // serial over the 256 partial sums of one field
        uint32_t run = 0;
        for (int k = 0; k < 256; k++) {
            const uint32_t v = part[k][t];
            part[k][t] = run;
            run += v;
        }
        hdr[t] = run;
        __hip_atomic_store(host_out + t, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (t == 0) {
        hdr[HDR_P] = (uint32_t)P;
        hdr[HDR_N] = (uint32_t)N;
    }
    __syncthreads();
    uint32_t run[N_COUNTS];
    for (int f = 0; f < N_COUNTS; f++) run[f] = part[t][f];
    for (uint32_t w = w0; w < w1; w++)
        for (int f = 0; f < N_COUNTS; f++) {
            const uint32_t v = wave_count[(size_t)w * N_COUNTS + f];
            wave_count[(size_t)w * N_COUNTS + f] = run[f];
            run[f] += v;
        }
}

__global__ void __launch_bounds__(256) densify_scatter_kernel(int P, Workspace ws)
{
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (gw >= n_waves(P)) return;  // wave-uniform
    const size_t row0 = (size_t)gw * DENSIFY_ROWS_PER_WAVE;
    uint32_t off[4];
#pragma unroll
    for (int f = 0; f < 4; f++) off[f] = ws.wave_count[(size_t)gw * N_COUNTS + f];
    for (int it = 0; it < DENSIFY_ROWS_PER_WAVE / 64; it++) {
        const size_t i = row0 + (size_t)it * 64 + lane;
        const uint32_t c = i < (size_t)P ? ws.code[i] : 0u;
        uint64_t b[4];
#pragma unroll
        for (int f = 0; f < 4; f++) b[f] = __ballot((c >> f) & 1u);
        // every index below is < the field's total <= P (a row sets each bit at most once)
        if (c & DC_KEEP_ORIG) ws.orig[off[0] + lanes_below(b[0])] = (uint32_t)i;
        if (c & DC_KEEP_CLONE) ws.clone[off[1] + lanes_below(b[1])] = (uint32_t)i;
        if (c & DC_KEEP_SPLIT) {
            const uint32_t k = off[3] + lanes_below(b[3]);
            ws.split[k] = (uint32_t)i;
            ws.split_rank[k] = off[2] + lanes_below(b[2]);
        }
#pragma unroll
        for (int f = 0; f < 4; f++) off[f] += (uint32_t)__popcll(b[f]);
    }
}

size_t densify_workspace_bytes(int P)
{
    if (P <= 0) return 0;
    size_t off[7];
    return layout(P, off);
}

// the 0.8 * N of gaussian_model.py:419 as torch divides by it: the double product rounded to float
float densify_split_shrink(int N) { return (float)(0.8 * (double)N); }

hipError_t launch_densify_plan(const DensifyPlanArgs& a, char* workspace, uint32_t* host_counts, hipStream_t s)
{
    if (a.P <= 0) return hipSuccess;
    const Workspace ws = carve(workspace, a.P);
    const uint32_t nw = n_waves(a.P), blocks = (nw + 3) / 4;
    hipLaunchKernelGGL(densify_decide_kernel, dim3(blocks), dim3(256), 0, s, a, ws.code, ws.wave_count);
    hipLaunchKernelGGL(densify_offsets_kernel, dim3(1), dim3(256), 0, s, nw, ws.wave_count, ws.hdr, host_counts, a.P,
                       a.N);
    hipLaunchKernelGGL(densify_scatter_kernel, dim3(blocks), dim3(256), 0, s, a.P, ws);
    return hipGetLastError();
}

// ---- apply ----------------------------------------------------------------------------------
struct DensifyApplyKernelArgs {
    DensifyApplyArgs a;
    Workspace ws;
    uint32_t block_start[DENSIFY_MAX_GROUPS];  // first workgroup of each group
};

// component c of R(normalize(q)) (s * z) + xyz, as multiview.build_rotation and the bmm form it
__device__ __forceinline__ float child_xyz(const float* q4, const float* s3, const float* z3, float xyz_c, int c)
{
    const float r0 = q4[0], r1 = q4[1], r2 = q4[2], r3 = q4[3];
    const float norm = sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    const float w = r0 / norm, x = r1 / norm, y = r2 / norm, z = r3 / norm;
    float R0, R1, R2;
    if (c == 0) {
        R0 = 1.f - 2.f * (y * y + z * z);
        R1 = 2.f * (x * y - w * z);
        R2 = 2.f * (x * z + w * y);
    } else if (c == 1) {
        R0 = 2.f * (x * y + w * z);
        R1 = 1.f - 2.f * (x * x + z * z);
        R2 = 2.f * (y * z - w * x);
    } else {
        R0 = 2.f * (x * z - w * y);
        R1 = 2.f * (y * z + w * x);
        R2 = 1.f - 2.f * (x * x + y * y);
    }
    const float v0 = z3[0] * expf(s3[0]), v1 = z3[1] * expf(s3[1]), v2 = z3[2] * expf(s3[2]);
    return (R0 * v0 + R1 * v1 + R2 * v2) + xyz_c;
}

__global__ void __launch_bounds__(256) densify_apply_kernel(DensifyApplyKernelArgs k)
{
    const DensifyApplyArgs& a = k.a;
    const uint32_t* hdr = k.ws.hdr;
    const uint32_t n_ko = hdr[0], n_kc = hdr[1], n_split = hdr[2], n_ks = hdr[3];
    // the plan in the workspace is the one these sizes came from, or nothing is read or written
    if (hdr[HDR_P] != (uint32_t)a.P || hdr[HDR_N] != (uint32_t)a.N || n_split != (uint32_t)a.n_split ||
        (uint64_t)n_ko + n_kc + (uint64_t)a.N * n_ks != (uint64_t)a.P_after)
        return;
    int gi = 0;
#pragma unroll
    for (int g = 1; g < DENSIFY_MAX_GROUPS; g++)
        if (g < a.n_groups && blockIdx.x >= k.block_start[g]) gi = g;
    const uint32_t M = (uint32_t)a.M[gi];
    const size_t n = (size_t)a.P_after * M;
    const size_t e = (size_t)(blockIdx.x - k.block_start[gi]) * 256 + threadIdx.x;
    if (e >= n) return;
    size_t o;
    uint32_t c;
    if (n <= 0xFFFFFFFFull) {  // (uniform) 32-bit division
        const uint32_t o32 = (uint32_t)e / M;
        o = o32;
        c = (uint32_t)e - o32 * M;
    } else {
        o = e / M;
        c = (uint32_t)(e - o * M);
    }
    size_t src;
    uint32_t r = 0, j = 0;
    int kind;  // 0 original, 1 clone, 2 split child
    if (o < n_ko) {
        src = k.ws.orig[o];
        kind = 0;
    } else if (o < (size_t)n_ko + n_kc) {
        src = k.ws.clone[o - n_ko];
        kind = 1;
    } else {  // n_ks > 0 here: the children are the last N * n_ks rows
        const size_t q = o - n_ko - n_kc;
        r = (uint32_t)(q / n_ks);
        const size_t p = q - (size_t)r * n_ks;
        src = k.ws.split[p];
        j = k.ws.split_rank[p];
        kind = 2;
    }
    float v;
    if (kind == 2 && gi == a.xyz_group) {
        const float* z3 = a.samples + 3 * ((size_t)r * n_split + j);
        v = child_xyz(a.src[a.rotation_group] + 4 * src, a.src[a.scaling_group] + 3 * src, z3,
                      a.src[gi][3 * src + c], (int)c);
    } else if (kind == 2 && gi == a.scaling_group) {
        v = logf(expf(a.src[gi][3 * src + c]) / a.shrink);
    } else {
        v = a.src[gi][src * M + c];
    }
    a.dst[gi][e] = v;
    if (a.dst_m[gi]) {
        a.dst_m[gi][e] = kind == 0 ? a.src_m[gi][src * M + c] : 0.f;
        a.dst_v[gi][e] = kind == 0 ? a.src_v[gi][src * M + c] : 0.f;
    }
}

hipError_t launch_densify_apply(const DensifyApplyArgs& a, const char* workspace, hipStream_t s)
{
    if (a.P <= 0 || a.P_after <= 0 || a.n_groups <= 0) return hipSuccess;
    DensifyApplyKernelArgs k;
    k.a = a;
    k.ws = carve(const_cast<char*>(workspace), a.P);
    size_t blocks = 0;
    for (int g = 0; g < DENSIFY_MAX_GROUPS; g++) {
        k.block_start[g] = (uint32_t)blocks;
        if (g < a.n_groups) blocks += ((size_t)a.P_after * a.M[g] + 255) / 256;
        if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    }
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(densify_apply_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, k);
    return hipGetLastError();
}

}  // namespace gsr
