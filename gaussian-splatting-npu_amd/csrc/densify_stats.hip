// densify_stats.hip -- train.py's densification statistics for a batch of views in one launch.
// The reference updates them once per view with boolean-mask indexing (train.py:166: running max of
// the screen radii over the visible Gaussians; gaussian_model.py:471-473: the norm of the view's
// screen-space gradient and a visit count); every such indexing is a nonzero() and so a
// device-to-host synchronisation.  Here one thread owns one Gaussian and folds the V views in
// order, so the float sums round exactly as V successive per-view updates do, and nothing is read
// back.  Streaming: 20 B per (view, Gaussian) in, 12-16 B per visible Gaussian in and out.
#include "gsr_common.h"
#include "gsr_kernels.h"

namespace gsr {

__global__ void __launch_bounds__(256) densify_stats_kernel(DensifyStatsArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.P) return;
    int seen = 0, rmax = 0;
    float sum = 0.f;
    for (int v = 0; v < a.V; v++) {
        const size_t k = (size_t)v * a.P + i;
        const int r = a.radii[k];
        if (r <= 0) continue;
        if (seen == 0) sum = a.accum[i * a.accum_stride];  // read only for a Gaussian some view sees
        const float gx = a.grads[3 * k], gy = a.grads[3 * k + 1];
        sum += sqrtf(gx * gx + gy * gy);
        rmax = r > rmax ? r : rmax;  // (float)max = max of the floats: the conversion is monotone
        seen++;
    }
    if (seen == 0) return;  // invisible in every view: its rows stay as they are
    a.accum[i * a.accum_stride] = sum;
    a.max_radii[i] = fmaxf(a.max_radii[i], (float)rmax);
    // V <= 16 visits: successive "+= 1" in float, as the per-view updates add them
    float d = a.denom[i * a.denom_stride];
    for (int k = 0; k < seen; k++) d += 1.f;
    a.denom[i * a.denom_stride] = d;
    if (a.visible_count) {
        float c = a.visible_count[i];
        for (int k = 0; k < seen; k++) c += 1.f;
        a.visible_count[i] = c;
    }
}

hipError_t launch_densify_stats(const DensifyStatsArgs& a, hipStream_t s)
{
    if (a.P <= 0 || a.V <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((size_t)a.P + 255) / 256);
    hipLaunchKernelGGL(densify_stats_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace gsr
