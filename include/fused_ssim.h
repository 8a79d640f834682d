/*
 * fused_ssim.h -- C ABI of the fused SSIM map (libgsr_hip.so, csrc/ssim.hip): the drop-in
 * behind the reference's optional `fused_ssim` module (submodule fused-ssim, un-vendored;
 * used by train.py:31-35,121-124) and the `fusedssim` / `fusedssim_backward` ops that
 * utils/loss_utils.py:17-38 imports from diff_gaussian_rasterization._C.
 *
 * Semantics: the reference's PyTorch SSIM (utils/loss_utils.py:56-86) -- 11x11 Gaussian window
 * (sigma 1.5), zero ("same") padding, per plane.  Images are float32 [planes, H, W] device
 * arrays (planes = batch x channels).  Same conventions as gsr.h: explicit stream, int status
 * + gsr_last_error(), nothing throws.
 */
#ifndef FUSED_SSIM_H_INCLUDED
#define FUSED_SSIM_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ssim_map = SSIM(img1, img2) per pixel.  With dm_dmu1 / dm_dsigma1_sq / dm_dsigma12 all
 * non-NULL (training), also writes the map's partial derivatives the backward needs:
 * d map / d mu1 (including mu1's share in sigma1_sq and sigma12), d map / d sigma1_sq and
 * d map / d sigma12. */
int gsr_ssim_forward(int planes, int H, int W, float C1, float C2, const float* img1, const float* img2,
                     float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream);

/* dL_dimg1 from dL_dmap and the forward's partial derivatives. */
int gsr_ssim_backward(int planes, int H, int W, float C1, float C2, const float* img1, const float* img2,
                      const float* dL_dmap, const float* dm_dmu1, const float* dm_dsigma1_sq,
                      const float* dm_dsigma12, float* dL_dimg1, void* stream);

/*
 * Fused photometric loss of V views (train.py:119-124 for a batch of views):
 *   loss[v] = (1 - lambda_dssim) mean|x_v - gt_v| + lambda_dssim (1 - mean SSIM(x_v, gt_v)),
 * x = img, or clamp(img, 0, 1) with clamp != 0; the means run over the view's C*H*W elements and
 * SSIM is the map of gsr_ssim_forward with C1 = 0.01^2, C2 = 0.03^2.  img, the partial planes and
 * dL_dimg are contiguous (V, C, H, W) device arrays; gt is a HOST array of V device pointers, one
 * (C, H, W) image per view (the ground truths need not be stacked).  1 <= V <= 16.  No atomics:
 * results are bitwise reproducible.  Arguments are validated before any HIP call; a zero size
 * returns GSR_OK.
 */

/* Bytes of the forward's workspace (per-tile partial sums; 0 for a zero or invalid size). */
size_t gsr_photo_loss_workspace_size(int V, int C, int H, int W);

/* loss[V] (device).  With dm_dmu1 / dm_dsigma1_sq / dm_dsigma12 all non-NULL the partial
 * derivative planes for gsr_photo_loss_backward are written too; otherwise nothing but loss. */
int gsr_photo_loss_forward(int V, int C, int H, int W, float lambda_dssim, int clamp, const float* img,
                           const float* const* gt, float* loss, float* dm_dmu1, float* dm_dsigma1_sq,
                           float* dm_dsigma12, void* workspace, void* stream);

/* dL_dimg from the per-view upstream gradients dL_dloss[V] (device; never read by the host) and the
 * forward's planes: the SSIM term plus (1 - lambda_dssim) / (C H W) sign(x - gt) (sign(0) = 0), zero
 * where the clamp is active (img outside [0, 1]). */
int gsr_photo_loss_backward(int V, int C, int H, int W, float lambda_dssim, int clamp, const float* img,
                            const float* const* gt, const float* dL_dloss, const float* dm_dmu1,
                            const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg, void* stream);

#ifdef __cplusplus
}
#endif

#endif
