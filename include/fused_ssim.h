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

/*
 * Fused view loss of V views (train.py:112-141 for a batch of views), from the raw rasterizer outputs:
 *   e_c     = sum_k img_k E_v[k][c] + E_v[c][3]        (exposure: device (V, 3, 4), needs C == 3; NULL: e = img)
 *   x_c     = clamp(e_c, 0, 1) * m_v                    (clamp != 0; alpha_mask[v]: (H, W); NULL: m = 1)
 *   loss[v] = (1 - lambda_dssim) mean|x - gt_v| + lambda_dssim (1 - mean SSIM(x, gt_v))
 *             + depth_weight mean|(invdepth_v - invdepth_target[v]) * depth_mask[v]|
 * The depth term (mean over H*W) is taken for the views with a target, if invdepth (device (V, H, W)) is
 * given and depth_weight > 0.  alpha_mask, invdepth_target and depth_mask are HOST arrays of V device
 * pointers, like gt; the array or any entry may be NULL (that view has none).  Conventions of
 * gsr_photo_loss_*: 1 <= V <= 16, arguments validated before any HIP call, a zero size returns GSR_OK, no
 * atomics (bitwise reproducible), and H*W < 2^30.  Refused: exposure with C != 3, invdepth_target without invdepth,
 * depth_mask without invdepth_target, a negative or non-finite depth_weight.
 */

/* Bytes of the workspace of either pass (per-tile partial sums; 0 for a zero or invalid size). */
size_t gsr_view_loss_workspace_size(int V, int C, int H, int W);

/* loss[V] (device).  With dm_dmu1 / dm_dsigma1_sq / dm_dsigma12 (each (V, C, H, W)) all non-NULL the
 * partial derivative planes for gsr_view_loss_backward are written too; otherwise nothing but loss. */
int gsr_view_loss_forward(int V, int C, int H, int W, float lambda_dssim, int clamp, const float* img,
                          const float* const* gt, const float* exposure, const float* const* alpha_mask,
                          const float* invdepth, const float* const* invdepth_target,
                          const float* const* depth_mask, float depth_weight, float* loss, float* dm_dmu1,
                          float* dm_dsigma1_sq, float* dm_dsigma12, void* workspace, void* stream);

/* From the per-view upstream gradients dL_dloss[V] (device; never read by the host) and the forward's planes:
 *   dL_draw (V, C, H, W): dL/dimg_k = sum_c E[k][c] g_c, g_c = m pass_c dL/dx_c, pass_c = (0 <= e_c <= 1)
 *     with clamp, dL/dx_c the expression of gsr_photo_loss_backward at the masked x (sign(0) = 0);
 *   dL_dexposure (V, 3, 4), required with exposure, ignored without: dL/dE[k][c] = sum_pixels img_k g_c,
 *     dL/dE[c][3] = sum_pixels g_c;
 *   dL_dinvdepth (V, H, W), optional, written only with invdepth:
 *     dL_dloss[v] depth_weight / (H W) sign((invdepth - target) mask) mask, zero for a view without a target.
 * The same inputs as the forward call.  workspace: required with exposure. */
int gsr_view_loss_backward(int V, int C, int H, int W, float lambda_dssim, int clamp, const float* img,
                           const float* const* gt, const float* exposure, const float* const* alpha_mask,
                           const float* invdepth, const float* const* invdepth_target,
                           const float* const* depth_mask, float depth_weight, const float* dL_dloss,
                           const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_draw,
                           float* dL_dexposure, float* dL_dinvdepth, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif
