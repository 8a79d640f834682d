/*
 * gsr.h -- C ABI of the MI355X-native differentiable Gaussian-splatting
 * rasterizer (libgsr_hip.so, built for gfx950).
 *
 * This is the drop-in boundary for the reference's native rasterizer
 * `CudaRasterizer::Rasterizer` (diff-gaussian-rasterization-npu/
 * cuda_rasterizer/rasterizer.h:20-91).  Argument order and meaning follow the
 * reference one-for-one; the differences are C-ABI plumbing only:
 *   - std::function<char*(size_t)> resize lambdas (rasterize_points.cu:27-33)
 *     become a C function pointer + context (gsr_resize_fn);
 *   - every entry point takes the HIP stream it must run on (hipStream_t as
 *     void*; NULL = legacy default stream, as in the reference);
 *   - errors are returned as an int status (0 = ok) with a thread-local
 *     message from gsr_last_error(); nothing throws across the ABI.
 * All data pointers are DEVICE pointers owned by the caller.  Absent optional
 * inputs are NULL, exactly like `.data<float>()` of the empty tensors the
 * reference passes (shs / colors_precomp / scales+rotations / cov3D_precomp,
 * rasterize_points.cu:104-110).  No torch types cross this boundary.
 */
#ifndef GSR_H_INCLUDED
#define GSR_H_INCLUDED

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gsr_stream_t; /* hipStream_t */

/* Resize callback: must return a device pointer to at least `bytes` bytes
 * (rasterize_points.cu:27-33 resizeFunctional). */
typedef char* (*gsr_resize_fn)(void* ctx, size_t bytes);

enum {
    GSR_OK = 0,
    GSR_ERR_INVALID = 1,     /* bad argument / shape                          */
    GSR_ERR_HIP = 2,         /* HIP runtime error (launch, memcpy, sync)      */
    GSR_ERR_ALLOC = 3,       /* a resize callback returned NULL               */
    GSR_ERR_PREFILTERED = 4  /* prefiltered=true but a point was near-culled  */
                             /* (reference: printf + __trap, auxiliary.h:168-172) */
};

/* Thread-local description of the last error returned on this thread. */
const char* gsr_last_error(void);
/* Build identification string ("gsr-hip <version> gfx950"). */
const char* gsr_version(void);

/* Scratch sizes (bytes) of the three opaque state buffers.  They replace
 * required<GeometryState/ImageState/BinningState> (rasterizer_impl.h:67-73). */
size_t gsr_geometry_buffer_size(int P);
size_t gsr_image_buffer_size(int width, int height);
size_t gsr_binning_buffer_size(int num_rendered);

/* Replaces Rasterizer::markVisible (rasterizer.h:24-29; kernel
 * rasterizer_impl.cu:54-66): present[i] = view-space z of point i > 0.2. */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     bool* present, gsr_stream_t stream);

/* Replaces Rasterizer::forward (rasterizer.h:31-55; rasterizer_impl.cu:198-341).
 * Writes out_color (3,H,W), depth = inverse depth (1,H,W) (may be NULL),
 * radii (P) (may be NULL: an internal array is used), and *num_rendered. */
int gsr_forward(gsr_resize_fn geometryBuffer, void* geometry_ctx,
                gsr_resize_fn binningBuffer, void* binning_ctx,
                gsr_resize_fn imageBuffer, void* image_ctx,
                int P, int D, int M,
                const float* background,
                int width, int height,
                const float* means3D,
                const float* shs,
                const float* colors_precomp,
                const float* opacities,
                const float* scales,
                float scale_modifier,
                const float* rotations,
                const float* cov3D_precomp,
                const float* viewmatrix,
                const float* projmatrix,
                const float* cam_pos,
                float tan_fovx, float tan_fovy,
                bool prefiltered,
                float* out_color,
                float* depth,
                bool antialiasing,
                int* radii,
                bool debug,
                gsr_stream_t stream,
                int* num_rendered);

/* Two-phase form of gsr_forward for hosts that own allocation (the Python
 * package): phase 1 = preprocess + tile-count scan + the one D2H of
 * num_rendered (rasterizer_impl.cu:250-284) into caller buffers of
 * gsr_geometry_buffer_size(P) / gsr_image_buffer_size(W,H) bytes; phase 2 =
 * key emission, tile|depth sort, tile ranges and render
 * (rasterizer_impl.cu:286-338) with a binning buffer of
 * gsr_binning_buffer_size(num_rendered) bytes. */
int gsr_forward_geometry(char* geometry_buffer, char* image_buffer,
                         int P, int D, int M, int width, int height,
                         const float* means3D, const float* shs, const float* colors_precomp,
                         const float* opacities, const float* scales, float scale_modifier,
                         const float* rotations, const float* cov3D_precomp,
                         const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                         float tan_fovx, float tan_fovy, bool prefiltered, bool antialiasing,
                         int* radii, bool debug, gsr_stream_t stream, int* num_rendered);

int gsr_forward_render(char* geometry_buffer, char* binning_buffer, char* image_buffer,
                       int P, int num_rendered, const float* background, int width, int height,
                       const float* colors_precomp, float* out_color, float* depth, int* radii,
                       bool debug, gsr_stream_t stream);

/* Both phases in one call when the caller's binning buffer is already big enough:
 * gsr_forward_geometry, then, if gsr_binning_buffer_size(*num_rendered) <=
 * binning_capacity, gsr_forward_render into binning_buffer and *rendered = 1;
 * otherwise *rendered = 0 and the caller allocates the exact size and calls
 * gsr_forward_render itself.  Replaces the allocator round trip between the
 * reference's two halves (binningBuffer resize lambda, rasterizer_impl.cu:286-288)
 * when the host can guess the size, so the GPU does not idle while the host
 * allocates. */
int gsr_forward_prealloc(char* geometry_buffer, char* image_buffer, char* binning_buffer,
                         size_t binning_capacity, int P, int D, int M, const float* background,
                         int width, int height, const float* means3D, const float* shs,
                         const float* colors_precomp, const float* opacities, const float* scales,
                         float scale_modifier, const float* rotations, const float* cov3D_precomp,
                         const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                         float tan_fovx, float tan_fovy, bool prefiltered, bool antialiasing,
                         float* out_color, float* depth, int* radii, bool debug,
                         gsr_stream_t stream, int* num_rendered, int* rendered);

/* Replaces Rasterizer::backward (rasterizer.h:57-90; rasterizer_impl.cu:345-450).
 * dL_dinvdepths / dL_dinvdepth may both be NULL (rasterize_points.cu:174-182).
 * Every output is fully written (zeros for culled Gaussians), so unlike the
 * reference glue (rasterize_points.cu:163-182) the caller need not zero them.
 * The render-pass gradients (dL_dmean2D (P,3), dL_dconic (P,2,2),
 * dL_dopacity (P), dL_dcolor (P,3), dL_dinvdepth (P)) are reduced on chip and
 * gathered per Gaussian in a fixed order: results are bitwise reproducible
 * run to run (the reference sums with float atomics).
 * radii (may be NULL: the forward's own, in geom_buffer) gate each Gaussian as
 * backward.cu:163,420 do; a Gaussian with radius 0 gets zeros in EVERY output,
 * including the render-pass ones the reference would still report from its
 * render backward -- the two agree for radii produced by the forward (radius 0
 * <=> no tile <=> no record).
 * Argument checks (gsr_backward, gsr_backward_dc, gsr_backward_dc_acc alike): P < 0
 * ("P must be >= 0") or R < 0 ("R must be >= 0") is GSR_ERR_INVALID; with P > 0, a
 * NULL means3D or opacities, or a NULL scales or rotations without cov3D_precomp, is
 * GSR_ERR_INVALID ("null parameter array"), a NULL geom_buffer, or with R > 0 a NULL
 * image_buffer, is GSR_ERR_ALLOC ("null state buffer"; a NULL binning_buffer with
 * R > 0: "null binning buffer"), and with R > 0 a NULL dL_dpix is GSR_ERR_INVALID
 * ("null dL_dpix").  P == 0 returns GSR_OK without reading a buffer. */
int gsr_backward(int P, int D, int M, int R,
                 const float* background,
                 int width, int height,
                 const float* means3D,
                 const float* shs,
                 const float* colors_precomp,
                 const float* opacities,
                 const float* scales,
                 float scale_modifier,
                 const float* rotations,
                 const float* cov3D_precomp,
                 const float* viewmatrix,
                 const float* projmatrix,
                 const float* campos,
                 float tan_fovx, float tan_fovy,
                 const int* radii,
                 char* geom_buffer,
                 char* binning_buffer,
                 char* image_buffer,
                 const float* dL_dpix,
                 const float* dL_invdepths,
                 float* dL_dmean2D,
                 float* dL_dconic,
                 float* dL_dopacity,
                 float* dL_dcolor,
                 float* dL_dinvdepth,
                 float* dL_dmean3D,
                 float* dL_dcov3D,
                 float* dL_dsh,
                 float* dL_dscale,
                 float* dL_drot,
                 bool antialiasing,
                 bool debug,
                 gsr_stream_t stream);

/* Separate-DC ("dc=") forms of the four entry points above: the accelerated
 * upstream rasterizer's Rasterizer::forward/backward, which take `dc` (P,1,3,
 * SH coefficient 0) and `shs` (P,M,3, coefficients 1..M) as two arrays and
 * return dL_ddc / dL_dsh separately.  train.py picks that surface whenever the
 * package exports SparseGaussianAdam (train.py:37-41 -> gaussian_renderer/
 * __init__.py:82-100, rasterizer(dc=features_dc, shs=features_rest)), which
 * saves the caller's torch.cat of the two parameter tensors (192 B/Gaussian
 * written and read again) and the split of its gradient.  Here M counts the
 * rest coefficients only (sh.size(1) of features_rest; 15 at degree 3) and may
 * be 0 with shs NULL; dc NULL makes each call identical to its non-dc form. */
int gsr_forward_dc(gsr_resize_fn geometryBuffer, void* geometry_ctx,
                   gsr_resize_fn binningBuffer, void* binning_ctx,
                   gsr_resize_fn imageBuffer, void* image_ctx,
                   int P, int D, int M, const float* background, int width, int height,
                   const float* means3D, const float* dc, const float* shs,
                   const float* colors_precomp, const float* opacities, const float* scales,
                   float scale_modifier, const float* rotations, const float* cov3D_precomp,
                   const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                   float tan_fovx, float tan_fovy, bool prefiltered, float* out_color, float* depth,
                   bool antialiasing, int* radii, bool debug, gsr_stream_t stream, int* num_rendered);

int gsr_forward_geometry_dc(char* geometry_buffer, char* image_buffer,
                            int P, int D, int M, int width, int height,
                            const float* means3D, const float* dc, const float* shs,
                            const float* colors_precomp, const float* opacities, const float* scales,
                            float scale_modifier, const float* rotations, const float* cov3D_precomp,
                            const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                            float tan_fovx, float tan_fovy, bool prefiltered, bool antialiasing,
                            int* radii, bool debug, gsr_stream_t stream, int* num_rendered);

int gsr_forward_prealloc_dc(char* geometry_buffer, char* image_buffer, char* binning_buffer,
                            size_t binning_capacity, int P, int D, int M, const float* background,
                            int width, int height, const float* means3D, const float* dc,
                            const float* shs, const float* colors_precomp, const float* opacities,
                            const float* scales, float scale_modifier, const float* rotations,
                            const float* cov3D_precomp, const float* viewmatrix,
                            const float* projmatrix, const float* cam_pos, float tan_fovx,
                            float tan_fovy, bool prefiltered, bool antialiasing, float* out_color,
                            float* depth, int* radii, bool debug, gsr_stream_t stream,
                            int* num_rendered, int* rendered);

int gsr_backward_dc(int P, int D, int M, int R, const float* background, int width, int height,
                    const float* means3D, const float* dc, const float* shs,
                    const float* colors_precomp, const float* opacities, const float* scales,
                    float scale_modifier, const float* rotations, const float* cov3D_precomp,
                    const float* viewmatrix, const float* projmatrix, const float* campos,
                    float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer,
                    char* binning_buffer, char* image_buffer, const float* dL_dpix,
                    const float* dL_invdepths, float* dL_dmean2D, float* dL_dconic,
                    float* dL_dopacity, float* dL_dcolor, float* dL_dinvdepth, float* dL_dmean3D,
                    float* dL_dcov3D, float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot,
                    bool antialiasing, bool debug, gsr_stream_t stream);

/* gsr_backward_dc with in-place gradient accumulation: for every GSR_ACC_* bit set
 * in `accumulate`, the matching parameter-gradient array is ADDED to (out += this
 * call's gradient, one fp32 add per element, as autograd's AccumulateGrad does
 * `grad += new`) instead of overwritten.  A multi-view step (several views'
 * backward passes into one gradient buffer) then costs no separate
 * accumulation pass over the 236 B/Gaussian of gradients.  The render-pass outputs
 * (dL_dmean2D, dL_dconic, dL_dinvdepth) are always written. */
enum {
    GSR_ACC_MEANS3D = 1, GSR_ACC_DC = 2, GSR_ACC_SH = 4, GSR_ACC_OPACITY = 8, GSR_ACC_SCALES = 16,
    GSR_ACC_ROTATIONS = 32, GSR_ACC_COV3D = 64, GSR_ACC_COLORS = 128, GSR_ACC_ALL = 255
};
int gsr_backward_dc_acc(int P, int D, int M, int R, const float* background, int width, int height,
                        const float* means3D, const float* dc, const float* shs,
                        const float* colors_precomp, const float* opacities, const float* scales,
                        float scale_modifier, const float* rotations, const float* cov3D_precomp,
                        const float* viewmatrix, const float* projmatrix, const float* campos,
                        float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer,
                        char* binning_buffer, char* image_buffer, const float* dL_dpix,
                        const float* dL_invdepths, float* dL_dmean2D, float* dL_dconic,
                        float* dL_dopacity, float* dL_dcolor, float* dL_dinvdepth, float* dL_dmean3D,
                        float* dL_dcov3D, float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot,
                        bool antialiasing, bool debug, unsigned accumulate, gsr_stream_t stream);

/* Backward of a batch of V <= 16 camera views rendered from the same Gaussians (each with its
 * own gsr_forward* call and state buffers): per view BACKWARD::render (rasterizer_impl.cu:399-418),
 * then ONE pass of BACKWARD::preprocess over the Gaussians that reads each Gaussian's parameters
 * once, walks the V views' records and writes the parameter gradients summed over the views
 * (the views' loss terms add up) -- instead of V passes that each read the 236 B/Gaussian of
 * parameters and write (or accumulate) the 236 B/Gaussian of gradients.  Per-view arrays hold
 * one device pointer per view (viewmatrices, projmatrices, campos, radii (may be NULL: the
 * forward's internal copy), state buffers, dL_dpix, dL_invdepths (NULL: no invdepth term in
 * any view), dL_dmean2D: each view's (P,3) screen-space gradient); R, tan_fovx and tan_fovy are
 * host arrays.  dL_dcolor (may be NULL) and the parameter gradients are the sums over the views;
 * `accumulate` as in gsr_backward_dc_acc.  Results equal the sum of V gsr_backward_dc calls up to
 * fp32 summation order.
 * radii: accepted for the reference's argument list but NOT read -- the batched preprocess
 * backward (and gsr_backward_preprocess_views / _range below) takes a Gaussian's visibility in a
 * view from that view's forward state (its tiles_touched, i.e. radius > 0 as the forward computed
 * it), where the reference gates on the radii passed in (backward.cu:163,420).  The two agree for
 * radii produced by the forward; a caller that edits radii between forward and backward has that
 * edit ignored here (the single-view gsr_backward* entry points do read radii).
 * Argument checks of the batched backward entry points (this one, its halves below and
 * gsr_backward_camera_views): V outside [1, 16], P < 0 or a NULL per-view array is GSR_ERR_INVALID.
 * This entry point and its halves return GSR_OK for P == 0 without reading an element of a per-view
 * array, so the per-view checks that follow apply to them with P > 0 only; gsr_backward_camera_views
 * has no such return (it writes its zeros for P == 0) and applies the first two for every P.
 * Per view: R[v] < 0 ("R must be >= 0"), a NULL viewmatrices[v], projmatrices[v] or campos[v]
 * ("null camera") and a NULL per-view gradient are GSR_ERR_INVALID; with P > 0 a NULL means3D or
 * opacities, or a NULL scales or rotations without cov3D_precomp, is GSR_ERR_INVALID ("null parameter
 * array"), and a NULL geom_buffers[v] or image_buffers[v] of any view, or a NULL binning_buffers[v]
 * of a view with R[v] > 0, is GSR_ERR_ALLOC ("null state buffer"). */
int gsr_backward_views(int V, int P, int D, int M, const int* R, const float* background, int width, int height,
                       const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
                       const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                       const float* cov3D_precomp, const float* const* viewmatrices,
                       const float* const* projmatrices, const float* const* campos, const float* tan_fovx,
                       const float* tan_fovy, const int* const* radii, char* const* geom_buffers,
                       char* const* binning_buffers, char* const* image_buffers, const float* const* dL_dpix,
                       const float* const* dL_invdepths, float* const* dL_dmean2D, float* dL_dcolor,
                       float* dL_dopacity, float* dL_dmean3D, float* dL_dcov3D, float* dL_ddc, float* dL_dsh,
                       float* dL_dscale, float* dL_drot, bool antialiasing, bool debug, unsigned accumulate,
                       gsr_stream_t stream);

/* The two halves of gsr_backward_views, for callers that run each view's backward as soon as its
 * image gradient exists and the parameter gradients once per batch (diff_gaussian_rasterization.
 * deferred_backward: view v's render backward beside view v+1's forward on another stream).
 * gsr_backward_render: BACKWARD::render of one view (rasterizer_impl.cu:399-418) -- its
 * per-(tile, Gaussian) gradient records into its binning buffer, nothing else.
 * gsr_backward_preprocess_views: BACKWARD::preprocess (rasterizer_impl.cu:423-449) of V <= 16
 * such views in one pass over the Gaussians, arguments as gsr_backward_views; has_invdepth: some
 * view's render backward had an inverse-depth gradient.  Running the first for every view and then
 * the second equals gsr_backward_views bit for bit. */
int gsr_backward_render(int P, int R, const float* background, int width, int height, char* geom_buffer,
                        char* binning_buffer, char* image_buffer, const float* dL_dpix, const float* dL_invdepths,
                        bool debug, gsr_stream_t stream);
int gsr_backward_preprocess_views(int V, int P, int D, int M, const int* R, int width, int height,
                                  const float* means3D, const float* dc, const float* shs,
                                  const float* colors_precomp, const float* opacities, const float* scales,
                                  float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                  const float* const* viewmatrices, const float* const* projmatrices,
                                  const float* const* campos, const float* tan_fovx, const float* tan_fovy,
                                  const int* const* radii, char* const* geom_buffers, char* const* binning_buffers,
                                  bool has_invdepth, float* const* dL_dmean2D, float* dL_dcolor, float* dL_dopacity,
                                  float* dL_dmean3D, float* dL_dcov3D, float* dL_ddc, float* dL_dsh,
                                  float* dL_dscale, float* dL_drot, bool antialiasing, bool debug,
                                  unsigned accumulate, gsr_stream_t stream);
/* gsr_backward_render_views: the BACKWARD::render half of gsr_backward_views for all V views (one
 * tile-order launch and one render launch per batch).  gsr_backward_preprocess_views_range: the
 * BACKWARD::preprocess half restricted to the Gaussians [g_begin, g_end) -- only their rows of the
 * parameter gradients (and of each view's dL_dmean2D) are written, so a caller can hand finished
 * row ranges to a gradient all-reduce while the next range computes (the collective
 * overlapped with the backward).  Chunks covering [0, P) equal one full call bit for bit. */
int gsr_backward_render_views(int V, int P, const int* R, const float* background, int width, int height,
                              char* const* geom_buffers, char* const* binning_buffers, char* const* image_buffers,
                              const float* const* dL_dpix, const float* const* dL_invdepths, bool debug,
                              gsr_stream_t stream);
int gsr_backward_preprocess_views_range(int V, int P, int D, int M, const int* R, int width, int height,
                                        const float* means3D, const float* dc, const float* shs,
                                        const float* colors_precomp, const float* opacities, const float* scales,
                                        float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                        const float* const* viewmatrices, const float* const* projmatrices,
                                        const float* const* campos, const float* tan_fovx, const float* tan_fovy,
                                        const int* const* radii, char* const* geom_buffers,
                                        char* const* binning_buffers, bool has_invdepth, float* const* dL_dmean2D,
                                        float* dL_dcolor, float* dL_dopacity, float* dL_dmean3D, float* dL_dcov3D,
                                        float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                        bool antialiasing, bool debug, unsigned accumulate, int g_begin, int g_end,
                                        gsr_stream_t stream);

/* The alpha output, alpha = 1 - final_T per pixel: the opacity a pixel accumulated, i.e. the
 * reference's render with colour 1 and background 0 (FORWARD::render, forward.cu:277-400: T behind
 * the last contributor, the `final_T` that the forward keeps for the backward).  The reference does
 * not return it; a silhouette or mask loss and compositing over a per-iteration background need it.
 * gsr_alpha_views: valid after any forward (gsr_forward*, gsr_forward_render, gsr_forward_views) into
 * those image buffers, before the next forward into them; it only reads the state.  Per-view host
 * arrays of V device pointers: image_buffers, and out_alphas (H*W floats each), every one fully
 * written -- zeros for a view with num_rendered == 0, whose final_T is 1.  One elementwise launch
 * per 8 views (8 B per pixel).  V outside [1, 16], width or height <= 0, a NULL array or a NULL
 * element: GSR_ERR_INVALID, before any HIP call.  (P == 0 forwards return before they write the
 * image state: there is no alpha to read.)  Asynchronous; never throws (status + gsr_last_error). */
int gsr_alpha_views(int V, int width, int height, char* const* image_buffers, float* const* out_alphas,
                    gsr_stream_t stream);

/* The backward entry points with a gradient on the alpha output: gsr_backward_alpha is
 * gsr_backward_dc_acc, gsr_backward_views_alpha is gsr_backward_views and
 * gsr_backward_render_views_alpha is gsr_backward_render_views (with V = 1: gsr_backward_render),
 * each with dL_dalphas directly after dL_invdepths -- (H,W) floats, the loss's gradient with respect
 * to gsr_alpha_views' output of that view; for the batched two a host array of V device pointers.
 * BACKWARD::render (backward.cu:601-612) gives dL/dalpha_j the background's term
 * -T_final / (1 - alpha_j) (bg . dL/dpixel); d(1 - T_final)/dalpha_j = +T_final / (1 - alpha_j), so the
 * alpha gradient enters as bg . dL/dpixel - dL_dalphas in that term and nowhere else: the gradient
 * records, and with them the parameter gradients, dL_dmean2D and gsr_backward_camera_views' outputs,
 * carry it with no further argument.  dL_dalphas NULL (for the batched two also any element NULL,
 * views with and without one mixed freely): that view has no alpha term and gets the bits the entry
 * point without the argument gives; those entry points pass NULL here and are otherwise this code.
 * Argument checks, return codes and messages are those of gsr_backward_dc_acc, gsr_backward_views and
 * gsr_backward_render_views; no check is added for dL_dalphas.  Asynchronous; never throw (status +
 * gsr_last_error). */
int gsr_backward_alpha(int P, int D, int M, int R, const float* background, int width, int height,
                       const float* means3D, const float* dc, const float* shs,
                       const float* colors_precomp, const float* opacities, const float* scales,
                       float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* campos,
                       float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer,
                       char* binning_buffer, char* image_buffer, const float* dL_dpix,
                       const float* dL_invdepths, const float* dL_dalphas, float* dL_dmean2D,
                       float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dinvdepth,
                       float* dL_dmean3D, float* dL_dcov3D, float* dL_ddc, float* dL_dsh, float* dL_dscale,
                       float* dL_drot, bool antialiasing, bool debug, unsigned accumulate, gsr_stream_t stream);
int gsr_backward_views_alpha(int V, int P, int D, int M, const int* R, const float* background, int width, int height,
                             const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
                             const float* opacities, const float* scales, float scale_modifier,
                             const float* rotations, const float* cov3D_precomp, const float* const* viewmatrices,
                             const float* const* projmatrices, const float* const* campos, const float* tan_fovx,
                             const float* tan_fovy, const int* const* radii, char* const* geom_buffers,
                             char* const* binning_buffers, char* const* image_buffers, const float* const* dL_dpix,
                             const float* const* dL_invdepths, const float* const* dL_dalphas,
                             float* const* dL_dmean2D, float* dL_dcolor, float* dL_dopacity, float* dL_dmean3D,
                             float* dL_dcov3D, float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot,
                             bool antialiasing, bool debug, unsigned accumulate, gsr_stream_t stream);
int gsr_backward_render_views_alpha(int V, int P, const int* R, const float* background, int width, int height,
                                    char* const* geom_buffers, char* const* binning_buffers,
                                    char* const* image_buffers, const float* const* dL_dpix,
                                    const float* const* dL_invdepths, const float* const* dL_dalphas, bool debug,
                                    gsr_stream_t stream);

/* The camera gradient of V <= 16 views: dL/dviewmatrix, dL/dprojmatrix and dL/dcampos of each view,
 * which no other entry point returns (the reference treats the camera as a constant).  Called after
 * the views' render backward (gsr_backward*, gsr_backward_render or gsr_backward_render_views), before
 * or after their preprocess backward, and before the next forward into the same state buffers; it
 * only reads the state (the gradient records stay valid until then).  Arguments as
 * gsr_backward_preprocess_views; a Gaussian counts for a view iff the forward gave it tiles there
 * (the forward state, not a caller's radii).
 * With V = viewmatrix and Pm = projmatrix as stored, row-major (4,4) as torch stores them
 * (t = [m,1] V the view-space mean, p_hom = [m,1] Pm), mh = (m.x, m.y, m.z, 1), and the factors
 * BACKWARD::preprocess forms per visible Gaussian (backward.cu:147-326, 423-440):
 *   dL/dV[r][c]  = sum_i mh[r] dL/dt[c]                                   r 0..3, c 0..2
 *                + sum_i sum_a dL/dT[a][r] J[a][c]                        r, c 0..2
 *     dL/dt: the reference's dL_dtx, dL_dty, dL_dtz (clamp multipliers and inverse-depth term
 *     included); T = J V[:3,:3]^T the 2x3 factor of cov2D = T cov3D T^T with dL/dT the reference's
 *     dL_dT00 .. dL_dT12; J = [[fx/tz, 0, -fx tx/tz^2], [0, fy/tz, -fy ty/tz^2]] with the clamped tx, ty;
 *   dL/dPm[r][c] = sum_i mh[r] dL/dp_hom[c],
 *     dL/dp_hom = (m_w g2x, m_w g2y, 0, -(mul1 g2x + mul2 g2y)), g2 = dL/dmean2D, m_w = 1/(p_hom.w + 1e-7),
 *     mul1 = p_hom.x m_w^2, mul2 = p_hom.y m_w^2;
 *   dL/dcampos   = -sum_i (the view-direction term of dL/dmean3D: computeColorFromSH's backward,
 *     backward.cu:103-141); zero with colors_precomp or degree 0.
 * Column 3 of dL/dV and column 2 of dL/dPm are written as zeros.  The three outputs (device memory:
 * V*16, V*16 and V*3 floats) are fully written, also for P == 0 (zeros).  workspace:
 * gsr_camera_grad_workspace_size(V, P) bytes of device memory, 4-byte aligned, contents irrelevant on
 * entry (monotone in V and P).  No atomics: the sums are bitwise reproducible, and a view's are the
 * same bits alone or inside a batch.  V outside [1, 16], P < 0, a NULL output, workspace or per-view
 * array: GSR_ERR_INVALID.  Asynchronous; never throws (status + gsr_last_error). */
size_t gsr_camera_grad_workspace_size(int V, int P);
int gsr_backward_camera_views(int V, int P, int D, int M, const int* R, int width, int height, const float* means3D,
                              const float* dc, const float* shs, const float* colors_precomp,
                              const float* opacities, const float* scales, float scale_modifier,
                              const float* rotations, const float* cov3D_precomp, const float* const* viewmatrices,
                              const float* const* projmatrices, const float* const* campos, const float* tan_fovx,
                              const float* tan_fovy, char* const* geom_buffers, char* const* binning_buffers,
                              bool has_invdepth, bool antialiasing, char* workspace,
                              float* dL_dviewmatrix /* V*16 */, float* dL_dprojmatrix /* V*16 */,
                              float* dL_dcampos /* V*3 */, bool debug, gsr_stream_t stream);

/* Forward of a batch of V <= 16 camera views of the same Gaussians (the forward half of
 * gsr_backward_views; each view the result of gsr_forward_prealloc_dc with its own state buffers).
 * Every stage is ONE launch over up to 8 views (grid.y = view), on an internal high-priority
 * stream: preprocess (the Gaussians' parameters read once for the batch; GeometryState's means2D,
 * depths and rgb, read by nothing downstream, are not written), the record-slot scans (beside the
 * depth sorts, on an auxiliary stream), the depth sorts, the tile-count scans; then every view's
 * num_rendered is read back (the one host hand-off, rasterizer_impl.cu:283-284); then the tile
 * sorts with the instance emission fused into their first pass, tile ranges, tile orders, and on
 * the caller's stream one render launch for the views (one launch tail per batch).  Per-view arrays hold one pointer per view
 * (viewmatrices, projmatrices, campos, the three state buffers, out_colors (3,H,W), out_invdepths
 * (1,H,W), radii (P) -- radii may be NULL); tan_fovx, tan_fovy, binning_capacity, num_rendered and
 * rendered are host arrays.  rendered[v] = 0: view v's binning buffer was NULL or smaller than
 * gsr_binning_buffer_size(num_rendered[v]) -- the caller allocates that and finishes the view with
 * gsr_forward_render.  Every result is bit-identical to the single-view call's. */
int gsr_forward_views(int V, int P, int D, int M, const float* background, int width, int height,
                      const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
                      const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                      const float* cov3D_precomp, const float* const* viewmatrices, const float* const* projmatrices,
                      const float* const* campos, const float* tan_fovx, const float* tan_fovy, bool prefiltered,
                      bool antialiasing, char* const* geometry_buffers, char* const* image_buffers,
                      char* const* binning_buffers, const size_t* binning_capacity, float* const* out_colors,
                      float* const* out_invdepths, int* const* radii, bool debug, gsr_stream_t stream,
                      int* num_rendered, int* rendered);

/* Visibility-masked Adam step (the accelerated upstream's `_C.adamUpdate`, called
 * by SparseGaussianAdam.step(visibility, N) from train.py:180-183): for each of the
 * N Gaussians with visible[i] set, its M consecutive elements of param are updated
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  param -= lr m / (sqrt(v) + eps)
 * (no bias correction); other rows are left untouched.  N*M < 2^32. */
int gsr_adam_update(float* param, const float* param_grad, float* exp_avg, float* exp_avg_sq,
                    const bool* visible, float lr, float b1, float b2, float eps, int N, int M,
                    gsr_stream_t stream);

/* The same step for n_groups parameter tensors sharing one visibility mask (one
 * SparseGaussianAdam.step over its per-attribute groups, scene/gaussian_model.py:
 * 181-196) in a single launch: group i has Ms[i] elements per Gaussian, learning
 * rate lrs[i] and epsilon epss[i].  Per group identical to gsr_adam_update. */
int gsr_adam_update_multi(int n_groups, float* const* params, const float* const* param_grads,
                          float* const* exp_avgs, float* const* exp_avg_sqs, const int* Ms,
                          const float* lrs, const float* epss, const bool* visible, float b1,
                          float b2, int N, gsr_stream_t stream);

/* train.py's densification statistics (train.py:166, gaussian_model.py:471-473) for V views of
 * the same P Gaussians in one launch, without a host synchronisation.  For every Gaussian i and
 * v = 0 .. V-1 in order, where radii[v*P + i] > 0:
 *   max_radii2D[i] = max(max_radii2D[i], (float)radii[v*P + i]);
 *   accum[i*accum_stride] += sqrt(gx^2 + gy^2), (gx, gy) = viewspace_grads[(v*P + i)*3 + 0..1];
 *   denom[i*denom_stride] += 1;  visible_count[i] += 1 (when visible_count is not NULL).
 * The strides count floats and are >= 1 (accum and denom may be columns of one (P,2) buffer).
 * Gaussians no view sees are not written. */
int gsr_densification_stats(int V, int P, const float* viewspace_grads, const int* radii, float* max_radii2D,
                            float* accum, long accum_stride, float* denom, long denom_stride,
                            float* visible_count, gsr_stream_t stream);

/* The parameter activations between the optimizer's raw tensors and the rasterizer
 * (GaussianModel.get_scaling / get_rotation / get_opacity, gaussian_model.py:102-135) for P Gaussians in
 * one launch.  For every Gaussian i, in fp32 without contraction:
 *   scales[3i+k]    = expf(scaling[3i+k]);
 *   opacities[i]    = 1 / (1 + expf(-opacity[i]));
 *   n = sqrtf(sum_k q_k^2), d = fmaxf(n, 1e-12f), rotations[4i+k] = q_k / d,   q = rotation[4i ..]
 * (torch.nn.functional.normalize's x / max(|x|_2, eps) with its default eps 1e-12).  All six arrays
 * are device memory, contiguous, 4-byte aligned; no output may overlap an input or another output.
 * P == 0: nothing is launched.  P < 0 or a NULL pointer: GSR_ERR_INVALID.  Asynchronous. */
int gsr_activate_forward(int P, const float* scaling, const float* rotation, const float* opacity,
                         float* scales, float* rotations, float* opacities, gsr_stream_t stream);

/* The backward of gsr_activate_forward: the chain rule torch's autograd applies to the same three ops,
 * from the forward's OUTPUTS scales and opacities and the raw quaternions `rotation`:
 *   dL_dscaling[3i+k]  = dL_dscales[3i+k] * scales[3i+k];
 *   dL_dopacity[i]     = dL_dopacities[i] * (1 - y) * y,  y = opacities[i];
 *   n, d as above, r = q / d, m = (n >= 1e-12f):
 *   dL_drotation[4i+k] = (g_k - m r_k (r . g)) / d,  g = dL_drotations[4i ..]
 * (m is clamp_min's mask: a quaternion shorter than eps, the zero one included, gets g / eps).
 * Group g (0 scaling, 1 rotation, 2 opacity) is skipped -- nothing of it is read or written -- when its
 * incoming gradient or its destination is NULL.  Bit g of accumulate_mask selects `+=` for that
 * group's destination (one fp32 add per element, the arithmetic of autograd's AccumulateGrad; the
 * contract of gsr_backward_dc_acc); otherwise it is overwritten.  Destinations need only 4-byte
 * alignment (views of a flat gradient buffer at any float offset) and must not overlap an input or
 * each other.  P == 0: nothing is launched.  P < 0 or unknown mask bits: GSR_ERR_INVALID.
 * Asynchronous; results are bitwise reproducible. */
int gsr_activate_backward(int P, const float* scales, const float* rotation, const float* opacities,
                          const float* dL_dscales, const float* dL_drotations, const float* dL_dopacities,
                          float* dL_dscaling, float* dL_drotation, float* dL_dopacity,
                          int accumulate_mask, gsr_stream_t stream);

/* GaussianModel.densify_and_prune (gaussian_model.py:402-469) in two calls: gsr_densify_plan decides
 * what becomes of each of the P Gaussians and returns the counts the caller needs to allocate the new
 * tensors and to draw the split's samples; gsr_densify_apply writes the new tensors.  For source row i:
 *   g     = accum[i*accum_stride] / denom[i*denom_stride], 0 where that is NaN;
 *   smax  = max_k expf(scaling[3i+k]);
 *   clone = g >= max_grad && smax <= dense_extent;    split = g >= max_grad && smax > dense_extent;
 *   low   = 1/(1 + expf(-opacity[i])) < min_opacity;
 *   big   = big_extent >= 0 && smax > big_extent;
 *   bigchild = big_extent >= 0 && max_k expf(logf(expf(scaling[3i+k]) / (0.8 N))) > big_extent.
 * (The reference's screen-size test never fires -- max_radii2D is zeroed before it is read -- and is
 * not part of this.)  Output rows, each run in source order: the rows with !split && !(low || big);
 * the clones of the rows with clone && !(low || big); then, for r = 0 .. N-1, child r of every row with
 * split && !(low || bigchild).  Child r of row i, the j-th of ALL split rows (pruned ones included), has
 *   xyz     = R(rotation_i / |rotation_i|) (expf(scaling_i) * z) + xyz_i,  z = samples[3 (r n_split + j) ..],
 *   scaling = logf(expf(scaling_i) / (0.8 N)),
 * (R: the rotation matrix of a wxyz quaternion) and row i's values in every other group.  Adam
 * moments are copied for the surviving rows and zero for clones and children.
 *
 * gsr_densify_workspace_size: bytes of device memory both calls need for P Gaussians (0 for P <= 0).
 * gsr_densify_rows_per_workgroup: source rows one workgroup of the plan's scan covers. */
size_t gsr_densify_workspace_size(int P);
int gsr_densify_rows_per_workgroup(void);

/* The plan.  accum, denom: device, read with element strides >= 1 (columns of one (P,2) buffer, or
 * arrays of their own); scaling (P,3) log scales and opacity (P) logits: device, contiguous.
 * max_grad, dense_extent (percent_dense x scene extent), min_opacity: the thresholds above;
 * big_extent: the world-size threshold (0.1 x extent), or < 0 for none; N >= 1: children per split
 * row.  workspace: gsr_densify_workspace_size(P) bytes of device memory, 256-byte aligned, kept
 * unchanged until gsr_densify_apply has run.  counts: FOUR host ints, written before the call
 * returns: the rows with clone, the rows with split (= n_split), the rows the final prune removes
 * (a pruned split row counts N times, a pruned cloned row twice) and the new row count P_after.
 * Synchronises `stream` once.  P == 0: counts are zero, nothing is launched. */
int gsr_densify_plan(int P, const float* accum, long accum_stride, const float* denom, long denom_stride,
                     const float* scaling, const float* opacity, float max_grad, float dense_extent,
                     float min_opacity, float big_extent, int N, char* workspace, int* counts,
                     gsr_stream_t stream);

/* The apply, after gsr_densify_plan with the same P, N and workspace on the same stream; P_after and
 * n_split are that call's counts[3] and counts[1] (when they do not match the plan in the workspace,
 * nothing is written).  n_groups <= 8 parameter tensors of Ms[g] floats per row; xyz_group,
 * scaling_group, rotation_group: which of them are the positions (3 floats), log scales (3) and wxyz
 * quaternions (4).  src[g]: the (P, Ms[g]) tensor; dst[g]: the (P_after, Ms[g]) tensor to write; src_m /
 * src_v and dst_m / dst_v: the group's Adam moments likewise -- a group with dst_m[g] and dst_v[g]
 * NULL has no moments (the six arrays themselves are never NULL).  Host arrays of device pointers,
 * all contiguous; no output may overlap an input.  samples: (N n_split, 3) standard normal draws on the
 * device, NULL iff n_split == 0.  P == 0 or P_after == 0: nothing is launched.  Asynchronous. */
int gsr_densify_apply(int P, int P_after, int n_split, int N, int n_groups, const int* Ms, int xyz_group,
                      int scaling_group, int rotation_group, const float* const* src,
                      const float* const* src_m, const float* const* src_v, float* const* dst,
                      float* const* dst_m, float* const* dst_v, const float* samples, const char* workspace,
                      gsr_stream_t stream);

/* Visibility-compacted gradient exchange for data-parallel steps.  A Gaussian no view of a step saw on
 * any rank has a zero gradient row on every rank, so the SUM over the ranks needs only the union of the
 * ranks' visible rows.  Each rank packs its visibility counts into bits (gsr_visibility_pack), the
 * ranks exchange the words, gsr_union_plan ORs them into the ascending list of union rows, and
 * gsr_rows_gather / gsr_rows_scatter move those rows of every gradient tensor into and out of a
 * compact buffer that the collective then reduces.  Every rank that plans the same words gets the
 * same U and the same list.
 *
 * Bit layout: Gaussian g is bit (g & 31) of word (g >> 5); a row of words has (P + 31) / 32 words;
 * bits at or beyond P are zero.
 * Compact layout: [group][union row][column] -- group k starts at U * (Ms[0] + .. + Ms[k-1]) floats,
 * union row u of it at another u * Ms[k]; U * sum(Ms) floats in all.
 * All device arrays are contiguous and need 4-byte alignment only, except the workspace (256).
 *
 * gsr_union_rows_per_wave: the Gaussians one wave of the plan covers; boundaries are multiples of it.
 * gsr_union_workspace_size: bytes of device memory gsr_union_plan needs for P Gaussians (0 for P <= 0). */
int gsr_union_rows_per_wave(void);
size_t gsr_union_workspace_size(int P);

/* words[w] bit b = (count[32 w + b] > 0) for the P floats of `count` (device); every one of the
 * (P + 31) / 32 words (device) is written in full.  P == 0: nothing is launched.  Asynchronous. */
int gsr_visibility_pack(int P, const float* count, uint32_t* words, gsr_stream_t stream);

/* The plan.  words: (ranks, (P + 31) / 32) device words, one row per rank (ranks >= 1); tail bits at
 * or beyond P are ignored.  workspace: gsr_union_workspace_size(P) bytes of device memory, 256-byte
 * aligned.  rows: P device words; rows[0 .. U) become the union's Gaussians in ascending order, the
 * rest is not written.  mask: P device bytes (1 = in the union), or NULL.  bounds: n_bounds <= 16 HOST
 * ints, each P or a multiple of gsr_union_rows_per_wave() in [0, P].  U and bound_ranks (n_bounds HOST
 * ints: the number of union rows below each boundary, i.e. the boundary's index into rows) are
 * written before the call returns.  Synchronises `stream` once.  P == 0: U and the ranks are zero,
 * nothing is launched.  ranks < 1, more than 16 boundaries or an unaligned boundary:
 * GSR_ERR_INVALID. */
int gsr_union_plan(int P, int ranks, const uint32_t* words, int n_bounds, const int* bounds, char* workspace,
                   uint32_t* rows, uint8_t* mask, int* U, int* bound_ranks, gsr_stream_t stream);

/* compact[group k][u][c] = src[k][rows[u] * Ms[k] + c] for the window u0 <= u < u1 of the U union rows,
 * every group in one launch.  n_groups <= 8; src: HOST array of device pointers to the (P, Ms[k])
 * tensors; a group with Ms[k] == 0 is skipped (its pointer may be NULL).  rows: gsr_union_plan's list;
 * an entry >= P is skipped.  compact: U * sum(Ms) device floats; only the window's elements are
 * written.  U * Ms[k] < 2^32 - 16.  P == 0, U == 0 or an empty window: nothing is launched.  A window
 * outside [0, U], U > P or more than 8 groups: GSR_ERR_INVALID.  Asynchronous. */
int gsr_rows_gather(int P, int U, int u0, int u1, int n_groups, const int* Ms, const float* const* src,
                    const uint32_t* rows, float* compact, gsr_stream_t stream);

/* The inverse: dst[k][rows[u] * Ms[k] + c] = compact[group k][u][c] for u0 <= u < u1.  Only the union
 * rows of the window are written; no other row of dst is touched.  Arguments and refusals as
 * gsr_rows_gather.  Asynchronous. */
int gsr_rows_scatter(int P, int U, int u0, int u1, int n_groups, const int* Ms, float* const* dst,
                     const uint32_t* rows, const float* compact, gsr_stream_t stream);

/* Where the forward's binning prefix (preprocess .. tile order) runs.  on = 1: on an internal
 * stream of the highest priority, forked from and joined back into the caller's stream, its side
 * work (record-slot scan, tile histogram, forward tile order) on a second internal stream;
 * on = 2: on the caller's stream, the side work on the internal one (no join before render_fwd);
 * on = 0: every launch on the caller's stream.  Other values: GSR_ERR_INVALID.  Per host
 * thread; the default is 1. */
int gsr_set_prefix_stream(int on);

/* Debug / parity helper: writes the sorted 64-bit tile|depth keys
 * (rasterizer_impl.cu:102-104 layout, after the sort of :306-311) and the
 * sorted Gaussian ids of the last forward held in these buffers. */
int gsr_debug_sorted_keys(const char* geometry_buffer, const char* binning_buffer, const char* image_buffer,
                          int P, int num_rendered, int width, int height,
                          uint64_t* keys_out, uint32_t* vals_out, uint32_t* ranges_out,
                          gsr_stream_t stream);

/* Debug / parity helper: the forward's depth sort alone (the first half of the
 * rasterizer_impl.cu:306-311 key sort): out_ids = the stable order of n u32 keys
 * (the forward's depth keys: float bit patterns, 0xFFFFFFFF = culled, sorted
 * last).
 * workspace: gsr_debug_depth_sort_workspace_size(n) device bytes. */
size_t gsr_debug_depth_sort_workspace_size(int n);
int gsr_debug_depth_sort(const uint32_t* keys, int n, uint32_t* out_ids, char* workspace, gsr_stream_t stream);

/* The depth sort runs three 9-bit passes, the third relative to the smallest visible key; in a forward
 * whose visible depth keys span too wide a range for that (depths beyond a factor of ~2^16) that
 * view's depth sort and tile-count scan run again in four 8-bit passes -- for that call only, no
 * state is kept (the reference's sort is stateless, rasterizer_impl.cu:306-311).
 * Test hooks: gsr_debug_set_depth_wide(1) forces four passes for every depth sort of the calling host
 * thread (0 releases it; gsr_debug_depth_wide reads it); gsr_debug_last_depth_passes(v) = the passes
 * the final depth sort of view v of this thread's last forward ran (3, or 4 after a re-run or when
 * forced; 0 before any forward). */
int gsr_debug_depth_wide(void);
int gsr_debug_set_depth_wide(int on);
int gsr_debug_last_depth_passes(int view);

/* Floats per per-instance gradient record in the binning buffer's GRAD_INST region (10 = 40 B),
 * for diagnostics that decode the records. */
int gsr_debug_grad_record_floats(void);

/* Byte offsets of the arrays inside each opaque state buffer (n entries
 * written, count of arrays returned; entry [count] is the total size).  For
 * parity tests and debugging only; the layout is private to this library. */
int gsr_geometry_layout(int P, size_t* offsets, int n);
int gsr_image_layout(int width, int height, size_t* offsets, int n);
int gsr_binning_layout(int num_rendered, size_t* offsets, int n);

/* Per-kernel timing with HIP events recorded on the launch stream (used by
 * bench.py's roofline measurement).  gsr_profile_enable(1) starts recording
 * (and resets); gsr_profile_read waits for the recorded events and returns,
 * per kernel id, the summed milliseconds and launch counts since the last
 * enable/read.  Both return the number of kernel ids. */
int gsr_profile_enable(int on);
int gsr_profile_read(double* total_ms, int* counts, int n);
const char* gsr_profile_kernel_name(int kernel_id);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H_INCLUDED */
