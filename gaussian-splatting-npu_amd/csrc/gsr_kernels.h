// gsr_kernels.h -- kernel argument blocks and host launchers (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

struct PreprocessArgs {
    int P, D, M, W, H;
    const float* means3D;
    const float* scales;
    float scale_modifier;
    const float* rotations;
    const float* opacities;
    const float* shs;  // (P,M,3); with dc: the (P,M-1,3) rest coefficients (M counts the dc one)
    const float* dc;   // separate coefficient 0 (P,1,3), or null
    const float* cov3D_precomp;
    const float* colors_precomp;
    const float* view;
    const float* proj;
    const float* campos;
    float tan_fovx, tan_fovy, focal_x, focal_y;
    uint32_t grid_x, grid_y;
    int prefiltered, antialiasing;
    // outputs (means2D, depths, rgb: GeometryState fields nothing downstream reads -- kept for the
    // single-view forward's parity with the reference, null in the batched forward)
    int* radii;
    float* means2D;
    float* depths;
    float* rgb;
    float* conic_opacity;
    uint8_t* clamped;
    uint32_t* tiles_touched;
    uint32_t* host_flags;     // pinned host word: set to 1 on a prefiltered violation (no device memset)
    uint64_t* scan_status;    // look-back status words of the tiles_touched scan, zeroed here
    int scan_status_words;
    float4* splat;  // 3 x float4 per Gaussian (GEOM_SPLAT)
    uint32_t* dkey; // depth-sort key per Gaussian
    uint2* rect;    // {x0 | y0 << 16, x1 | y1 << 16} per Gaussian (zero if culled); null with rect4
    uint32_t* rect4;  // the rect packed (rect_pack) instead, on grids of <= 255 x 255 tiles
    int* tile_diff;   // IMG_TILE_DIFF, zeroed here (tile_hist adds into it), or null
    int tile_diff_words;
    uint32_t* rec_mask;  // GEOM_REC_MASK, zeroed here (render_bwd sets it)
    uint32_t* dsort_gsum;  // the depth sort's chunk-group digit counts (radix_gsum_*), zeroed here, or null
    int dsort_gsum_words;
};

struct RenderFwdArgs {
    const uint2* ranges;
    const uint32_t* tile_order;  // IMG_TILE_ORDER: block b renders tile tile_order[b]
    uint32_t* tile_work;         // IMG_TILE_WORK: largest n_contrib of the tile (out)
    const uint32_t* point_list;
    int W, H;
    uint32_t grid_x;
    const float4* splat;  // GEOM_SPLAT records (xy+extent, conic+opacity, rgb+1/depth)
    const float* bg;
    float* final_T;
    uint32_t* n_contrib;
    float* out_color;
    float* invdepth;
    uint8_t* hit;   // BIN_HIT: contributing quadrants of every processed list entry (out)
};

struct RenderBwdArgs {
    const uint2* ranges;
    const uint32_t* tile_order;  // IMG_TILE_ORDER (re-ordered from IMG_TILE_WORK for the backward)
    const uint32_t* tile_work;   // IMG_TILE_WORK (render_fwd): the tile's largest n_contrib
    const uint32_t* point_list;
    int W, H;
    uint32_t grid_x;
    int T;  // tiles
    const float* bg;
    const float4* splat;
    const float* final_Ts;
    const uint32_t* n_contrib;
    const float* dL_dpixels;
    const float* dL_invdepths;  // (1,H,W) or null
    const float* dL_dalphas;    // (H,W) or null: the gradient on alpha = 1 - final_T (per view, wave-uniform)
    const uint32_t* slot;       // gradient-record slot of each sorted position
    uint32_t* valid;            // bit (slot & 31) of valid[slot >> 5] set for every record written (cleared by emit)
    float* grad_inst;           // f32x10[L]: one gradient record per (tile, Gaussian) entry, at its record slot
    const uint8_t* hit;         // BIN_HIT (render_fwd): the quadrants each entry contributed to
    const uint32_t* emit_start; // GEOM_EMIT_START: first record slot of each Gaussian
    uint32_t* rec_mask;         // GEOM_REC_MASK: bit (slot - emit_start[id]) set for records at local index < 32
};

// Layout of one per-instance gradient record (GRAD_REC floats: 40 B packed).  With u = G dL/dalpha
// per pixel, the mean2D fields hold Sx = sum u dx, Sy = sum u dy and the conic fields
// sum u dx^2, u dx dy, u dy^2 -- WITHOUT the per-Gaussian factors (backward.cu:619-636):
// preprocess_bwd forms dL/dmean2D = (a Sx + b Sy, b Sx + c Sy) * (-opacity W/2, -opacity H/2)
// from the conic (a, b, c) and scales the conic sums by -opacity/2, once per Gaussian.
enum GradField {
    GF_MEAN2D_X = 0, GF_MEAN2D_Y, GF_CONIC_A, GF_CONIC_B, GF_CONIC_C, GF_OPACITY, GF_COLOR_R, GF_COLOR_G,
    GF_COLOR_B, GF_INVDEPTH, GF_NUM
};

// In-place gradient accumulation (gsr_backward_dc_acc): bit set = that output array is added to.
enum AccBits : uint32_t {
    ACC_MEANS3D = 1u, ACC_DC = 2u, ACC_SH = 4u, ACC_OPACITY = 8u, ACC_SCALES = 16u, ACC_ROTATIONS = 32u,
    ACC_COV3D = 64u, ACC_COLORS = 128u
};

struct PreprocessBwdArgs {
    int P, D, M;
    const float* means3D;
    const int* radii;  // the single-view launch: visibility radius > 0 (backward.cu:420); null for batches
    const float* shs;  // as PreprocessArgs: with dc, the rest coefficients and M counts dc
    const float* dc;
    const float* opacities;
    const float* scales;
    const float* rotations;
    float scale_modifier;
    const float* cov3D_precomp;  // null: cov3D is recomputed from scales/rotations
    int antialiasing;
    int has_invdepth;
    int W, H;
    // the single-view launch's other render-pass gradients (outputs of the reference glue; null for batches)
    float* dL_dconic;    // (P,4)
    float* dL_dinvdepth; // (P) or null
    float* dL_dopacity;  // (P)
    float* dL_dcolor;    // (P,3)
    float* dL_dmean3D;
    float* dL_dcov3D;
    float* dL_dsh;
    float* dL_ddc;  // (P,1,3) when dc is given
    float* dL_dscale;
    float* dL_drot;
    uint32_t acc;  // GSR_ACC_* bits (include/gsr.h): outputs added to instead of overwritten
};

// Multi-view backward (gsr_backward_views): one entry per camera view of the batch.  The
// per-Gaussian parameters and their gradients are shared (PreprocessBwdArgs), everything
// view-dependent comes from here; each view's screen-space gradient is written separately.
constexpr int MAX_VIEWS = 16;
struct BwdView {
    const float* view;
    const float* proj;
    const float* campos;
    float focal_x, focal_y, tan_fovx, tan_fovy;
    const int* radii;
    const float4* conic_opacity;
    const uint8_t* clamped;
    const uint32_t* emit_start;
    const uint32_t* tiles_touched;
    const float* grad_inst;
    const uint32_t* valid;
    const uint32_t* rec_mask;
    float* dL_dmean2D;  // (P,3)
};
struct PreprocessBwdViewsArgs {
    PreprocessBwdArgs a;
    int V;  // views in v[] (1 for the single view, whose launcher also reads a.radii)
    int g_begin, g_end;  // the Gaussians [g_begin, g_end) of this launch (a chunk of [0, P))
    BwdView v[MAX_VIEWS];
};

// Camera gradient of V views (gsr_backward_camera_views; preprocess_bwd.hip): `a` carries the
// parameters and flags (its outputs are not used), v[] what preprocess_bwd reads per view.
constexpr int CAM_SUMS = 27;               // 12 dL/dview + 12 dL/dproj + 3 dL/dcampos
constexpr int CAM_ROW = 32;                // floats per workgroup row of the workspace
constexpr int CAM_WG_GAUSSIANS = 256;      // Gaussians per workgroup: one per lane
struct CameraBwdArgs {
    PreprocessBwdArgs a;
    int V;
    BwdView v[MAX_VIEWS];
    float* partial;  // workspace: [V][nwg][CAM_ROW]
    int nwg;         // set by the launcher: camera_bwd_workgroups(a.P)
    float* dL_dview;    // (V,4,4)
    float* dL_dproj;    // (V,4,4)
    float* dL_dcampos;  // (V,3)
};
int camera_bwd_workgroups(int P);
size_t camera_bwd_workspace_bytes(int V, int P);
hipError_t launch_camera_bwd_views(const CameraBwdArgs& a, hipStream_t s);

struct AdamArgs {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    const uint8_t* visible;  // one flag per Gaussian (bool)
    float lr, b1, b2, eps;
    int N, M;  // N Gaussians of M elements each
};
constexpr int ADAM_MAX_GROUPS = 8;
struct AdamMultiArgs {
    AdamArgs g[ADAM_MAX_GROUPS];
    uint32_t block_start[ADAM_MAX_GROUPS];  // first workgroup of each group
    int n_groups;
};
hipError_t launch_adam_update(const AdamArgs& a, hipStream_t s);
hipError_t launch_adam_update_multi(const AdamArgs* groups, int n_groups, hipStream_t s);

hipError_t launch_preprocess(const PreprocessArgs& a, hipStream_t s);
// V views of the same Gaussians (a[v] differ in camera and output buffers only), PREPROCESS_BATCH
// views per launch: each launch reads the Gaussians' parameters once.
constexpr int PREPROCESS_BATCH = 8;
hipError_t launch_preprocess_views(const PreprocessArgs* a, int V, hipStream_t s);
hipError_t launch_mark_visible(int P, const float* means3D, const float* view, bool* present, hipStream_t s);
// The u64 words of a scan's `status` (ScanJob)
int scan_status_words(int n);

// Batched prefix launches (gsr_forward_views): up to VIEW_BATCH views per launch, view =
// blockIdx.y, each with its own arrays and sizes (workgroups past a view's size exit at once).
// One launch per step over all views replaces V launches of a few hundred workgroups each: the
// latency-bound prefix kernels of one 1M-Gaussian view fill a fraction of the chip.
constexpr int VIEW_BATCH = 8;
template <typename A>
struct ViewBatch {
    A v[VIEW_BATCH];
    int n;
};

// One view's scan of in[0..n): chained chunks with decoupled look-back over `status`
// (scan_status_words(n) u64 words, zero on entry: preprocess clears them).  The total goes to
// *total_out (pinned host memory is fine; may be null).
struct ScanJob {
    const uint32_t* in;
    uint32_t* out;
    int n;
    uint64_t* status;
    uint32_t* total_out;
};
// inclusive sums, or exclusive ones: one launch per VIEW_BATCH views
hipError_t launch_scan_batch(const ScanJob* jobs, int V, bool exclusive, hipStream_t s);

struct SortJob {  // radix_sort's arguments for one view
    int n;
    const uint32_t* keys_in;
    const uint2* pairs;
    uint32_t *k0, *v0, *k1, *v1;
    uint32_t *out_x, *out_y, *sorted_keys;
    char* scratch;
    const uint2* rects;
    uint2* sorted_rects;
    uint32_t* sorted_counts;
    // packed rects (rect_pack) in key order: carried as payload beside the id (v0 / v1 then hold
    // u32x2), the last pass unpacks them into sorted_rects -- no gather by id
    const uint32_t* rects4 = nullptr;
    // > 0 (one pass, pairs given, keys_in null): the key is pairs[i].y >> key_hi_shift, and out_y
    // gets pairs[i].y with those bits cleared
    int key_hi_shift = 0;
    // (with key_hi_shift, instead of pairs) the pairs as two arrays: x[i], y[i] -- the count kernel then
    // reads the 4-B y words only
    const uint32_t* soa_x = nullptr;
    const uint32_t* soa_y = nullptr;
    // the three-pass depth sort: a pinned host word set to 1 when the keys' range was too wide for it
    uint32_t* host_wide = nullptr;
    // the three-pass depth sort's chunk-group counts (radix_gsum_offset/bytes inside `scratch`) are
    // already zero (preprocess clears them); otherwise the sort clears them itself
    bool gsum_zeroed = false;
};
// The chunk-group digit counts of the three-pass depth sort inside its scratch: byte offset and size
// (zero-initialised by the caller, see SortJob::gsum_zeroed).
size_t radix_gsum_offset(int n);
size_t radix_gsum_bytes(int n);
// After a depth sort reported a range too wide for three 9-bit passes (SortJob::host_wide), the
// forward re-runs that sort with four_pass (radix_sort_batch), for that call only.  Test hook: force
// four passes for every depth sort of the calling host thread.
void set_depth_force_wide(bool on);
bool depth_force_wide();
// byte offset, inside a sort's scratch (radix_status_bytes(n)), of its {base, fits} range word
size_t radix_range_offset(int n);
// which sort a radix pass serves (selects the kernels' name tag only: profiles attribute dispatches)
enum SortKind { SORT_DEPTH = 0, SORT_TILE = 1, SORT_CELLS = 2 };
// V independent stable sorts over the same bit width (key bits [shift0, shift0 + nbits)), pass by
// pass in shared launches.
// four_pass: the depth sort (32-bit keys, shift0 0) in four 8-bit passes instead of three 9-bit ones
// (keys whose range is too wide for the relative third pass).
hipError_t radix_sort_batch(const SortJob* jobs, int V, int nbits, hipStream_t s, int shift0 = 0,
                            SortKind kind = SORT_DEPTH, bool four_pass = false);

// Emission fused into the tile sort (gsr_forward_views): the instances are generated from the
// depth-ordered rects inside the first radix pass's count and scatter kernels instead of being
// written out by an emission kernel and read back by that pass.
struct TileSortJob {
    int P, L;
    const uint32_t* sorted_ids;
    const uint32_t* offsets;      // inclusive scan of the tile counts in depth order
    const uint2* sorted_rects;
    char* pass1_scratch;          // fused_pass1_scratch_bytes(P): the first pass's count matrix
    uint32_t *k0, *v0, *k1, *v1;  // ping-pong (v: u32x2)
    char* scratch;                // radix_status_bytes(L) for the later passes
    uint32_t* out_slot;           // BIN_SLOT
    uint32_t* out_ids;            // BIN_POINT_LIST
    uint32_t* out_tiles;          // BIN_SORTED_TILES
    uint32_t* valid;              // BIN_VALID, cleared
    uint2* ranges;                // IMG_RANGES, cleared
    bool slotless;                // slots_from_rect: no record slots written (render_bwd derives them)
};
size_t fused_pass1_scratch_bytes(int P);
// phases: FUSED_COUNT = the first pass's histogram and row scan (needs neither L nor the binning
// buffer: the batched forward runs it while the host reads L back), FUSED_SCATTER = the rest
enum FusedPhase { FUSED_COUNT = 1, FUSED_SCATTER = 2, FUSED_ALL = 3 };
hipError_t tile_sort_fused_batch(const TileSortJob* jobs, int V, uint32_t gx, int T, hipStream_t s,
                                 int phases = FUSED_ALL);

struct RangesJob {
    int L;
    const uint32_t* sorted_tiles;
    uint2* ranges;
};
// views with L == 0 get their ranges zeroed (no emission cleared them); the others' ranges must be
// zero on entry (the fused tile sort's first pass clears them)
hipError_t launch_tile_ranges_batch(const RangesJob* jobs, int V, int T, hipStream_t s);

struct OrderJob {
    const uint2* ranges;
    const uint32_t* work;
    uint32_t* order;
    // the forward's order from the rects' difference array (use_tile_diff): the kernel derives the
    // per-tile counts, WRITES the ranges (ranges_out) and orders by count; ranges and work unused
    const int* diff;
    uint2* ranges_out;
    uint32_t grid_x, grid_y;
};
// Longest-first launch order of each view's T tiles: order[] = tiles by decreasing work, work = range
// length (ranges, the forward) or work[] (the backward's per-tile largest n_contrib).
// every job with ranges (the forward's order), every job with diff (the forward's, ranges written),
// or every job with work (the backward's)
hipError_t launch_tile_order_batch(const OrderJob* jobs, int V, int T, hipStream_t s);

// The rects' 2-D difference array (+1 at (x0, y0) and (x1, y1), -1 at (x1, y0) and (x0, y1) of every
// packed rect, rect_pack) added into diff (zeroed by preprocess): TILE_HIST_WGS workgroups per view
// accumulate in LDS and add their arrays into diff with integer atomics (order-independent).
struct TileHistJob {
    const uint32_t* rect4;
    int P;
    int* diff;
};
hipError_t launch_tile_hist_batch(const TileHistJob* jobs, int V, uint32_t grid_x, uint32_t grid_y, hipStream_t s);

hipError_t radix_sort(int n, int nbits, const uint32_t* keys_in, const uint2* pairs, uint32_t* k0, uint32_t* v0,
                      uint32_t* k1, uint32_t* v1, uint32_t* out_x, uint32_t* out_y, uint32_t* sorted_keys,
                      char* scratch, hipStream_t s, const uint2* rects = nullptr, uint2* sorted_rects = nullptr,
                      uint32_t* sorted_counts = nullptr, SortKind kind = SORT_DEPTH);
hipError_t launch_debug_keys(int L, const uint32_t* sorted_tiles, const uint32_t* point_list, const uint32_t* dkeys,
                             uint64_t* keys, hipStream_t s);
hipError_t launch_debug_keys_from_ranges(int T, const uint2* ranges, const uint32_t* point_list, const uint32_t* dkeys,
                                         uint64_t* keys, hipStream_t s);

// V views of one image size in one launch per VIEW_BATCH views (grid.y = view); render_bwd: every
// view with dL_invdepths, or none (dL_dalphas: any view, tested per view)
hipError_t launch_render_fwd_batch(const RenderFwdArgs* a, int V, int T, hipStream_t s);
hipError_t launch_render_bwd_batch(const RenderBwdArgs* a, int V, int T, hipStream_t s);
// The alpha output of V views of n = H*W pixels each: out[i] = 1 - final_T[i] (final_T as render_fwd
// stored it), one launch per VIEW_BATCH views (grid.y = view).
struct AlphaJob {
    const float* final_T;
    float* out;
};
hipError_t launch_alpha_batch(const AlphaJob* jobs, int V, size_t n, hipStream_t s);
hipError_t launch_preprocess_bwd_views(const PreprocessBwdViewsArgs& a, hipStream_t s);
// one view through the batched kernel at one lane per Gaussian (a.radii set: the view's visibility)
hipError_t launch_preprocess_bwd_single(const PreprocessBwdViewsArgs& a, hipStream_t s);

// fused SSIM (ssim.hip); dA/dB/dC null: map only
hipError_t launch_ssim_fwd(int planes, int H, int W, float C1, float C2, const float* img1, const float* img2,
                           float* map, float* dA, float* dB, float* dC, hipStream_t s);
hipError_t launch_ssim_bwd(int planes, int H, int W, const float* img1, const float* img2, const float* dmap,
                           const float* dA, const float* dB, const float* dC, float* dimg1, hipStream_t s);

// fused photometric loss of V views of C planes each (ssim.hip):
//   loss[v] = (1 - lambda) mean|x - gt_v| + lambda (1 - mean SSIM(x, gt_v)),  x = img or clamp(img, 0, 1).
// img / dimg / dA..dC: contiguous (V, C, H, W); gt: one (C, H, W) array per view.
struct PhotoViews {
    const float* gt[MAX_VIEWS];
    int V, C;
};
// bytes of the forward's workspace (one (sum SSIM, sum |x - gt|) pair of doubles per tile)
size_t photo_loss_workspace_bytes(int V, int C, int H, int W);
// dA/dB/dC null: no backward will follow (nothing but loss[V] is written)
hipError_t launch_photo_loss_fwd(const PhotoViews& views, int H, int W, float lambda, bool clamp, const float* img,
                                 float* loss, float* dA, float* dB, float* dC, void* workspace, hipStream_t s);
// dloss: V upstream gradients on the device
hipError_t launch_photo_loss_bwd(const PhotoViews& views, int H, int W, float lambda, bool clamp, const float* img,
                                 const float* dloss, const float* dA, const float* dB, const float* dC, float* dimg,
                                 hipStream_t s);

// fused view loss (ssim.hip): train.py:112-141 for V views, from the raw rasterizer outputs --
//   e_c = sum_k raw_k E[k, c] + E[c, 3] (exposure: (V,3,4), C = 3; null: e = raw),
//   x_c = clamp(e_c, 0, 1) * mask_v (mask[v]: (H,W) or null),
//   loss[v] = photo(x, gt_v) + depth_weight mean|(invdepth_v - target[v]) * dmask[v]| (views with a target).
struct ViewLossArgs {
    PhotoViews pv;
    const float* mask[MAX_VIEWS];
    const float* target[MAX_VIEWS];
    const float* dmask[MAX_VIEWS];
    const float* exposure;
    const float* invdepth;  // (V,H,W); the depth term runs if this is set, depth_weight > 0 and a view has a target
    float depth_weight;
    int clamp;
};
// bytes of the workspace of either pass (per-tile partial sums in double)
size_t view_loss_workspace_bytes(int V, int C, int H, int W);
hipError_t launch_view_loss_fwd(const ViewLossArgs& a, int H, int W, float lambda, const float* img, float* loss,
                                float* dA, float* dB, float* dC, void* workspace, hipStream_t s);
// dexposure: (V,3,4), with a.exposure; dinv: (V,H,W) or null (zero-filled if the depth term does not run)
hipError_t launch_view_loss_bwd(const ViewLossArgs& a, int H, int W, float lambda, const float* img,
                                const float* dloss, const float* dA, const float* dB, const float* dC, float* dimg,
                                float* dexposure, float* dinv, void* workspace, hipStream_t s);

// densification statistics of V views in one pass (densify_stats.hip): for every Gaussian i and every
// view v in order with radii[v, i] > 0: max_radii[i] = max(max_radii[i], radii[v, i]),
// accum[i] += |grads[v, i, 0:2]|, denom[i] += 1, visible_count[i] += 1 (if given).  accum / denom are
// addressed with element strides; Gaussians no view sees are not written.
struct DensifyStatsArgs {
    int V, P;
    const float* grads;  // (V, P, 3)
    const int* radii;    // (V, P)
    float* max_radii;    // (P,)
    float* accum;
    float* denom;
    long accum_stride, denom_stride;
    float* visible_count;  // (P,) or null
};
hipError_t launch_densify_stats(const DensifyStatsArgs& a, hipStream_t s);

// parameter activations (activations.hip): scales = exp(scaling), opacities = sigmoid(opacity),
// rotations = rotation / max(|rotation|_2, 1e-12), all (P,3) / (P,) / (P,4) contiguous, one launch.
struct ActivateFwdArgs {
    int P;
    const float* scaling;
    const float* rotation;
    const float* opacity;
    float* scales;
    float* rotations;
    float* opacities;
};
// bit set = that destination of the backward is added to instead of overwritten
enum ActAccBits : uint32_t { ACT_ACC_SCALING = 1u, ACT_ACC_ROTATION = 2u, ACT_ACC_OPACITY = 4u };
// the chain rule of the three activations from the saved outputs (scales, opacities) and the raw
// quaternion; a group whose incoming gradient is null is skipped (its destination is not touched)
struct ActivateBwdArgs {
    int P;
    const float* scales;
    const float* rotation;
    const float* opacities;
    const float* dL_dscales;
    const float* dL_drotations;
    const float* dL_dopacities;
    float* dL_dscaling;
    float* dL_drotation;
    float* dL_dopacity;
    uint32_t acc;  // ACT_ACC_* bits
};
hipError_t launch_activate_fwd(const ActivateFwdArgs& a, hipStream_t s);
hipError_t launch_activate_bwd(const ActivateBwdArgs& a, hipStream_t s);

// densify_and_prune (densify.hip): the plan decides every source row's fate (one wave scans
// DENSIFY_ROWS_PER_WAVE rows, four waves per workgroup) and leaves, in `workspace`, the source rows of
// the output rows in output order; the apply writes every output element of every group once.
constexpr int DENSIFY_ROWS_PER_WAVE = 1024;
constexpr int DENSIFY_ROWS_PER_WG = 4 * DENSIFY_ROWS_PER_WAVE;
constexpr int DENSIFY_MAX_GROUPS = 8;
struct DensifyPlanArgs {
    int P, N;
    const float* accum;
    const float* denom;
    long accum_stride, denom_stride;
    const float* scaling;  // (P,3) log scales
    const float* opacity;  // (P,) logits
    float max_grad, dense_extent, min_opacity;
    float big_extent;  // < 0: no world-size test
    float shrink;      // densify_split_shrink(N)
};
struct DensifyApplyArgs {
    int P, P_after, n_split, N, n_groups;
    int M[DENSIFY_MAX_GROUPS];  // floats per row
    int xyz_group, scaling_group, rotation_group;
    const float* src[DENSIFY_MAX_GROUPS];
    const float* src_m[DENSIFY_MAX_GROUPS];
    const float* src_v[DENSIFY_MAX_GROUPS];
    float* dst[DENSIFY_MAX_GROUPS];
    float* dst_m[DENSIFY_MAX_GROUPS];  // null: the group has no moments
    float* dst_v[DENSIFY_MAX_GROUPS];
    const float* samples;  // (N * n_split, 3)
    float shrink;
};
size_t densify_workspace_bytes(int P);
float densify_split_shrink(int N);  // a child's scale is its parent's divided by this (0.8 N)
// host_counts: 5 words of pinned host memory (kept originals, kept clones, split-selected, kept split
// parents, clone-selected), valid once the stream has been synchronised
hipError_t launch_densify_plan(const DensifyPlanArgs& a, char* workspace, uint32_t* host_counts, hipStream_t s);
hipError_t launch_densify_apply(const DensifyApplyArgs& a, const char* workspace, hipStream_t s);

// visibility-compacted gradient exchange (compact.hip): the bit set of the Gaussians a rank's views saw,
// the union of the ranks' sets as an ascending row list, and the move of those rows of every group
// into and out of a compact buffer laid out [group][union row][column].
constexpr int UNION_ROWS_PER_WAVE = 1024;  // one wave of the plan covers this many Gaussians (32 words)
constexpr int UNION_MAX_BOUNDS = 16;
// words: (P + 31) / 32; bit g & 31 of word g >> 5 = count[g] > 0, bits at or beyond P zero
hipError_t launch_visibility_pack(int P, const float* count, uint32_t* words, hipStream_t s);
size_t union_workspace_bytes(int P);
// words: (ranks, (P + 31) / 32); rows: P words, [0, U) written; mask: P bytes or null; bounds: n_bounds
// <= UNION_MAX_BOUNDS host ints, each a multiple of UNION_ROWS_PER_WAVE or P; host_out: 1 + n_bounds
// words of pinned host memory (U, then the union rows below each boundary), valid once the stream has
// been synchronised
hipError_t launch_union_plan(int P, int ranks, const uint32_t* words, int n_bounds, const int* bounds,
                             char* workspace, uint32_t* rows, uint8_t* mask, uint32_t* host_out, hipStream_t s);
struct RowsMoveArgs {
    int P, U, u0, u1, n_groups;  // the window [u0, u1) of the U union rows
    int M[ADAM_MAX_GROUPS];      // floats per row (0: the group is skipped)
    float* full[ADAM_MAX_GROUPS];  // (P, M[g]) (only read by the gather)
    const uint32_t* rows;        // the plan's list
    float* compact;              // U * sum(M) floats (only read by the scatter)
};
hipError_t launch_rows_move(const RowsMoveArgs& a, bool scatter, hipStream_t s);

// distCUDA2 (knn.hip); host_bounds: 6 words of pinned host memory
size_t knn_workspace_bytes(int P);
hipError_t knn_dist2(int P, const float* pts, float* dist2, char* workspace, uint32_t* host_bounds, hipStream_t s);

}  // namespace gsr
