// capi.hip -- C-ABI entry points (include/gsr.h).  Host-side orchestration that
// replaces CudaRasterizer::Rasterizer::{markVisible, forward, backward}
// (rasterizer_impl.cu:141-450): state-buffer carving, launch order, the one
// stream-ordered D2H of num_rendered, and error reporting.  No exceptions
// cross the ABI; every launch goes to the caller's stream.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "gsr.h"
#include "simple_knn.h"
#include "fused_ssim.h"
#include "gsr_common.h"
#include "gsr_kernels.h"

using namespace gsr;

static_assert(GSR_ACC_MEANS3D == ACC_MEANS3D && GSR_ACC_DC == ACC_DC && GSR_ACC_SH == ACC_SH &&
                  GSR_ACC_OPACITY == ACC_OPACITY && GSR_ACC_SCALES == ACC_SCALES &&
                  GSR_ACC_ROTATIONS == ACC_ROTATIONS && GSR_ACC_COV3D == ACC_COV3D && GSR_ACC_COLORS == ACC_COLORS,
              "include/gsr.h accumulate bits match the kernel's");

namespace {

thread_local std::string g_err;
thread_local uint32_t* g_pinned = nullptr;
constexpr uint32_t L_PENDING = 0xFFFFFFFFu;  // h[2] before the scan stores num_rendered (< 2^31)
// forward_geometry_wait: the depth keys' range was too wide for the three-pass depth sort (h[1]); that
// call's depth sort and tile-count scan are re-run with four passes (depth_sort_rerun_wide) --
// internal, never returned to a caller
constexpr int GSR_RERUN_WIDE = -100;
// depth-sort passes of this thread's last forward (per view: 3, or 4 after a re-run of its depth
// sort; gsr_debug_last_depth_passes)
thread_local int t_last_depth_passes[MAX_VIEWS] = {};

int fail(int code, const char* msg)
{
    g_err = msg;
    return code;
}

int fail_hip(hipError_t e, int line)
{
    char buf[256];
    snprintf(buf, sizeof(buf), "HIP error: %s (capi.hip:%d)", hipGetErrorString(e), line);
    g_err = buf;
    return GSR_ERR_HIP;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail_hip(e_, __LINE__);                                   \
    } while (0)

#define DEBUG_SYNC(stream)                                                                    \
    do {                                                                                      \
        if (debug) {                                                                          \
            HIP_TRY(hipStreamSynchronize(stream));                                            \
            HIP_TRY(hipGetLastError());                                                       \
        }                                                                                     \
    } while (0)

// Pinned, device-mapped host words of this host thread, one 16-word slot per view of a
// multi-view forward (slot 0 for a single view).  The forward's kernels store the
// prefiltered-violation flag and num_rendered straight into them (system-scope stores), so the
// forward needs neither a device memset nor a D2H copy before its one stream synchronisation.
constexpr int PINNED_SLOT_WORDS = 16;
int pinned(int slot, uint32_t** out)
{
    if (!g_pinned) {
        // (two more slots behind the views': gsr_union_plan's 1 + UNION_MAX_BOUNDS words)
        hipError_t e = hipHostMalloc((void**)&g_pinned, 4 * PINNED_SLOT_WORDS * (MAX_VIEWS + 2),
                                     hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) return fail_hip(e, __LINE__);
    }
    *out = g_pinned + PINNED_SLOT_WORDS * slot;
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// The forward's binning prefix (preprocess, depth sort, scans, tile sort, tile ranges,
// tile order: small, latency-bound launches) runs on an internal stream of the highest priority,
// forked from the caller's stream and joined back into it before render_fwd.  When the caller
// overlaps views on several streams (the forward of view v+1 beside the backward of view v,
// bench.py), the dispatcher then places the prefix's workgroups ahead of the queued workgroups of
// the other view's long kernels instead of behind them.  Buffers stay stream-ordered for the caller:
// everything the prefix writes is joined into its stream before the entry point returns.
// ---------------------------------------------------------------------------
// the fork / join events order streams of one device only: no system-scope fence (the host never
// inspects them; what the host reads -- num_rendered -- the scan stores with system-scope atomics)
constexpr unsigned EVENT_FLAGS = hipEventDisableTiming | hipEventDisableSystemFence;
// An internal stream of the highest priority with the events that order it against the stream it is
// forked from (in) and joined back into (out); created lazily, one per host thread and device.
struct PrefixStream {
    hipStream_t s = nullptr;
    hipEvent_t in = nullptr, out = nullptr;
};
constexpr int MAX_DEVICES = 64;
thread_local PrefixStream g_prefix[MAX_DEVICES];
// side work of a prefix (the index-order scan, the rects' difference array) beside its critical path
thread_local PrefixStream g_aux[MAX_DEVICES];
// gsr_set_prefix_stream: 0 = everything on the caller's stream; 1 = the prefix on its own
// high-priority stream (forked from the caller's, joined before render_fwd) and its side work on
// the auxiliary stream; 2 = the prefix on the caller's stream, its side work on the auxiliary stream
thread_local int g_prefix_mode = 1;

// *out: the current device's stream of `streams`, forked from `from` (it waits for everything
// enqueued on `from` so far); `from` itself when the stream is off (or the device is out of range).
int stream_fork(PrefixStream* streams, bool on, hipStream_t from, hipStream_t* out)
{
    *out = from;
    if (!on) return GSR_OK;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) return GSR_OK;
    PrefixStream& ps = streams[dev];
    if (!ps.s) {
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipEventCreateWithFlags(&ps.in, EVENT_FLAGS));
        HIP_TRY(hipEventCreateWithFlags(&ps.out, EVENT_FLAGS));
        HIP_TRY(hipStreamCreateWithPriority(&ps.s, hipStreamNonBlocking, greatest));
    }
    HIP_TRY(hipEventRecord(ps.in, from));
    HIP_TRY(hipStreamWaitEvent(ps.s, ps.in, 0));
    *out = ps.s;
    return GSR_OK;
}

// `from` waits for everything enqueued so far on `forked`, which stream_fork(streams, ...) gave
int stream_join(PrefixStream* streams, hipStream_t from, hipStream_t forked)
{
    if (forked == from) return GSR_OK;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    PrefixStream& ps = streams[dev];
    HIP_TRY(hipEventRecord(ps.out, forked));
    HIP_TRY(hipStreamWaitEvent(from, ps.out, 0));
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// Optional per-kernel timing with HIP events recorded on the launch stream
// (bench.py's roofline leg).  Off by default; costs two event records per
// launch when on.
// ---------------------------------------------------------------------------
enum ProfKernel {
    PK_PREPROCESS = 0, PK_DEPTH_SORT, PK_SCAN, PK_EMIT, PK_TILE_SORT, PK_RANGES, PK_RENDER_FWD, PK_RENDER_BWD,
    PK_PREPROCESS_BWD, PK_TILE_ORDER, PK_CAMERA_BWD,
    PK_COUNT
};
const char* kProfNames[PK_COUNT] = {"preprocess_fwd", "depth_sort", "scan", "emit_instances", "tile_sort",
                                    "tile_ranges", "render_fwd", "render_bwd", "preprocess_bwd", "tile_order",
                                    "camera_bwd"};
struct Prof {
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool[PK_COUNT];
    size_t used[PK_COUNT] = {};
    size_t parts[PK_COUNT] = {};  // scopes that continue the kernel's previous one (not a new launch)
};
Prof g_prof;

hipEvent_t prof_begin(int k, hipStream_t s)
{
    if (!g_prof.on) return nullptr;
    auto& pool = g_prof.pool[k];
    if (g_prof.used[k] == pool.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return nullptr;
        pool.push_back({a, b});
    }
    hipEvent_t e = pool[g_prof.used[k]].first;
    (void)hipEventRecord(e, s);
    return e;
}

void prof_end(int k, hipStream_t s, hipEvent_t begun, bool part)
{
    if (!g_prof.on || !begun) return;
    (void)hipEventRecord(g_prof.pool[k][g_prof.used[k]].second, s);
    g_prof.used[k]++;
    if (part) g_prof.parts[k]++;
}

// part: the scope times the rest of a kernel stage whose first part had a scope of its own (its time
// adds to the stage's total, not to its launch count)
struct ProfScope {
    int k; hipStream_t s; hipEvent_t e; bool part;
    ProfScope(int k_, hipStream_t s_, bool part_ = false) : k(k_), s(s_), e(prof_begin(k_, s_)), part(part_) {}
    ~ProfScope() { prof_end(k, s, e, part); }
};

// The tile grid of a width x height image: tiles per row and column, and their number.
struct TileGrid {
    uint32_t gx, gy;
    int T;
    TileGrid(int width, int height)
        : gx((uint32_t)((width + GSR_BLOCK_X - 1) / GSR_BLOCK_X)), gy((uint32_t)((height + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y)),
          T((int)(gx * gy))
    {
    }
};

template <typename T>
T* at(char* base, size_t off) { return reinterpret_cast<T*>(base + off); }
template <typename T>
const T* at(const char* base, size_t off) { return reinterpret_cast<const T*>(base + off); }

// What the entry points' positional arguments say, filled once at the ABI boundary.
// The Gaussians and what every view of a call shares (M as the caller counts it: without dc)
struct Scene {
    int P, D, M;
    const float *means3D, *dc, *shs, *colors_precomp, *opacities, *scales;
    float scale_modifier;
    const float *rotations, *cov3D_precomp;
    bool prefiltered, antialiasing;
    int width, height;
};
struct Camera {
    const float *view, *proj, *campos;
    float tan_fovx, tan_fovy;
};
// One view's state buffers and outputs (radii null: the GeometryState's own; the backward only reads them)
struct ViewState {
    char *geometry, *image, *binning;
    size_t binning_capacity;
    float *out_color, *invdepth;
    int* radii;
};

}  // namespace

extern "C" {

const char* gsr_last_error(void) { return g_err.c_str(); }

const char* gsr_version(void) { return GSR_REF_ALPHA ? "gsr-hip 0.1 gfx950 ref-alpha (TEST BUILD)" : "gsr-hip 0.1 gfx950"; }

int gsr_set_prefix_stream(int on)
{
    if (on < 0 || on > 2) return fail(GSR_ERR_INVALID, "prefix stream mode must be 0, 1 or 2");
    g_prefix_mode = on;
    return GSR_OK;
}

int gsr_profile_enable(int on)
{
    g_prof.on = on != 0;
    for (int k = 0; k < PK_COUNT; k++) g_prof.used[k] = 0;
    return PK_COUNT;
}

const char* gsr_profile_kernel_name(int k) { return (k >= 0 && k < PK_COUNT) ? kProfNames[k] : ""; }

// Waits for every recorded event, returns per-kernel summed milliseconds and launch counts
// since the last enable/read, and resets the counters.
int gsr_profile_read(double* total_ms, int* counts, int n)
{
    for (int k = 0; k < PK_COUNT && k < n; k++) {
        double acc = 0.0;
        for (size_t j = 0; j < g_prof.used[k]; j++) {
            auto& ev = g_prof.pool[k][j];
            HIP_TRY(hipEventSynchronize(ev.second));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev.first, ev.second));
            acc += ms;
        }
        total_ms[k] = acc;
        counts[k] = (int)(g_prof.used[k] - g_prof.parts[k]);
        g_prof.used[k] = 0;
        g_prof.parts[k] = 0;
    }
    return PK_COUNT;
}

size_t gsr_geometry_buffer_size(int P) { return geom_layout(P).off[GEOM_COUNT] + 256; }
size_t gsr_image_buffer_size(int width, int height) { return image_layout(width, height).off[IMG_COUNT] + 256; }
size_t gsr_binning_buffer_size(int num_rendered) { return bin_layout(num_rendered).off[BIN_COUNT] + 256; }

// Byte offsets of the arrays inside each state buffer (test/debug introspection).
int gsr_geometry_layout(int P, size_t* offsets, int n)
{
    GeomLayout l = geom_layout(P);
    for (int i = 0; i < n && i <= GEOM_COUNT; i++) offsets[i] = l.off[i];
    return GEOM_COUNT;
}
int gsr_image_layout(int W, int H, size_t* offsets, int n)
{
    ImageLayout l = image_layout(W, H);
    for (int i = 0; i < n && i <= IMG_COUNT; i++) offsets[i] = l.off[i];
    return IMG_COUNT;
}
int gsr_binning_layout(int L, size_t* offsets, int n)
{
    BinLayout l = bin_layout(L);
    for (int i = 0; i < n && i <= BIN_COUNT; i++) offsets[i] = l.off[i];
    return BIN_COUNT;
}

int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, bool* present,
                     gsr_stream_t stream)
{
    (void)projmatrix;
    if (P < 0) return fail(GSR_ERR_INVALID, "P must be >= 0");
    if (P == 0) return GSR_OK;
    if (!means3D || !viewmatrix || !present) return fail(GSR_ERR_INVALID, "null pointer");
    HIP_TRY(launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream));
    return GSR_OK;
}


// The forward's argument checks for one view (no HIP call)
static int forward_args_check(const Scene& sc, const ViewState& vs)
{
    if (sc.width <= 0 || sc.height <= 0) return fail(GSR_ERR_INVALID, "image size must be positive");
    if (!sc.colors_precomp && !sc.dc && (!sc.shs || sc.M <= 0))
        return fail(GSR_ERR_INVALID, "Please provide exactly one of either SHs or precomputed colors!");
    if (sc.dc && sc.M < 0) return fail(GSR_ERR_INVALID, "M (rest SH coefficients) must be >= 0");
    if (sc.dc && sc.colors_precomp)
        return fail(GSR_ERR_INVALID, "Please provide exactly one of either SHs or precomputed colors!");
    if (sc.dc && sc.M > 0 && !sc.shs)
        return fail(GSR_ERR_INVALID, "dc given with M > 0 rest coefficients but shs is NULL");
    if (!sc.cov3D_precomp && (!sc.scales || !sc.rotations))
        return fail(GSR_ERR_INVALID,
                    "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    if (!vs.geometry || !vs.image) return fail(GSR_ERR_ALLOC, "null state buffer");
    return GSR_OK;
}

// The arguments of one view's preprocess (checked: forward_args_check); the view's pinned read-back
// slot is reset: *h_out its host words, *hdev_out their device address.
// geometry_outputs: GeometryState's means2D, depths, rgb and conic_opacity are written
static int preprocess_args(const Scene& sc, const Camera& cam, const ViewState& vs, int slot, bool geometry_outputs,
                           PreprocessArgs* out, uint32_t** h_out, uint32_t** hdev_out)
{
    const int P = sc.P, width = sc.width, height = sc.height;
    const GeomLayout g = geom_layout(P);
    char* gb = vs.geometry;
    // h[0]: prefiltered violation (written by preprocess), h[2]: num_rendered (written by the scan).
    // This thread's previous forward has read its num_rendered back, so no kernel still writes them.
    uint32_t* h;
    int rc = pinned(slot, &h);
    if (rc) return rc;
    h[0] = 0;
    h[1] = 0;  // the depth sort's "range too wide" flag
    __atomic_store_n(&h[2], L_PENDING, __ATOMIC_RELEASE);
    uint32_t* h_dev = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void**)&h_dev, h, 0));

    PreprocessArgs& a = *out;
    a.P = P; a.D = sc.D; a.M = sc.dc ? sc.M + 1 : sc.M; a.W = width; a.H = height;  // kernels count the dc coefficient
    a.dc = sc.dc;
    a.means3D = sc.means3D; a.scales = sc.scales; a.scale_modifier = sc.scale_modifier; a.rotations = sc.rotations;
    a.opacities = sc.opacities; a.shs = sc.shs; a.cov3D_precomp = sc.cov3D_precomp;
    a.colors_precomp = sc.colors_precomp;
    a.view = cam.view; a.proj = cam.proj; a.campos = cam.campos;
    a.tan_fovx = cam.tan_fovx; a.tan_fovy = cam.tan_fovy;
    a.focal_y = height / (2.0f * cam.tan_fovy);
    a.focal_x = width / (2.0f * cam.tan_fovx);
    const TileGrid tg(width, height);
    a.grid_x = tg.gx;
    a.grid_y = tg.gy;
    a.prefiltered = sc.prefiltered; a.antialiasing = sc.antialiasing;
    a.radii = vs.radii ? vs.radii : at<int>(gb, g.off[GEOM_RADII]);
    // (the batched forward leaves them out: nothing reads them after the forward -- preprocess_bwd
    // recomputes conic_opacity -- and they are 40 B per visible Gaussian and view)
    a.means2D = geometry_outputs ? at<float>(gb, g.off[GEOM_MEANS2D]) : nullptr;
    a.depths = geometry_outputs ? at<float>(gb, g.off[GEOM_DEPTH]) : nullptr;
    a.rgb = geometry_outputs ? at<float>(gb, g.off[GEOM_RGB]) : nullptr;
    a.conic_opacity = geometry_outputs ? at<float>(gb, g.off[GEOM_CONIC_OPACITY]) : nullptr;
    a.clamped = at<uint8_t>(gb, g.off[GEOM_CLAMPED]);
    a.tiles_touched = at<uint32_t>(gb, g.off[GEOM_TILES_TOUCHED]);
    a.host_flags = h_dev;
    a.scan_status = at<uint64_t>(gb, g.off[GEOM_SCAN_SCRATCH]);
    a.scan_status_words = 2 * scan_status_words(P);  // the depth-order and the index-order scan
    a.splat = at<float4>(gb, g.off[GEOM_SPLAT]);
    a.dkey = at<uint32_t>(gb, g.off[GEOM_DKEY]);
    a.rect = at<uint2>(gb, g.off[GEOM_RECT]);
    a.rect4 = nullptr;
    if (rect_packable(a.grid_x, a.grid_y)) {  // the depth sort carries the packed rect as payload
        a.rect4 = at<uint32_t>(gb, g.off[GEOM_RECT]);
        a.rect = nullptr;
    }
    a.rec_mask = at<uint32_t>(gb, g.off[GEOM_REC_MASK]);
    // the depth sort's chunk-group counts, zeroed by preprocess (SortJob::gsum_zeroed)
    a.dsort_gsum = at<uint32_t>(gb, g.off[GEOM_RADIX_SCRATCH] + radix_gsum_offset(P));
    a.dsort_gsum_words = (int)(radix_gsum_bytes(P) / 4);
    a.tile_diff = nullptr;
    a.tile_diff_words = 0;
    if (use_tile_diff(a.grid_x, a.grid_y)) {  // the tile ranges from the rects' difference array
        a.tile_diff = at<int>(vs.image, image_layout(width, height).off[IMG_TILE_DIFF]);
        a.tile_diff_words = (int)((a.grid_x + 1) * (a.grid_y + 1));
    }
    *h_out = h;
    *hdev_out = h_dev;
    return GSR_OK;
}

// The forward tile order of a view whose tile ranges come from the rects' difference array
// (tile_hist): it needs nothing from the tile sort, so it runs on the auxiliary stream right after
// tile_hist, beside the depth and tile sorts, instead of between the tile sort and render_fwd.
static OrderJob diff_order_job(char* ib, int width, int height)
{
    const ImageLayout im = image_layout(width, height);
    const TileGrid tg(width, height);
    OrderJob oj = {};
    oj.order = at<uint32_t>(ib, im.off[IMG_TILE_ORDER]);
    oj.diff = at<int>(ib, im.off[IMG_TILE_DIFF]);
    oj.ranges_out = at<uint2>(ib, im.off[IMG_RANGES]);
    oj.grid_x = tg.gx;
    oj.grid_y = tg.gy;
    return oj;
}

// A view's depth sort (the first half of the reference's tile|depth key sort): the keys preprocess
// wrote, ping-pong buffers carved from GEOM_DSORT_TMP; the last pass also lays the tile rects and tile
// counts out in depth order (the counts into point_offsets, which the scan then turns into offsets in
// place).  h_dev: the view's pinned words (word 1: the "range too wide" flag).
static SortJob depth_sort_job(char* gb, const PreprocessArgs& a, uint32_t* h_dev)
{
    const GeomLayout g = geom_layout(a.P);
    char* tmp = gb + g.off[GEOM_DSORT_TMP];
    const size_t q = align_up(4 * (size_t)a.P, 256);
    // keys u32, payload u32x2 (id, packed rect): k0 | v0 v0 | k1 | v1 v1
    SortJob j = {a.P, a.dkey, nullptr, at<uint32_t>(tmp, 0), at<uint32_t>(tmp, q), at<uint32_t>(tmp, 3 * q),
                 at<uint32_t>(tmp, 4 * q), at<uint32_t>(gb, g.off[GEOM_SORTED_IDS]), nullptr, nullptr,
                 gb + g.off[GEOM_RADIX_SCRATCH], a.rect, at<uint2>(gb, g.off[GEOM_SORTED_RECT]),
                 at<uint32_t>(gb, g.off[GEOM_POINT_OFFSETS]), a.rect4};
    j.host_wide = h_dev + 1;
    j.gsum_zeroed = true;  // (preprocess)
    return j;
}

static int forward_geometry_wait(uint32_t* h, gsr_stream_t stream, int* num_rendered)
{
    hipStream_t s = (hipStream_t)stream;
    // 4. the one device->host hand-off of the forward: num_rendered (rasterizer_impl.cu:283-284),
    //    stored by the scan into pinned memory, plus the error flag.  The host polls the word
    //    itself (no driver wake-up on the critical path); hipStreamQuery now and then notices a
    //    stream that failed, or finished without storing it.
    for (uint32_t spin = 1;; spin++) {
        if (__atomic_load_n(&h[2], __ATOMIC_ACQUIRE) != L_PENDING) break;
        if ((spin & 1023u) == 0u) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return fail_hip(q, __LINE__);
        }
    }
    if (__atomic_load_n(&h[2], __ATOMIC_ACQUIRE) == L_PENDING) return fail(GSR_ERR_HIP, "scan did not publish num_rendered");
    if (h[0] & 1u)
        return fail(GSR_ERR_PREFILTERED, "Point is filtered although prefiltered is set. This shouldn't happen!");
    if (__atomic_load_n(&h[1], __ATOMIC_ACQUIRE)) return GSR_RERUN_WIDE;  // (stored before the scan ran: visible with L)
    if (h[2] > 0x7fffffffu) return fail(GSR_ERR_INVALID, "num_rendered overflows int");
    *num_rendered = (int)h[2];
    return GSR_OK;
}

// A view whose visible depth keys spanned too wide a range for the three-pass depth sort
// (forward_geometry_wait returned GSR_RERUN_WIDE): its depth sort runs again in four 8-bit passes and
// the tile-count scan re-publishes num_rendered (its status words cleared first), for THIS call only
// -- the next forward starts with three passes again (the reference's sort keeps no state,
// rasterizer_impl.cu:306-311).  Preprocess, the record-slot scan, the rects' difference array and the
// forward tile order do not depend on the depth order and stand.  (What follows the scan -- the tile
// sort's first-pass histograms -- is the caller's to enqueue again.)  h: the views' pinned words, whose
// scans have published (no kernel still writes them).
static int depth_sort_rerun_wide(SortJob* dsort, const ScanJob* off, uint32_t* const* h, int V, hipStream_t s)
{
    for (int v = 0; v < V; v++) {
        h[v][1] = 0;
        __atomic_store_n(&h[v][2], L_PENDING, __ATOMIC_RELEASE);
        dsort[v].host_wide = nullptr;  // (four passes: no range to report)
        HIP_TRY(hipMemsetAsync(off[v].status, 0, sizeof(uint64_t) * (size_t)scan_status_words(off[v].n), s));
    }
    {
        ProfScope ps_(PK_DEPTH_SORT, s);
        HIP_TRY(radix_sort_batch(dsort, V, DEPTH_BITS, s, 0, SORT_DEPTH, /*four_pass=*/true));
    }
    ProfScope ps_(PK_SCAN, s);
    HIP_TRY(launch_scan_batch(off, V, false, s));
    return GSR_OK;
}

int gsr_debug_last_depth_passes(int view) { return view >= 0 && view < MAX_VIEWS ? t_last_depth_passes[view] : 0; }

int gsr_debug_grad_record_floats(void) { return GRAD_REC; }

// The tile sort of one view (L > 0 instances) with the instance emission fused into its first
// pass: the instances are generated from the depth-ordered rects; the sort's ping-pong buffers live
// in the (not yet used) gradient-record region of the binning buffer, the first pass's count
// matrix in the depth sort's ping-pong buffer (free by then).
// count_only: the job of the histogram phase (FUSED_COUNT), which needs neither L nor the binning buffer
static TileSortJob fused_tile_sort_job(const Scene& sc, const ViewState& vs, int L, bool count_only)
{
    const int P = sc.P, width = sc.width, height = sc.height;
    char *gb = vs.geometry, *ib = vs.image, *bb = vs.binning;
    const GeomLayout g = geom_layout(P);
    const ImageLayout im = image_layout(width, height);
    const BinLayout b = bin_layout(L);
    const size_t q = align_up(4 * (size_t)L, 256);
    TileSortJob j = {};
    j.P = P;
    j.L = L;
    j.sorted_ids = at<uint32_t>(gb, g.off[GEOM_SORTED_IDS]);
    j.offsets = at<uint32_t>(gb, g.off[GEOM_POINT_OFFSETS]);
    j.sorted_rects = at<uint2>(gb, g.off[GEOM_SORTED_RECT]);
    j.pass1_scratch = gb + g.off[GEOM_DSORT_TMP];
    const TileGrid tg(width, height);
    const bool diff = use_tile_diff(tg.gx, tg.gy);
    // with the difference array the tile order writes every range and nothing reads the sorted
    // tile ids: no clearing of the ranges, no tile id written per instance
    j.ranges = diff ? nullptr : at<uint2>(ib, im.off[IMG_RANGES]);
    if (count_only) return j;
    char* w = bb + b.off[BIN_GRAD_INST];
    j.k0 = reinterpret_cast<uint32_t*>(w + 2 * q);
    j.k1 = reinterpret_cast<uint32_t*>(w + 3 * q);
    j.v0 = reinterpret_cast<uint32_t*>(w + 4 * q);  // u32x2 payloads
    j.v1 = reinterpret_cast<uint32_t*>(w + 6 * q);
    j.scratch = bb + b.off[BIN_RADIX_SCRATCH];
    j.slotless = slots_from_rect(tg.gx, tg.gy);
    j.out_slot = j.slotless ? nullptr : at<uint32_t>(bb, b.off[BIN_SLOT]);
    j.out_ids = at<uint32_t>(bb, b.off[BIN_POINT_LIST]);
    j.out_tiles = diff ? nullptr : at<uint32_t>(bb, b.off[BIN_SORTED_TILES]);
    j.valid = at<uint32_t>(bb, b.off[BIN_VALID]);
    return j;
}

// render_fwd's arguments for a view whose binning is complete
static RenderFwdArgs render_fwd_args(const Scene& sc, const ViewState& vs, int L, const float* background)
{
    const int width = sc.width, height = sc.height;
    char *gb = vs.geometry, *ib = vs.image, *bb = vs.binning;
    const GeomLayout g = geom_layout(sc.P);
    const ImageLayout im = image_layout(width, height);
    const BinLayout b = bin_layout(L);
    RenderFwdArgs r;
    r.ranges = at<uint2>(ib, im.off[IMG_RANGES]);
    r.tile_order = at<uint32_t>(ib, im.off[IMG_TILE_ORDER]);
    r.tile_work = at<uint32_t>(ib, im.off[IMG_TILE_WORK]);
    r.point_list = L > 0 ? at<uint32_t>(bb, b.off[BIN_POINT_LIST]) : nullptr;
    r.W = width; r.H = height;
    r.grid_x = TileGrid(width, height).gx;
    r.splat = at<float4>(gb, g.off[GEOM_SPLAT]);
    r.bg = background;
    r.final_T = at<float>(ib, im.off[IMG_FINAL_T]);
    r.n_contrib = at<uint32_t>(ib, im.off[IMG_N_CONTRIB]);
    r.out_color = vs.out_color;
    r.invdepth = vs.invdepth;
    r.hit = L > 0 ? at<uint8_t>(bb, b.off[BIN_HIT]) : nullptr;
    return r;
}

// ---------------------------------------------------------------------------
// The forward of V >= 1 views of the same Gaussians, in two stages split at the num_rendered
// read-back.  Every stage is one launch over all views (grid.y = view).  What the entry points
// differ in they decide themselves and pass in: the stream of the binning prefix (`ps`: the forked
// prefix stream, or the caller's own) and the ForwardOptions.
// ---------------------------------------------------------------------------
enum PreprocessLauncher {
    PREPROCESS_SINGLE,  // launch_preprocess: the one-view kernel instantiation (V == 1 only)
    PREPROCESS_VIEWS    // launch_preprocess_views: the parameters and SH rows read once per 8 views
};
struct ForwardOptions {
    PreprocessLauncher preprocess;
    bool geometry_outputs;  // preprocess writes GeometryState's means2D, depths, rgb and conic_opacity
    // the tile sort's first-pass histograms (FUSED_COUNT) need only the depth-ordered rects and offsets
    // (not L or the binning buffer): enqueued before the read-back, they run while the host waits
    bool early_count;
};

static int tile_sort_count_pass(const Scene& sc, const ViewState* vs, const int* which, int n, hipStream_t ps)
{
    const TileGrid tg(sc.width, sc.height);
    TileSortJob cj[MAX_VIEWS];
    for (int i = 0; i < n; i++) cj[i] = fused_tile_sort_job(sc, vs[which[i]], 0, /*count_only=*/true);
    ProfScope ps_(PK_TILE_SORT, ps);
    HIP_TRY(tile_sort_fused_batch(cj, n, tg.gx, tg.T, ps, FUSED_COUNT));
    return GSR_OK;
}

// Stage one (arguments checked, P > 0): preprocess, depth sort and the tile-count scan, then the one
// host hand-off: L[v] = view v's num_rendered (all zero on failure).  View v uses pinned slot v.
static int forward_geometry(const Scene& sc, int V, const Camera* cam, const ViewState* vs, const ForwardOptions& opt,
                            hipStream_t ps, bool debug, int* L)
{
    const int P = sc.P;
    const TileGrid tg(sc.width, sc.height);
    const GeomLayout g = geom_layout(P);
    for (int v = 0; v < V; v++) L[v] = 0;
    uint32_t *h[MAX_VIEWS], *hdev[MAX_VIEWS];
    PreprocessArgs pa[MAX_VIEWS];
    for (int v = 0; v < V; v++) {
        const int rc = preprocess_args(sc, cam[v], vs[v], v, opt.geometry_outputs, &pa[v], &h[v], &hdev[v]);
        if (rc) return rc;
    }
    // 1. preprocess (forward.cu:154-272)
    {
        ProfScope ps_(PK_PREPROCESS, ps);
        HIP_TRY(opt.preprocess == PREPROCESS_SINGLE ? launch_preprocess(pa[0], ps) : launch_preprocess_views(pa, V, ps));
    }
    DEBUG_SYNC(ps);
    ScanJob rec[MAX_VIEWS], off[MAX_VIEWS];
    SortJob dsort[MAX_VIEWS];
    TileHistJob hj[MAX_VIEWS];
    OrderJob dj[MAX_VIEWS];
    for (int v = 0; v < V; v++) {
        char* gb = vs[v].geometry;
        const PreprocessArgs& a = pa[v];
        rec[v] = {a.tiles_touched, at<uint32_t>(gb, g.off[GEOM_EMIT_START]), P, a.scan_status + scan_status_words(P),
                  nullptr};
        dsort[v] = depth_sort_job(gb, a, hdev[v]);
        uint32_t* offsets = at<uint32_t>(gb, g.off[GEOM_POINT_OFFSETS]);
        off[v] = {offsets, offsets, P, a.scan_status, hdev[v] + 2};  // L -> the view's pinned word
        hj[v] = {a.rect4, P, a.tile_diff};
        dj[v] = diff_order_job(vs[v].image, sc.width, sc.height);
    }
    // 1b. each Gaussian's first gradient-record slot: index-order exclusive scan of the tile counts
    //     (records in Gaussian order: preprocess_bwd's per-Gaussian gathers are contiguous), on the
    //     auxiliary stream beside the depth sort; the tile sort's first pass (which reads it) waits for it
    hipStream_t aux = ps;
    int rc = stream_fork(g_aux, g_prefix_mode != 0, ps, &aux);
    if (rc) return rc;
    // every exit after the fork joins the auxiliary stream back first (the caller's stream stays
    // ordered after the scans queued there, which write into the caller's geometry buffers)
    hipError_t e = launch_scan_batch(rec, V, true, aux);
    if (e == hipSuccess && use_tile_diff(tg.gx, tg.gy)) {  // the rects' difference arrays, beside the depth sorts as well
        ProfScope ps_(PK_RANGES, aux);
        e = launch_tile_hist_batch(hj, V, tg.gx, tg.gy, aux);
    }
    if (e == hipSuccess && use_tile_diff(tg.gx, tg.gy)) {  // ... and from them the tile ranges and the forward's tile orders
        ProfScope ps_(PK_TILE_ORDER, aux);
        e = launch_tile_order_batch(dj, V, tg.T, aux);
    }
    // 2. stable depth sort of the Gaussians
    if (e == hipSuccess) {
        ProfScope ps_(PK_DEPTH_SORT, ps);
        e = radix_sort_batch(dsort, V, DEPTH_BITS, ps);
    }
    // 3. instance offsets in depth order (cub::DeviceScan::InclusiveSum, rasterizer_impl.cu:280); it
    //    reads nothing the auxiliary stream writes, so it goes ahead of the join
    if (e == hipSuccess) {
        ProfScope ps_(PK_SCAN, ps);
        e = launch_scan_batch(off, V, false, ps);
    }
    rc = stream_join(g_aux, ps, aux);
    if (e != hipSuccess) return fail_hip(e, __LINE__);
    if (rc) return rc;
    if (opt.early_count) {
        int all[MAX_VIEWS];
        for (int v = 0; v < V; v++) all[v] = v;
        rc = tile_sort_count_pass(sc, vs, all, V, ps);
        if (rc) return rc;
    }
    DEBUG_SYNC(ps);
    // 4. the one host hand-off: every view's num_rendered (rasterizer_impl.cu:283-284); a view whose depth
    //    range was too wide for three passes re-runs its depth sort in four (this call only), and what
    //    had been enqueued behind its scan -- the histograms -- runs again
    int wide[MAX_VIEWS], nw = 0;
    for (int v = 0; v < V && !rc; v++) {
        rc = forward_geometry_wait(h[v], ps, &L[v]);
        t_last_depth_passes[v] = depth_force_wide() ? 4 : 3;
        if (rc == GSR_RERUN_WIDE) {
            wide[nw++] = v;
            rc = GSR_OK;
        }
    }
    if (!rc && nw) {
        SortJob wj[MAX_VIEWS];
        ScanJob wo[MAX_VIEWS];
        uint32_t* wh[MAX_VIEWS];
        for (int i = 0; i < nw; i++) {
            wj[i] = dsort[wide[i]];
            wo[i] = off[wide[i]];
            wh[i] = h[wide[i]];
            t_last_depth_passes[wide[i]] = 4;
        }
        rc = depth_sort_rerun_wide(wj, wo, wh, nw, ps);
        if (!rc && opt.early_count) rc = tile_sort_count_pass(sc, vs, wide, nw, ps);
        for (int i = 0; i < nw && !rc; i++) rc = forward_geometry_wait(h[wide[i]], ps, &L[wide[i]]);
    }
    if (rc)
        for (int v = 0; v < V; v++) L[v] = 0;
    return rc;
}

// Stage two, for the n views which[0..n) whose binning buffers hold their L[v] instances: the tile
// sort (emission fused in), tile ranges and tile order on the prefix stream `ps`, which is joined
// back into the caller's; then every view's render_fwd in one launch on the caller's.
// counted: the tile sort's first-pass histograms already ran (ForwardOptions::early_count)
static int forward_render(const Scene& sc, const ViewState* vs, const int* L, const int* which, int n,
                          const float* background, bool counted, hipStream_t caller, hipStream_t ps, bool debug)
{
    // (colors_precomp was folded into the render record by preprocess)
    const TileGrid tg(sc.width, sc.height);
    const ImageLayout im = image_layout(sc.width, sc.height);
    TileSortJob tsort[MAX_VIEWS];
    RangesJob rj[MAX_VIEWS];
    OrderJob oj[MAX_VIEWS];
    RenderFwdArgs ra[MAX_VIEWS];
    int ns = 0;
    for (int k = 0; k < n; k++) {
        const ViewState& s = vs[which[k]];
        const int Lv = L[which[k]];
        if (Lv > 0) tsort[ns++] = fused_tile_sort_job(sc, s, Lv, /*count_only=*/false);
        uint2* ranges = at<uint2>(s.image, im.off[IMG_RANGES]);
        rj[k] = {Lv, Lv > 0 ? at<uint32_t>(s.binning, bin_layout(Lv).off[BIN_SORTED_TILES]) : nullptr, ranges};
        oj[k] = {ranges, nullptr, at<uint32_t>(s.image, im.off[IMG_TILE_ORDER])};
        ra[k] = render_fwd_args(sc, s, Lv, background);
    }
    if (ns) {
        // stable sort by tile id over bits [0, msb(T)) of the depth-ordered instances
        // (rasterizer_impl.cu:303-311 sorts [0, 32 + msb(T)) of the tile|depth keys)
        ProfScope ps_(PK_TILE_SORT, ps, counted);
        HIP_TRY(tile_sort_fused_batch(tsort, ns, tg.gx, tg.T, ps, counted ? FUSED_SCATTER : FUSED_ALL));
    }
    DEBUG_SYNC(ps);
    // (with the difference array: ranges and orders were written by stage one, on the auxiliary
    // stream, joined before the tile sort's first pass)
    if (n && !use_tile_diff(tg.gx, tg.gy)) {
        {
            ProfScope ps_(PK_RANGES, ps);
            HIP_TRY(launch_tile_ranges_batch(rj, n, tg.T, ps));
        }
        DEBUG_SYNC(ps);
        ProfScope ps_(PK_TILE_ORDER, ps);
        HIP_TRY(launch_tile_order_batch(oj, n, tg.T, ps));
    }
    DEBUG_SYNC(ps);
    const int rc = stream_join(g_prefix, caller, ps);
    if (rc) return rc;
    if (n) {  // every view's render in one launch (one launch tail per batch)
        ProfScope ps_(PK_RENDER_FWD, caller);
        HIP_TRY(launch_render_fwd_batch(ra, n, tg.T, caller));
    }
    DEBUG_SYNC(caller);
    return GSR_OK;
}

// a view's binning buffer holds L instances (else the view is left to the caller: allocate
// gsr_binning_buffer_size(L), then gsr_forward_render)
static bool binning_fits(const ViewState& vs, int L)
{
    return vs.binning && gsr_binning_buffer_size(L) <= vs.binning_capacity;
}

int gsr_forward_geometry_dc(char* geometry_buffer, char* image_buffer, int P, int D, int M, int width, int height,
                         const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
                         const float* opacities, const float* scales, float scale_modifier,
                         const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                         const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                         bool prefiltered, bool antialiasing, int* radii, bool debug, gsr_stream_t stream,
                         int* num_rendered)
{
    *num_rendered = 0;
    if (P <= 0) return P < 0 ? fail(GSR_ERR_INVALID, "P must be >= 0") : GSR_OK;
    const Scene sc = {P, D, M, means3D, dc, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
                      cov3D_precomp, prefiltered, antialiasing, width, height};
    const Camera cam = {viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy};
    const ViewState vs = {geometry_buffer, image_buffer, nullptr, 0, nullptr, nullptr, radii};
    int rc = forward_args_check(sc, vs);
    if (rc) return rc;
    hipStream_t caller = (hipStream_t)stream, ps = nullptr;
    rc = stream_fork(g_prefix, g_prefix_mode == 1, caller, &ps);
    if (rc) return rc;
    // (no binning buffer yet, and the caller allocates it before gsr_forward_render: no early count pass)
    const ForwardOptions opt = {PREPROCESS_SINGLE, /*geometry_outputs=*/true, /*early_count=*/false};
    rc = forward_geometry(sc, 1, &cam, &vs, opt, ps, debug, num_rendered);
    const int rj = stream_join(g_prefix, caller, ps);
    return rc ? rc : rj;
}

int gsr_forward_render(char* geometry_buffer, char* binning_buffer, char* image_buffer, int P, int num_rendered,
                       const float* background, int width, int height, const float* colors_precomp,
                       float* out_color, float* depth, int* radii, bool debug, gsr_stream_t stream)
{
    (void)radii;
    (void)colors_precomp;
    if (P <= 0) return GSR_OK;
    if (num_rendered > 0 && !binning_buffer) return fail(GSR_ERR_ALLOC, "null binning buffer");
    Scene sc = {};
    sc.P = P; sc.width = width; sc.height = height;  // (all that stage two reads)
    const ViewState vs = {geometry_buffer, image_buffer, binning_buffer, 0, out_color, depth, nullptr};
    hipStream_t caller = (hipStream_t)stream, ps = nullptr;
    int rc = stream_fork(g_prefix, g_prefix_mode == 1, caller, &ps);
    if (rc) return rc;
    const int view = 0;
    rc = forward_render(sc, &vs, &num_rendered, &view, 1, background, /*counted=*/false, caller, ps, debug);
    if (rc) stream_join(g_prefix, caller, ps);
    return rc;
}

// Both stages of a forward whose binning buffers the caller sized in advance (gsr_forward_prealloc_dc,
// gsr_forward_views; arguments checked, P > 0).  A view whose buffer is too small is left unrendered.
static int forward_prealloc(const Scene& sc, int V, const Camera* cam, const ViewState* vs, const float* background,
                            const ForwardOptions& opt, hipStream_t caller, hipStream_t ps, bool debug,
                            int* num_rendered, int* rendered)
{
    int rc = forward_geometry(sc, V, cam, vs, opt, ps, debug, num_rendered);
    int fit[MAX_VIEWS], nf = 0;
    for (int v = 0; v < V && !rc; v++)
        if (binning_fits(vs[v], num_rendered[v])) fit[nf++] = v;
    if (!rc) rc = forward_render(sc, vs, num_rendered, fit, nf, background, opt.early_count, caller, ps, debug);
    if (rc) {
        stream_join(g_prefix, caller, ps);
        return rc;
    }
    for (int k = 0; k < nf; k++) rendered[fit[k]] = 1;
    return GSR_OK;
}

int gsr_forward_dc(gsr_resize_fn geometryBuffer, void* geometry_ctx, gsr_resize_fn binningBuffer, void* binning_ctx,
                gsr_resize_fn imageBuffer, void* image_ctx, int P, int D, int M, const float* background, int width,
                int height, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
                const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                float tan_fovx, float tan_fovy, bool prefiltered, float* out_color, float* depth, bool antialiasing,
                int* radii, bool debug, gsr_stream_t stream, int* num_rendered)
{
    *num_rendered = 0;
    if (P == 0) return GSR_OK;  // rasterize_points.cu:88 -- outputs stay as allocated
    char* gb = geometryBuffer(geometry_ctx, gsr_geometry_buffer_size(P));
    char* ib = imageBuffer(image_ctx, gsr_image_buffer_size(width, height));
    if (!gb || !ib) return fail(GSR_ERR_ALLOC, "resize callback returned NULL");
    int L = 0;
    int rc = gsr_forward_geometry_dc(gb, ib, P, D, M, width, height, means3D, dc, shs, colors_precomp, opacities, scales,
                                  scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx,
                                  tan_fovy, prefiltered, antialiasing, radii, debug, stream, &L);
    if (rc) return rc;
    char* bb = binningBuffer(binning_ctx, gsr_binning_buffer_size(L));
    if (!bb) return fail(GSR_ERR_ALLOC, "resize callback returned NULL");
    rc = gsr_forward_render(gb, bb, ib, P, L, background, width, height, colors_precomp, out_color, depth, radii,
                            debug, stream);
    if (rc) return rc;
    *num_rendered = L;
    return GSR_OK;
}

int gsr_forward_prealloc_dc(char* geometry_buffer, char* image_buffer, char* binning_buffer, size_t binning_capacity,
                         int P, int D, int M, const float* background, int width, int height, const float* means3D,
                         const float* dc, const float* shs, const float* colors_precomp, const float* opacities,
                         const float* scales, float scale_modifier, const float* rotations,
                         const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                         const float* cam_pos, float tan_fovx, float tan_fovy, bool prefiltered, bool antialiasing,
                         float* out_color, float* depth, int* radii, bool debug, gsr_stream_t stream,
                         int* num_rendered, int* rendered)
{
    *rendered = 0;
    *num_rendered = 0;
    if (P <= 0) return P < 0 ? fail(GSR_ERR_INVALID, "P must be >= 0") : GSR_OK;
    const Scene sc = {P, D, M, means3D, dc, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
                      cov3D_precomp, prefiltered, antialiasing, width, height};
    const Camera cam = {viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy};
    const ViewState vs = {geometry_buffer, image_buffer, binning_buffer, binning_capacity, out_color, depth, radii};
    int rc = forward_args_check(sc, vs);
    if (rc) return rc;
    hipStream_t caller = (hipStream_t)stream, ps = nullptr;
    rc = stream_fork(g_prefix, g_prefix_mode == 1, caller, &ps);
    if (rc) return rc;
    const ForwardOptions opt = {PREPROCESS_SINGLE, /*geometry_outputs=*/true, /*early_count=*/true};
    return forward_prealloc(sc, 1, &cam, &vs, background, opt, caller, ps, debug, num_rendered, rendered);
}

int gsr_forward_views(int V, int P, int D, int M, const float* background, int width, int height,
                      const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
                      const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                      const float* cov3D_precomp, const float* const* viewmatrices, const float* const* projmatrices,
                      const float* const* campos, const float* tan_fovx, const float* tan_fovy, bool prefiltered,
                      bool antialiasing, char* const* geometry_buffers, char* const* image_buffers,
                      char* const* binning_buffers, const size_t* binning_capacity, float* const* out_colors,
                      float* const* out_invdepths, int* const* radii, bool debug, gsr_stream_t stream,
                      int* num_rendered, int* rendered)
{
    if (V < 1 || V > MAX_VIEWS) return fail(GSR_ERR_INVALID, "V must be in [1, 16]");
    if (!viewmatrices || !projmatrices || !campos || !tan_fovx || !tan_fovy || !geometry_buffers || !image_buffers ||
        !binning_buffers || !binning_capacity || !out_colors || !out_invdepths || !num_rendered || !rendered)
        return fail(GSR_ERR_INVALID, "null per-view array");
    for (int v = 0; v < V; v++) {
        num_rendered[v] = 0;
        rendered[v] = 0;
    }
    if (P <= 0) return P < 0 ? fail(GSR_ERR_INVALID, "P must be >= 0") : GSR_OK;
    const Scene sc = {P, D, M, means3D, dc, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
                      cov3D_precomp, prefiltered, antialiasing, width, height};
    Camera cam[MAX_VIEWS];
    ViewState vs[MAX_VIEWS];
    for (int v = 0; v < V; v++) {
        cam[v] = {viewmatrices[v], projmatrices[v], campos[v], tan_fovx[v], tan_fovy[v]};
        vs[v] = {geometry_buffers[v], image_buffers[v], binning_buffers[v], binning_capacity[v], out_colors[v],
                 out_invdepths[v], radii ? radii[v] : nullptr};
        if (!vs[v].geometry || !vs[v].image) return fail(GSR_ERR_ALLOC, "null state buffer");
        if (!vs[v].out_color || !vs[v].invdepth) return fail(GSR_ERR_INVALID, "null per-view output");
        const int rc = forward_args_check(sc, vs[v]);
        if (rc) return rc;
    }
    // The binning prefix of all V views on the caller's stream, like the renders that follow (a
    // separate prefix stream would overlap nothing here -- it would fork from the caller's previous
    // work and the render would join it -- and each hop between the queues costs ~10 us of idle GPU).
    hipStream_t caller = (hipStream_t)stream;
    // GeometryState's means2D, depths, rgb and conic_opacity are read by nothing after the forward:
    // the batched forward does not write them
    const ForwardOptions opt = {PREPROCESS_VIEWS, /*geometry_outputs=*/false, /*early_count=*/true};
    return forward_prealloc(sc, V, cam, vs, background, opt, caller, caller, debug, num_rendered, rendered);
}

int gsr_alpha_views(int V, int width, int height, char* const* image_buffers, float* const* out_alphas,
                    gsr_stream_t stream)
{
    if (V < 1 || V > MAX_VIEWS) return fail(GSR_ERR_INVALID, "V must be in [1, 16]");
    if (width <= 0 || height <= 0) return fail(GSR_ERR_INVALID, "width and height must be > 0");
    if (!image_buffers || !out_alphas) return fail(GSR_ERR_INVALID, "null per-view array");
    for (int v = 0; v < V; v++)
        if (!image_buffers[v] || !out_alphas[v]) return fail(GSR_ERR_INVALID, "null image buffer or alpha output");
    const ImageLayout im = image_layout(width, height);
    AlphaJob jobs[MAX_VIEWS];
    for (int v = 0; v < V; v++) jobs[v] = {at<float>(image_buffers[v], im.off[IMG_FINAL_T]), out_alphas[v]};
    HIP_TRY(launch_alpha_batch(jobs, V, (size_t)width * height, (hipStream_t)stream));
    return GSR_OK;
}

// render_bwd's arguments for one view (P, R > 0), and the job of its backward tile order
static RenderBwdArgs render_bwd_args(const Scene& sc, const ViewState& vs, int R, const float* background,
                                     const float* dL_dpix, const float* dL_invdepths, const float* dL_dalphas,
                                     OrderJob* order)
{
    const int width = sc.width, height = sc.height;
    char *gb = vs.geometry, *ib = vs.image, *bb = vs.binning;
    const GeomLayout g = geom_layout(sc.P);
    const ImageLayout im = image_layout(width, height);
    const BinLayout b = bin_layout(R);
    const TileGrid tg(width, height);
    RenderBwdArgs r;
    r.ranges = at<uint2>(ib, im.off[IMG_RANGES]);
    r.tile_order = at<uint32_t>(ib, im.off[IMG_TILE_ORDER]);
    r.tile_work = at<uint32_t>(ib, im.off[IMG_TILE_WORK]);
    r.point_list = at<uint32_t>(bb, b.off[BIN_POINT_LIST]);
    r.W = width; r.H = height; r.grid_x = tg.gx;
    r.T = tg.T;
    r.bg = background;
    r.splat = at<float4>(gb, g.off[GEOM_SPLAT]);
    r.final_Ts = at<float>(ib, im.off[IMG_FINAL_T]);
    r.n_contrib = at<uint32_t>(ib, im.off[IMG_N_CONTRIB]);
    r.dL_dpixels = dL_dpix;
    r.dL_invdepths = dL_invdepths;
    r.dL_dalphas = dL_dalphas;
    r.grad_inst = at<float>(bb, b.off[BIN_GRAD_INST]);
    r.slot = slots_from_rect(tg.gx, tg.gy) ? nullptr : at<uint32_t>(bb, b.off[BIN_SLOT]);  // (render_bwd derives them)
    r.valid = at<uint32_t>(bb, b.off[BIN_VALID]);
    r.hit = at<uint8_t>(bb, b.off[BIN_HIT]);
    r.emit_start = at<uint32_t>(gb, g.off[GEOM_EMIT_START]);
    r.rec_mask = at<uint32_t>(gb, g.off[GEOM_REC_MASK]);
    *order = {nullptr, r.tile_work, at<uint32_t>(ib, im.off[IMG_TILE_ORDER])};
    return r;
}

// The backward of V >= 1 views of the same Gaussians, like the forward, exists once: backward_render,
// then backward_preprocess.  What the entry points differ in they pass in (BackwardOptions).
// The parameter gradients BACKWARD::preprocess writes (summed over the views) and their GSR_ACC_* bits
struct ParamGrads {
    float *dL_dcolor, *dL_dopacity, *dL_dmean3D, *dL_dcov3D, *dL_ddc, *dL_dsh, *dL_dscale, *dL_drot;
    unsigned accumulate;
};

// What every backward that reads the Gaussians' parameters checks of them (no HIP call).
// g: the gradients it writes; null for the camera gradient, which writes none
static int backward_scene_check(const Scene& sc, const ParamGrads* g)
{
    if (g && (g->accumulate & ~(unsigned)GSR_ACC_ALL)) return fail(GSR_ERR_INVALID, "unknown accumulate bits");
    if (sc.P < 0) return fail(GSR_ERR_INVALID, "P must be >= 0");
    if (g && sc.dc && !g->dL_ddc) return fail(GSR_ERR_INVALID, "dc given without dL_ddc");
    if (sc.dc && sc.colors_precomp)
        return fail(GSR_ERR_INVALID, "Please provide exactly one of either SHs or precomputed colors!");
    if (sc.dc && sc.M > 0 && (!sc.shs || (g && !g->dL_dsh)))
        return fail(GSR_ERR_INVALID,
                    g ? "dc given with M > 0 but shs/dL_dsh NULL" : "dc given with M > 0 but shs NULL");
    if (sc.P > 0 && (!sc.means3D || !sc.opacities || (!sc.cov3D_precomp && (!sc.scales || !sc.rotations))))
        return fail(GSR_ERR_INVALID, "null parameter array");
    return GSR_OK;
}

// The ABI's parallel per-view arrays (non-null: the entry point checks that ahead of its P == 0 return;
// their elements are read only here, after it) as ViewState[] and, with cameras (ca), Camera[], under the
// checks every batched backward applies: R[v] >= 0, no null camera, and with P > 0 no null state buffer a
// kernel would read -- geometry, image (null: no BACKWARD::render in this call), binning when R[v] > 0.
struct CameraArrays { const float *const *view, *const *proj, *const *campos, *tan_fovx, *tan_fovy; };
static int unpack_views(int V, int P, const int* R, const CameraArrays* ca, char* const* geometry, char* const* image,
                        char* const* binning, const int* const* radii, Camera* cam, ViewState* vs)
{
    for (int v = 0; v < V; v++) {
        if (R[v] < 0) return fail(GSR_ERR_INVALID, "R must be >= 0");
        if (ca && (!ca->view[v] || !ca->proj[v] || !ca->campos[v])) return fail(GSR_ERR_INVALID, "null camera");
        if (P > 0 && (!geometry[v] || (image && !image[v]) || (R[v] > 0 && !binning[v])))
            return fail(GSR_ERR_ALLOC, "null state buffer");
        if (ca) cam[v] = {ca->view[v], ca->proj[v], ca->campos[v], ca->tan_fovx[v], ca->tan_fovy[v]};
        vs[v] = {geometry[v], image ? image[v] : nullptr, binning[v], 0, nullptr, nullptr,
                 radii ? const_cast<int*>(radii[v]) : nullptr};  // (the backward only reads radii)
    }
    return GSR_OK;
}

// BACKWARD::render (rasterizer_impl.cu:399-418) of n views (arguments checked, P > 0; a view with R[v] == 0
// has no instances, so no records to write, and is skipped): every view's backward tile order (longest
// n_contrib first) in one launch, then their per-(tile, Gaussian) gradient records in one launch.
// dL_dalphas: null, or per view the gradient on the alpha output (gsr_alpha_views), null for a view without one
static int backward_render(const Scene& sc, int n, const ViewState* vs, const int* R, const float* const* dL_dpix,
                           const float* const* dL_invdepths, const float* const* dL_dalphas, const float* background,
                           bool debug, hipStream_t s)
{
    OrderJob oj[MAX_VIEWS];
    RenderBwdArgs ra[MAX_VIEWS];
    int nr = 0;
    for (int v = 0; v < n; v++) {
        if (R[v] == 0) continue;
        const float* dL_inv = dL_invdepths ? dL_invdepths[v] : nullptr;
        const float* dL_da = dL_dalphas ? dL_dalphas[v] : nullptr;
        ra[nr] = render_bwd_args(sc, vs[v], R[v], background, dL_dpix[v], dL_inv, dL_da, &oj[nr]);
        nr++;
    }
    if (nr) {
        ProfScope ps_(PK_TILE_ORDER, s);
        HIP_TRY(launch_tile_order_batch(oj, nr, ra[0].T, s));
    }
    if (nr) {
        ProfScope ps_(PK_RENDER_BWD, s);  // valid[] was cleared by the forward's tile sort
        HIP_TRY(launch_render_bwd_batch(ra, nr, ra[0].T, s));
    }
    DEBUG_SYNC(s);
    return GSR_OK;
}

// The parameters and flags that preprocess_bwd and the camera gradient read from the Scene (no outputs)
static void preprocess_bwd_params(PreprocessBwdArgs& p, const Scene& sc, bool has_invdepth)
{
    p.P = sc.P; p.D = sc.D; p.M = sc.dc ? sc.M + 1 : sc.M;
    p.means3D = sc.means3D; p.radii = nullptr; p.shs = sc.shs; p.dc = sc.dc;
    p.opacities = sc.opacities; p.scales = sc.scales; p.rotations = sc.rotations;
    p.scale_modifier = sc.scale_modifier;
    p.cov3D_precomp = sc.cov3D_precomp;
    p.antialiasing = sc.antialiasing;
    p.has_invdepth = has_invdepth;
    p.W = sc.width; p.H = sc.height;
}

// One view's part of preprocess_bwd's arguments (L: its num_rendered; vs.binning may be null when
// L == 0; vs.radii: what the forward wrote, null for the GeometryState's own)
static BwdView bwd_view(const Scene& sc, const Camera& cam, const ViewState& vs, int L, float* dL_dmean2D)
{
    char *gb = vs.geometry, *bb = vs.binning;
    const GeomLayout g = geom_layout(sc.P);
    const BinLayout b = bin_layout(L);
    BwdView bv;
    bv.view = cam.view; bv.proj = cam.proj; bv.campos = cam.campos;
    bv.focal_y = sc.height / (2.0f * cam.tan_fovy);
    bv.focal_x = sc.width / (2.0f * cam.tan_fovx);
    bv.tan_fovx = cam.tan_fovx; bv.tan_fovy = cam.tan_fovy;
    bv.radii = vs.radii ? vs.radii : at<int>(gb, g.off[GEOM_RADII]);
    bv.conic_opacity = at<float4>(gb, g.off[GEOM_CONIC_OPACITY]);
    bv.clamped = at<uint8_t>(gb, g.off[GEOM_CLAMPED]);
    bv.emit_start = at<uint32_t>(gb, g.off[GEOM_EMIT_START]);
    bv.tiles_touched = at<uint32_t>(gb, g.off[GEOM_TILES_TOUCHED]);
    bv.grad_inst = L > 0 ? at<float>(bb, b.off[BIN_GRAD_INST]) : nullptr;
    bv.valid = L > 0 ? at<uint32_t>(bb, b.off[BIN_VALID]) : nullptr;
    bv.rec_mask = at<uint32_t>(gb, g.off[GEOM_REC_MASK]);
    bv.dL_dmean2D = dL_dmean2D;
    return bv;
}

// The single view keeps its own launcher: one lane per Gaussian, gated on the caller's radii, which
// also writes the reference glue's other render-pass gradients.  (The V == 1 case of the batched one is
// another kernel instantiation, two lanes per Gaussian, whose sums round differently.)
enum PreprocessBwdLauncher { PREPROCESS_BWD_SINGLE, PREPROCESS_BWD_VIEWS };
struct BackwardOptions {
    PreprocessBwdLauncher preprocess;  // launch_preprocess_bwd_single (V == 1, the whole range) or _views
    int g_begin, g_end;                // the Gaussians [g_begin, g_end) whose gradient rows are written
    float *dL_dconic, *dL_dinvdepth;   // the single view's extras (null for batches)
};

// BACKWARD::preprocess (rasterizer_impl.cu:423-449) of V views (arguments checked, P > 0) with the gather of
// their gradient records: one pass over the Gaussians of the range.  has_invdepth: some view's records
// carry an inverse-depth gradient (a view rendered without one has zero invdepth fields in its records:
// subtracting their zero term leaves its gradients bit-identical)
static int backward_preprocess(const Scene& sc, int V, const Camera* cam, const ViewState* vs, const int* R,
                               bool has_invdepth, float* const* dL_dmean2D, const ParamGrads& g,
                               const BackwardOptions& opt, bool debug, hipStream_t s)
{
    PreprocessBwdViewsArgs A;
    PreprocessBwdArgs& p = A.a;
    preprocess_bwd_params(p, sc, has_invdepth);
    p.dL_dconic = opt.dL_dconic; p.dL_dinvdepth = opt.dL_dinvdepth;
    p.dL_dopacity = g.dL_dopacity; p.dL_dcolor = g.dL_dcolor;
    p.dL_dmean3D = g.dL_dmean3D; p.dL_dcov3D = g.dL_dcov3D;
    p.dL_ddc = sc.dc ? g.dL_ddc : nullptr; p.dL_dsh = (sc.shs && sc.M > 0) ? g.dL_dsh : nullptr;
    p.dL_dscale = g.dL_dscale; p.dL_drot = g.dL_drot;
    p.acc = g.accumulate;
    A.V = V;
    A.g_begin = opt.g_begin;
    A.g_end = opt.g_end;
    for (int v = 0; v < V; v++) A.v[v] = bwd_view(sc, cam[v], vs[v], R[v], dL_dmean2D[v]);
    const bool single = opt.preprocess == PREPROCESS_BWD_SINGLE;
    if (single) p.radii = A.v[0].radii;  // (the one-lane kernel gates on them)
    {
        ProfScope ps_(PK_PREPROCESS_BWD, s);
        HIP_TRY(single ? launch_preprocess_bwd_single(A, s) : launch_preprocess_bwd_views(A, s));
    }
    DEBUG_SYNC(s);
    return GSR_OK;
}

int gsr_backward_alpha(int P, int D, int M, int R, const float* background, int width, int height,
                       const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
                       const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                       const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                       const float* campos, float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer,
                       char* binning_buffer, char* image_buffer, const float* dL_dpix, const float* dL_invdepths,
                       const float* dL_dalphas, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                       float* dL_dcolor, float* dL_dinvdepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_ddc,
                       float* dL_dsh, float* dL_dscale, float* dL_drot, bool antialiasing, bool debug,
                       unsigned accumulate, gsr_stream_t stream)
{
    const Scene sc = {P, D, M, means3D, dc, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
                      cov3D_precomp, /*prefiltered=*/false, antialiasing, width, height};
    const Camera cam = {viewmatrix, projmatrix, campos, tan_fovx, tan_fovy};
    const ViewState vs = {geom_buffer, image_buffer, binning_buffer, 0, nullptr, nullptr, const_cast<int*>(radii)};
    const ParamGrads g = {dL_dcolor, dL_dopacity, dL_dmean3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscale, dL_drot,
                          accumulate};
    int rc = backward_scene_check(sc, &g);
    if (rc) return rc;
    if (R < 0) return fail(GSR_ERR_INVALID, "R must be >= 0");
    if (P == 0) return GSR_OK;
    if (R > 0 && !binning_buffer) return fail(GSR_ERR_ALLOC, "null binning buffer");
    if (!geom_buffer || (R > 0 && !image_buffer)) return fail(GSR_ERR_ALLOC, "null state buffer");
    if (R > 0 && !dL_dpix) return fail(GSR_ERR_INVALID, "null dL_dpix");
    if (dL_invdepths && !dL_dinvdepth) return fail(GSR_ERR_INVALID, "dL_dinvdepth must be given with dL_invdepths");
    hipStream_t s = (hipStream_t)stream;
    if (R > 0) {  // (no instances: no records to write)
        rc = backward_render(sc, 1, &vs, &R, &dL_dpix, dL_invdepths ? &dL_invdepths : nullptr,
                             dL_dalphas ? &dL_dalphas : nullptr, background, debug, s);
        if (rc) return rc;
    }
    const BackwardOptions opt = {PREPROCESS_BWD_SINGLE, 0, P, dL_dconic, dL_dinvdepth};
    return backward_preprocess(sc, 1, &cam, &vs, &R, dL_invdepths != nullptr, &dL_dmean2D, g, opt, debug, s);
}

int gsr_backward_dc_acc(int P, int D, int M, int R, const float* background, int width, int height,
                        const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
                        const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                        const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                        const float* campos, float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer,
                        char* binning_buffer, char* image_buffer, const float* dL_dpix, const float* dL_invdepths,
                        float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                        float* dL_dinvdepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_ddc, float* dL_dsh,
                        float* dL_dscale, float* dL_drot, bool antialiasing, bool debug, unsigned accumulate,
                        gsr_stream_t stream)
{
    return gsr_backward_alpha(P, D, M, R, background, width, height, means3D, dc, shs, colors_precomp, opacities,
                              scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
                              tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix,
                              dL_invdepths, /*dL_dalphas=*/nullptr, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor,
                              dL_dinvdepth, dL_dmean3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscale, dL_drot, antialiasing,
                              debug, accumulate, stream);
}

int gsr_backward_dc(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                    const float* dc, const float* shs, const float* colors_precomp, const float* opacities,
                    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                    const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                    float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                    const float* dL_dpix, const float* dL_invdepths, float* dL_dmean2D, float* dL_dconic,
                    float* dL_dopacity, float* dL_dcolor, float* dL_dinvdepth, float* dL_dmean3D, float* dL_dcov3D,
                    float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot, bool antialiasing, bool debug,
                    gsr_stream_t stream)
{
    return gsr_backward_dc_acc(P, D, M, R, background, width, height, means3D, dc, shs, colors_precomp, opacities,
                               scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
                               tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix,
                               dL_invdepths, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dinvdepth, dL_dmean3D,
                               dL_dcov3D, dL_ddc, dL_dsh, dL_dscale, dL_drot, antialiasing, debug, 0u, stream);
}

int gsr_backward_render(int P, int R, const float* background, int width, int height, char* geom_buffer,
                        char* binning_buffer, char* image_buffer, const float* dL_dpix, const float* dL_invdepths,
                        bool debug, gsr_stream_t stream)
{
    if (P < 0 || R < 0) return fail(GSR_ERR_INVALID, "P and R must be >= 0");
    if (P == 0 || R == 0) return GSR_OK;
    if (!geom_buffer || !image_buffer || !binning_buffer) return fail(GSR_ERR_ALLOC, "null state buffer");
    if (!dL_dpix) return fail(GSR_ERR_INVALID, "null dL_dpix");
    Scene sc = {};
    sc.P = P; sc.width = width; sc.height = height;  // (all that BACKWARD::render reads)
    const ViewState vs = {geom_buffer, image_buffer, binning_buffer, 0, nullptr, nullptr, nullptr};
    return backward_render(sc, 1, &vs, &R, &dL_dpix, dL_invdepths ? &dL_invdepths : nullptr, nullptr, background,
                           debug, (hipStream_t)stream);
}

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
                                  unsigned accumulate, gsr_stream_t stream)
{
    return gsr_backward_preprocess_views_range(V, P, D, M, R, width, height, means3D, dc, shs, colors_precomp,
                                               opacities, scales, scale_modifier, rotations, cov3D_precomp,
                                               viewmatrices, projmatrices, campos, tan_fovx, tan_fovy, radii,
                                               geom_buffers, binning_buffers, has_invdepth, dL_dmean2D, dL_dcolor,
                                               dL_dopacity, dL_dmean3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscale, dL_drot,
                                               antialiasing, debug, accumulate, 0, P, stream);
}

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
                                        gsr_stream_t stream)
{
    if (V < 1 || V > MAX_VIEWS) return fail(GSR_ERR_INVALID, "V must be in [1, 16]");
    if (g_begin < 0 || g_end > P || g_begin > g_end) return fail(GSR_ERR_INVALID, "range outside [0, P)");
    const Scene sc = {P, D, M, means3D, dc, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
                      cov3D_precomp, /*prefiltered=*/false, antialiasing, width, height};
    const ParamGrads g = {dL_dcolor, dL_dopacity, dL_dmean3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscale, dL_drot,
                          accumulate};
    int rc = backward_scene_check(sc, &g);
    if (rc) return rc;
    if (!R || !viewmatrices || !projmatrices || !campos || !tan_fovx || !tan_fovy || !geom_buffers ||
        !binning_buffers || !dL_dmean2D)
        return fail(GSR_ERR_INVALID, "null per-view array");
    if (P == 0) return GSR_OK;
    const CameraArrays ca = {viewmatrices, projmatrices, campos, tan_fovx, tan_fovy};
    Camera cam[MAX_VIEWS];
    ViewState vs[MAX_VIEWS];
    rc = unpack_views(V, P, R, &ca, geom_buffers, nullptr, binning_buffers, radii, cam, vs);
    if (rc) return rc;
    for (int v = 0; v < V; v++)
        if (!dL_dmean2D[v]) return fail(GSR_ERR_INVALID, "null per-view gradient");
    const BackwardOptions opt = {PREPROCESS_BWD_VIEWS, g_begin, g_end, nullptr, nullptr};
    return backward_preprocess(sc, V, cam, vs, R, has_invdepth, dL_dmean2D, g, opt, debug, (hipStream_t)stream);
}

size_t gsr_camera_grad_workspace_size(int V, int P) { return camera_bwd_workspace_bytes(V, P); }

int gsr_backward_camera_views(int V, int P, int D, int M, const int* R, int width, int height, const float* means3D,
                              const float* dc, const float* shs, const float* colors_precomp,
                              const float* opacities, const float* scales, float scale_modifier,
                              const float* rotations, const float* cov3D_precomp, const float* const* viewmatrices,
                              const float* const* projmatrices, const float* const* campos, const float* tan_fovx,
                              const float* tan_fovy, char* const* geom_buffers, char* const* binning_buffers,
                              bool has_invdepth, bool antialiasing, char* workspace, float* dL_dviewmatrix,
                              float* dL_dprojmatrix, float* dL_dcampos, bool debug, gsr_stream_t stream)
{
    if (V < 1 || V > MAX_VIEWS) return fail(GSR_ERR_INVALID, "V must be in [1, 16]");
    if (!workspace || !dL_dviewmatrix || !dL_dprojmatrix || !dL_dcampos)
        return fail(GSR_ERR_INVALID, "null workspace or camera gradient");
    const Scene sc = {P, D, M, means3D, dc, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
                      cov3D_precomp, /*prefiltered=*/false, antialiasing, width, height};
    int rc = backward_scene_check(sc, nullptr);
    if (rc) return rc;
    if (!R || !viewmatrices || !projmatrices || !campos || !tan_fovx || !tan_fovy || !geom_buffers ||
        !binning_buffers)
        return fail(GSR_ERR_INVALID, "null per-view array");
    const CameraArrays ca = {viewmatrices, projmatrices, campos, tan_fovx, tan_fovy};
    Camera cam[MAX_VIEWS];
    ViewState vs[MAX_VIEWS];
    rc = unpack_views(V, P, R, &ca, geom_buffers, nullptr, binning_buffers, nullptr, cam, vs);
    if (rc) return rc;
    CameraBwdArgs A = {};
    preprocess_bwd_params(A.a, sc, has_invdepth);  // (no gradient outputs)
    A.V = V;
    for (int v = 0; v < V && P > 0; v++) A.v[v] = bwd_view(sc, cam[v], vs[v], R[v], nullptr);
    A.partial = reinterpret_cast<float*>(workspace);
    A.dL_dview = dL_dviewmatrix; A.dL_dproj = dL_dprojmatrix; A.dL_dcampos = dL_dcampos;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps_(PK_CAMERA_BWD, s);
        HIP_TRY(launch_camera_bwd_views(A, s));
    }
    DEBUG_SYNC(s);
    return GSR_OK;
}

int gsr_backward_render_views_alpha(int V, int P, const int* R, const float* background, int width, int height,
                                    char* const* geom_buffers, char* const* binning_buffers,
                                    char* const* image_buffers, const float* const* dL_dpix,
                                    const float* const* dL_invdepths, const float* const* dL_dalphas, bool debug,
                                    gsr_stream_t stream)
{
    if (V < 1 || V > MAX_VIEWS) return fail(GSR_ERR_INVALID, "V must be in [1, 16]");
    if (!R || !geom_buffers || !binning_buffers || !image_buffers || !dL_dpix)
        return fail(GSR_ERR_INVALID, "null per-view array");
    if (P <= 0) return P < 0 ? fail(GSR_ERR_INVALID, "P must be >= 0") : GSR_OK;
    Scene sc = {};
    sc.P = P; sc.width = width; sc.height = height;  // (all that BACKWARD::render reads)
    ViewState vs[MAX_VIEWS];
    const int rc = unpack_views(V, P, R, nullptr, geom_buffers, image_buffers, binning_buffers, nullptr, nullptr, vs);
    if (rc) return rc;
    for (int v = 0; v < V; v++)
        if (!dL_dpix[v] || (dL_invdepths && !dL_invdepths[v])) return fail(GSR_ERR_INVALID, "null per-view gradient");
    return backward_render(sc, V, vs, R, dL_dpix, dL_invdepths, dL_dalphas, background, debug, (hipStream_t)stream);
}

int gsr_backward_render_views(int V, int P, const int* R, const float* background, int width, int height,
                              char* const* geom_buffers, char* const* binning_buffers, char* const* image_buffers,
                              const float* const* dL_dpix, const float* const* dL_invdepths, bool debug,
                              gsr_stream_t stream)
{
    return gsr_backward_render_views_alpha(V, P, R, background, width, height, geom_buffers, binning_buffers,
                                           image_buffers, dL_dpix, dL_invdepths, /*dL_dalphas=*/nullptr, debug, stream);
}

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
                       gsr_stream_t stream)
{
    return gsr_backward_views_alpha(V, P, D, M, R, background, width, height, means3D, dc, shs, colors_precomp,
                                    opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrices,
                                    projmatrices, campos, tan_fovx, tan_fovy, radii, geom_buffers, binning_buffers,
                                    image_buffers, dL_dpix, dL_invdepths, /*dL_dalphas=*/nullptr, dL_dmean2D, dL_dcolor,
                                    dL_dopacity, dL_dmean3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscale, dL_drot,
                                    antialiasing, debug, accumulate, stream);
}

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
                             bool antialiasing, bool debug, unsigned accumulate, gsr_stream_t stream)
{
    const int rc = gsr_backward_render_views_alpha(V, P, R, background, width, height, geom_buffers, binning_buffers,
                                                   image_buffers, dL_dpix, dL_invdepths, dL_dalphas, debug, stream);
    if (rc || P <= 0) return rc;
    return gsr_backward_preprocess_views(V, P, D, M, R, width, height, means3D, dc, shs, colors_precomp, opacities,
                                         scales, scale_modifier, rotations, cov3D_precomp, viewmatrices,
                                         projmatrices, campos, tan_fovx, tan_fovy, radii, geom_buffers,
                                         binning_buffers, dL_invdepths != nullptr, dL_dmean2D, dL_dcolor,
                                         dL_dopacity, dL_dmean3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscale, dL_drot,
                                         antialiasing, debug, accumulate, stream);
}

// ---- the non-dc entry points: the reference's Rasterizer API (rasterizer.h:31-90) ----
int gsr_forward_geometry(char* geometry_buffer, char* image_buffer, int P, int D, int M, int width, int height,
                         const float* means3D, const float* shs, const float* colors_precomp,
                         const float* opacities, const float* scales, float scale_modifier,
                         const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                         const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                         bool prefiltered, bool antialiasing, int* radii, bool debug, gsr_stream_t stream,
                         int* num_rendered)
{
    return gsr_forward_geometry_dc(geometry_buffer, image_buffer, P, D, M, width, height, means3D, nullptr, shs,
                                   colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp,
                                   viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, antialiasing,
                                   radii, debug, stream, num_rendered);
}

int gsr_forward(gsr_resize_fn geometryBuffer, void* geometry_ctx, gsr_resize_fn binningBuffer, void* binning_ctx,
                gsr_resize_fn imageBuffer, void* image_ctx, int P, int D, int M, const float* background, int width,
                int height, const float* means3D, const float* shs, const float* colors_precomp,
                const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                float tan_fovx, float tan_fovy, bool prefiltered, float* out_color, float* depth, bool antialiasing,
                int* radii, bool debug, gsr_stream_t stream, int* num_rendered)
{
    return gsr_forward_dc(geometryBuffer, geometry_ctx, binningBuffer, binning_ctx, imageBuffer, image_ctx, P, D, M,
                          background, width, height, means3D, nullptr, shs, colors_precomp, opacities, scales,
                          scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx,
                          tan_fovy, prefiltered, out_color, depth, antialiasing, radii, debug, stream, num_rendered);
}

int gsr_forward_prealloc(char* geometry_buffer, char* image_buffer, char* binning_buffer, size_t binning_capacity,
                         int P, int D, int M, const float* background, int width, int height, const float* means3D,
                         const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                         float scale_modifier, const float* rotations, const float* cov3D_precomp,
                         const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                         float tan_fovy, bool prefiltered, bool antialiasing, float* out_color, float* depth,
                         int* radii, bool debug, gsr_stream_t stream, int* num_rendered, int* rendered)
{
    return gsr_forward_prealloc_dc(geometry_buffer, image_buffer, binning_buffer, binning_capacity, P, D, M,
                                   background, width, height, means3D, nullptr, shs, colors_precomp, opacities,
                                   scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos,
                                   tan_fovx, tan_fovy, prefiltered, antialiasing, out_color, depth, radii, debug,
                                   stream, num_rendered, rendered);
}

int gsr_backward(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                 const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                 float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                 const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                 char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix,
                 const float* dL_invdepths, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                 float* dL_dinvdepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                 float* dL_drot, bool antialiasing, bool debug, gsr_stream_t stream)
{
    return gsr_backward_dc(P, D, M, R, background, width, height, means3D, nullptr, shs, colors_precomp, opacities,
                           scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx,
                           tan_fovy, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_invdepths,
                           dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dinvdepth, dL_dmean3D, dL_dcov3D, nullptr,
                           dL_dsh, dL_dscale, dL_drot, antialiasing, debug, stream);
}

// ---- sparse Adam (adam.hip) ----
int gsr_adam_update(float* param, const float* param_grad, float* exp_avg, float* exp_avg_sq, const bool* visible,
                    float lr, float b1, float b2, float eps, int N, int M, gsr_stream_t stream)
{
    if (N < 0 || M < 0) return fail(GSR_ERR_INVALID, "N and M must be >= 0");
    if ((size_t)N * M == 0) return GSR_OK;
    if ((size_t)N * M >= 0xFFFFFFF0ull) return fail(GSR_ERR_INVALID, "N*M must be < 2^32");
    if (!param || !param_grad || !exp_avg || !exp_avg_sq || !visible) return fail(GSR_ERR_INVALID, "null pointer");
    AdamArgs a;
    a.param = param; a.grad = param_grad; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq;
    a.visible = reinterpret_cast<const uint8_t*>(visible);
    a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.N = N; a.M = M;
    HIP_TRY(launch_adam_update(a, (hipStream_t)stream));
    return GSR_OK;
}

int gsr_adam_update_multi(int n_groups, float* const* params, const float* const* param_grads,
                          float* const* exp_avgs, float* const* exp_avg_sqs, const int* Ms, const float* lrs,
                          const float* epss, const bool* visible, float b1, float b2, int N, gsr_stream_t stream)
{
    if (n_groups < 0 || N < 0) return fail(GSR_ERR_INVALID, "n_groups and N must be >= 0");
    if (n_groups == 0 || N == 0) return GSR_OK;
    if (!params || !param_grads || !exp_avgs || !exp_avg_sqs || !Ms || !lrs || !epss || !visible)
        return fail(GSR_ERR_INVALID, "null pointer");
    std::vector<AdamArgs> g((size_t)n_groups);
    for (int i = 0; i < n_groups; i++) {
        if (Ms[i] < 0) return fail(GSR_ERR_INVALID, "M must be >= 0");
        if ((size_t)N * Ms[i] >= 0xFFFFFFF0ull) return fail(GSR_ERR_INVALID, "N*M must be < 2^32");
        if (Ms[i] > 0 && (!params[i] || !param_grads[i] || !exp_avgs[i] || !exp_avg_sqs[i]))
            return fail(GSR_ERR_INVALID, "null group pointer");
        AdamArgs& a = g[i];
        a.param = params[i]; a.grad = param_grads[i]; a.exp_avg = exp_avgs[i]; a.exp_avg_sq = exp_avg_sqs[i];
        a.visible = reinterpret_cast<const uint8_t*>(visible);
        a.lr = lrs[i]; a.b1 = b1; a.b2 = b2; a.eps = epss[i]; a.N = N; a.M = Ms[i];
    }
    HIP_TRY(launch_adam_update_multi(g.data(), n_groups, (hipStream_t)stream));
    return GSR_OK;
}

// ---- fused_ssim.h ----
int gsr_ssim_forward(int planes, int H, int W, float C1, float C2, const float* img1, const float* img2,
                     float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream)
{
    if (planes < 0 || H < 0 || W < 0) return fail(GSR_ERR_INVALID, "negative image size");
    if ((size_t)planes * H * W == 0) return GSR_OK;
    if (!img1 || !img2 || !ssim_map) return fail(GSR_ERR_INVALID, "null pointer");
    const bool train = dm_dmu1 && dm_dsigma1_sq && dm_dsigma12;
    HIP_TRY(launch_ssim_fwd(planes, H, W, C1, C2, img1, img2, ssim_map, train ? dm_dmu1 : nullptr,
                            train ? dm_dsigma1_sq : nullptr, train ? dm_dsigma12 : nullptr, (hipStream_t)stream));
    return GSR_OK;
}

int gsr_ssim_backward(int planes, int H, int W, float C1, float C2, const float* img1, const float* img2,
                      const float* dL_dmap, const float* dm_dmu1, const float* dm_dsigma1_sq,
                      const float* dm_dsigma12, float* dL_dimg1, void* stream)
{
    (void)C1;
    (void)C2;  // folded into the forward's partial derivatives
    if (planes < 0 || H < 0 || W < 0) return fail(GSR_ERR_INVALID, "negative image size");
    if ((size_t)planes * H * W == 0) return GSR_OK;
    if (!img1 || !img2 || !dL_dmap || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg1)
        return fail(GSR_ERR_INVALID, "null pointer");
    HIP_TRY(launch_ssim_bwd(planes, H, W, img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1,
                            (hipStream_t)stream));
    return GSR_OK;
}

// the loss entry points' shared argument checks (no HIP call); *empty: a zero size, nothing to do
static int photo_loss_args(int V, int C, int H, int W, float lambda_dssim, const float* const* gt, bool* empty,
                           PhotoViews* out)
{
    *empty = true;
    if (V < 0 || C < 0 || H < 0 || W < 0) return fail(GSR_ERR_INVALID, "negative image size");
    if (V > MAX_VIEWS) return fail(GSR_ERR_INVALID, "V must be <= 16");
    if (!(lambda_dssim >= 0.f && lambda_dssim <= 1.f)) return fail(GSR_ERR_INVALID, "lambda_dssim must be in [0, 1]");
    if ((size_t)V * C == 0 || (size_t)H * W == 0) return GSR_OK;
    if ((size_t)V * C > 0x7FFFFFFFu) return fail(GSR_ERR_INVALID, "too many planes");
    if (!gt) return fail(GSR_ERR_INVALID, "null pointer");
    out->V = V;
    out->C = C;
    for (int v = 0; v < MAX_VIEWS; v++) {
        if (v < V && !gt[v]) return fail(GSR_ERR_INVALID, "null ground-truth pointer");
        out->gt[v] = v < V ? gt[v] : nullptr;
    }
    *empty = false;
    return GSR_OK;
}

size_t gsr_photo_loss_workspace_size(int V, int C, int H, int W)
{
    return V > MAX_VIEWS ? 0 : photo_loss_workspace_bytes(V, C, H, W);
}

int gsr_photo_loss_forward(int V, int C, int H, int W, float lambda_dssim, int clamp, const float* img,
                           const float* const* gt, float* loss, float* dm_dmu1, float* dm_dsigma1_sq,
                           float* dm_dsigma12, void* workspace, void* stream)
{
    PhotoViews pv;
    bool empty;
    const int rc = photo_loss_args(V, C, H, W, lambda_dssim, gt, &empty, &pv);
    if (rc || empty) return rc;
    if (!img || !loss || !workspace) return fail(GSR_ERR_INVALID, "null pointer");
    const bool train = dm_dmu1 && dm_dsigma1_sq && dm_dsigma12;
    HIP_TRY(launch_photo_loss_fwd(pv, H, W, lambda_dssim, clamp != 0, img, loss, train ? dm_dmu1 : nullptr,
                                  train ? dm_dsigma1_sq : nullptr, train ? dm_dsigma12 : nullptr, workspace,
                                  (hipStream_t)stream));
    return GSR_OK;
}

int gsr_photo_loss_backward(int V, int C, int H, int W, float lambda_dssim, int clamp, const float* img,
                            const float* const* gt, const float* dL_dloss, const float* dm_dmu1,
                            const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg, void* stream)
{
    PhotoViews pv;
    bool empty;
    const int rc = photo_loss_args(V, C, H, W, lambda_dssim, gt, &empty, &pv);
    if (rc || empty) return rc;
    if (!img || !dL_dloss || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg)
        return fail(GSR_ERR_INVALID, "null pointer");
    HIP_TRY(launch_photo_loss_bwd(pv, H, W, lambda_dssim, clamp != 0, img, dL_dloss, dm_dmu1, dm_dsigma1_sq,
                                  dm_dsigma12, dL_dimg, (hipStream_t)stream));
    return GSR_OK;
}

// the view-loss entry points' shared argument checks (no HIP call); *empty: a zero size, nothing to do
static int view_loss_args(int V, int C, int H, int W, float lambda_dssim, int clamp, const float* const* gt,
                          const float* exposure, const float* const* alpha_mask, const float* invdepth,
                          const float* const* invdepth_target, const float* const* depth_mask, float depth_weight,
                          bool* empty, ViewLossArgs* out)
{
    const int rc = photo_loss_args(V, C, H, W, lambda_dssim, gt, empty, &out->pv);
    if (rc) return rc;
    if (!(depth_weight >= 0.f && depth_weight <= 3.402823466e38f))  // NaN and inf included
        return fail(GSR_ERR_INVALID, "depth_weight must be finite and >= 0");
    if (*empty) return GSR_OK;
    *empty = true;
    if ((size_t)H * W >= ((size_t)1 << 30)) return fail(GSR_ERR_INVALID, "H*W must be < 2^30");  // 32-bit byte offsets
    if (exposure && C != 3) return fail(GSR_ERR_INVALID, "exposure needs C == 3");
    if (invdepth_target && !invdepth) return fail(GSR_ERR_INVALID, "invdepth_target without invdepth");
    if (depth_mask && !invdepth_target) return fail(GSR_ERR_INVALID, "depth_mask without invdepth_target");
    for (int v = 0; v < MAX_VIEWS; v++) {
        out->mask[v] = alpha_mask && v < V ? alpha_mask[v] : nullptr;
        out->target[v] = invdepth_target && v < V ? invdepth_target[v] : nullptr;
        out->dmask[v] = depth_mask && v < V ? depth_mask[v] : nullptr;
    }
    out->exposure = exposure;
    out->invdepth = invdepth;
    out->depth_weight = depth_weight;
    out->clamp = clamp != 0;
    *empty = false;
    return GSR_OK;
}

size_t gsr_view_loss_workspace_size(int V, int C, int H, int W)
{
    return V > MAX_VIEWS ? 0 : view_loss_workspace_bytes(V, C, H, W);
}

int gsr_view_loss_forward(int V, int C, int H, int W, float lambda_dssim, int clamp, const float* img,
                          const float* const* gt, const float* exposure, const float* const* alpha_mask,
                          const float* invdepth, const float* const* invdepth_target,
                          const float* const* depth_mask, float depth_weight, float* loss, float* dm_dmu1,
                          float* dm_dsigma1_sq, float* dm_dsigma12, void* workspace, void* stream)
{
    ViewLossArgs a;
    bool empty;
    const int rc = view_loss_args(V, C, H, W, lambda_dssim, clamp, gt, exposure, alpha_mask, invdepth,
                                  invdepth_target, depth_mask, depth_weight, &empty, &a);
    if (rc || empty) return rc;
    if (!img || !loss || !workspace) return fail(GSR_ERR_INVALID, "null pointer");
    const bool train = dm_dmu1 && dm_dsigma1_sq && dm_dsigma12;
    HIP_TRY(launch_view_loss_fwd(a, H, W, lambda_dssim, img, loss, train ? dm_dmu1 : nullptr,
                                 train ? dm_dsigma1_sq : nullptr, train ? dm_dsigma12 : nullptr, workspace,
                                 (hipStream_t)stream));
    return GSR_OK;
}

int gsr_view_loss_backward(int V, int C, int H, int W, float lambda_dssim, int clamp, const float* img,
                           const float* const* gt, const float* exposure, const float* const* alpha_mask,
                           const float* invdepth, const float* const* invdepth_target,
                           const float* const* depth_mask, float depth_weight, const float* dL_dloss,
                           const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_draw,
                           float* dL_dexposure, float* dL_dinvdepth, void* workspace, void* stream)
{
    ViewLossArgs a;
    bool empty;
    const int rc = view_loss_args(V, C, H, W, lambda_dssim, clamp, gt, exposure, alpha_mask, invdepth,
                                  invdepth_target, depth_mask, depth_weight, &empty, &a);
    if (rc || empty) return rc;
    if (!img || !dL_dloss || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_draw)
        return fail(GSR_ERR_INVALID, "null pointer");
    if (exposure && (!dL_dexposure || !workspace))
        return fail(GSR_ERR_INVALID, "null pointer (exposure needs dL_dexposure and the workspace)");
    HIP_TRY(launch_view_loss_bwd(a, H, W, lambda_dssim, img, dL_dloss, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_draw,
                                 dL_dexposure, invdepth ? dL_dinvdepth : nullptr, workspace, (hipStream_t)stream));
    return GSR_OK;
}

// ---- densification statistics (densify_stats.hip) ----
int gsr_densification_stats(int V, int P, const float* viewspace_grads, const int* radii, float* max_radii2D,
                            float* accum, long accum_stride, float* denom, long denom_stride,
                            float* visible_count, gsr_stream_t stream)
{
    if (V < 0 || P < 0) return fail(GSR_ERR_INVALID, "V and P must be >= 0");
    if (accum_stride < 1 || denom_stride < 1) return fail(GSR_ERR_INVALID, "strides must be >= 1");
    if (V == 0 || P == 0) return GSR_OK;
    if (!viewspace_grads || !radii || !max_radii2D || !accum || !denom) return fail(GSR_ERR_INVALID, "null pointer");
    const DensifyStatsArgs a = {V, P, viewspace_grads, radii, max_radii2D, accum, denom, accum_stride, denom_stride,
                                visible_count};
    HIP_TRY(launch_densify_stats(a, (hipStream_t)stream));
    return GSR_OK;
}

// ---- parameter activations (activations.hip) ----
int gsr_activate_forward(int P, const float* scaling, const float* rotation, const float* opacity, float* scales,
                         float* rotations, float* opacities, gsr_stream_t stream)
{
    if (P < 0) return fail(GSR_ERR_INVALID, "P must be >= 0");
    if (P == 0) return GSR_OK;
    if (!scaling || !rotation || !opacity || !scales || !rotations || !opacities)
        return fail(GSR_ERR_INVALID, "null pointer");
    const ActivateFwdArgs a = {P, scaling, rotation, opacity, scales, rotations, opacities};
    HIP_TRY(launch_activate_fwd(a, (hipStream_t)stream));
    return GSR_OK;
}

int gsr_activate_backward(int P, const float* scales, const float* rotation, const float* opacities,
                          const float* dL_dscales, const float* dL_drotations, const float* dL_dopacities,
                          float* dL_dscaling, float* dL_drotation, float* dL_dopacity, int accumulate_mask,
                          gsr_stream_t stream)
{
    if (P < 0) return fail(GSR_ERR_INVALID, "P must be >= 0");
    if (accumulate_mask & ~7) return fail(GSR_ERR_INVALID, "unknown accumulate bits");
    if (P == 0) return GSR_OK;
    // a group runs when both its incoming gradient and its destination are given
    const bool s = dL_dscales && dL_dscaling, r = dL_drotations && dL_drotation, o = dL_dopacities && dL_dopacity;
    if (s && !scales) return fail(GSR_ERR_INVALID, "null pointer (scales)");
    if (r && !rotation) return fail(GSR_ERR_INVALID, "null pointer (rotation)");
    if (o && !opacities) return fail(GSR_ERR_INVALID, "null pointer (opacities)");
    const ActivateBwdArgs a = {P, scales, rotation, opacities, s ? dL_dscales : nullptr, r ? dL_drotations : nullptr,
                               o ? dL_dopacities : nullptr, s ? dL_dscaling : nullptr, r ? dL_drotation : nullptr,
                               o ? dL_dopacity : nullptr, (uint32_t)accumulate_mask};
    HIP_TRY(launch_activate_bwd(a, (hipStream_t)stream));
    return GSR_OK;
}

// ---- densify_and_prune (densify.hip) ----
size_t gsr_densify_workspace_size(int P) { return densify_workspace_bytes(P); }

int gsr_densify_rows_per_workgroup(void) { return DENSIFY_ROWS_PER_WG; }

int gsr_densify_plan(int P, const float* accum, long accum_stride, const float* denom, long denom_stride,
                     const float* scaling, const float* opacity, float max_grad, float dense_extent,
                     float min_opacity, float big_extent, int N, char* workspace, int* counts, gsr_stream_t stream)
{
    if (P < 0) return fail(GSR_ERR_INVALID, "P must be >= 0");
    if (N < 1) return fail(GSR_ERR_INVALID, "N must be >= 1");
    if (accum_stride < 1 || denom_stride < 1) return fail(GSR_ERR_INVALID, "strides must be >= 1");
    if (!counts) return fail(GSR_ERR_INVALID, "null pointer (counts)");
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (P == 0) return GSR_OK;
    if (!accum || !denom || !scaling || !opacity || !workspace) return fail(GSR_ERR_INVALID, "null pointer");
    uint32_t* h;
    int rc = pinned(MAX_VIEWS - 1, &h);
    if (rc) return rc;
    h += 8;  // (the words the forward does not use)
    const DensifyPlanArgs a = {P, N, accum, denom, accum_stride, denom_stride, scaling, opacity, max_grad,
                               dense_extent, min_opacity, big_extent, densify_split_shrink(N)};
    for (int k = 0; k < 5; k++) h[k] = L_PENDING;  // (every count is <= P < 2^31)
    HIP_TRY(launch_densify_plan(a, workspace, h, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int k = 0; k < 5; k++)
        if (__atomic_load_n(&h[k], __ATOMIC_ACQUIRE) == L_PENDING)
            return fail(GSR_ERR_HIP, "the plan did not publish its counts");
    const uint64_t keep_orig = h[0], keep_clone = h[1], split = h[2], keep_split = h[3], clone = h[4];
    const uint64_t after = keep_orig + keep_clone + (uint64_t)N * keep_split;
    if (after > 0x7fffffffull) return fail(GSR_ERR_INVALID, "the new row count overflows int");
    counts[0] = (int)clone;
    counts[1] = (int)split;
    // rows the final prune removes: originals that were not split, clones, and N children per parent
    counts[2] = (int)(((uint64_t)P - split - keep_orig) + (clone - keep_clone) + (uint64_t)N * (split - keep_split));
    counts[3] = (int)after;
    return GSR_OK;
}

int gsr_densify_apply(int P, int P_after, int n_split, int N, int n_groups, const int* Ms, int xyz_group,
                      int scaling_group, int rotation_group, const float* const* src, const float* const* src_m,
                      const float* const* src_v, float* const* dst, float* const* dst_m, float* const* dst_v,
                      const float* samples, const char* workspace, gsr_stream_t stream)
{
    if (P < 0 || P_after < 0 || n_split < 0 || n_groups < 0)
        return fail(GSR_ERR_INVALID, "P, P_after, n_split and n_groups must be >= 0");
    if (N < 1) return fail(GSR_ERR_INVALID, "N must be >= 1");
    if (n_groups > DENSIFY_MAX_GROUPS) return fail(GSR_ERR_INVALID, "n_groups must be <= 8");
    if (P == 0) return GSR_OK;
    if (n_split > P) return fail(GSR_ERR_INVALID, "n_split must be <= P");
    if (!Ms || !src || !src_m || !src_v || !dst || !dst_m || !dst_v || !workspace)
        return fail(GSR_ERR_INVALID, "null pointer");
    const int roles[3] = {xyz_group, scaling_group, rotation_group};
    const int role_M[3] = {3, 3, 4};
    const char* role_err[3] = {"xyz_group outside [0, n_groups)", "scaling_group outside [0, n_groups)",
                               "rotation_group outside [0, n_groups)"};
    const char* m_err[3] = {"the xyz group must have 3 floats per row", "the scaling group must have 3 floats per row",
                            "the rotation group must have 4 floats per row"};
    for (int k = 0; k < 3; k++) {
        if (roles[k] < 0 || roles[k] >= n_groups) return fail(GSR_ERR_INVALID, role_err[k]);
        if (Ms[roles[k]] != role_M[k]) return fail(GSR_ERR_INVALID, m_err[k]);
    }
    if (n_split > 0 && !samples) return fail(GSR_ERR_INVALID, "null samples with n_split > 0");
    DensifyApplyArgs a = {};
    a.P = P; a.P_after = P_after; a.n_split = n_split; a.N = N; a.n_groups = n_groups;
    a.xyz_group = xyz_group; a.scaling_group = scaling_group; a.rotation_group = rotation_group;
    a.samples = samples;
    a.shrink = densify_split_shrink(N);
    for (int g = 0; g < n_groups; g++) {
        if (Ms[g] < 0) return fail(GSR_ERR_INVALID, "M must be >= 0");
        const bool moments = dst_m[g] || dst_v[g];
        if (Ms[g] > 0 && (!src[g] || (P_after > 0 && !dst[g]))) return fail(GSR_ERR_INVALID, "null group pointer");
        if (Ms[g] > 0 && moments && (!src_m[g] || !src_v[g] || !dst_m[g] || !dst_v[g]))
            return fail(GSR_ERR_INVALID, "null moment pointer (a group has all four or none)");
        a.M[g] = Ms[g];
        a.src[g] = src[g]; a.src_m[g] = src_m[g]; a.src_v[g] = src_v[g];
        a.dst[g] = dst[g]; a.dst_m[g] = moments ? dst_m[g] : nullptr; a.dst_v[g] = moments ? dst_v[g] : nullptr;
    }
    HIP_TRY(launch_densify_apply(a, workspace, (hipStream_t)stream));
    return GSR_OK;
}

// ---- visibility-compacted gradient exchange (compact.hip) ----
int gsr_union_rows_per_wave(void) { return UNION_ROWS_PER_WAVE; }

size_t gsr_union_workspace_size(int P) { return union_workspace_bytes(P); }

int gsr_visibility_pack(int P, const float* count, uint32_t* words, gsr_stream_t stream)
{
    if (P < 0) return fail(GSR_ERR_INVALID, "P must be >= 0");
    if (P == 0) return GSR_OK;
    if (!count || !words) return fail(GSR_ERR_INVALID, "null pointer");
    HIP_TRY(launch_visibility_pack(P, count, words, (hipStream_t)stream));
    return GSR_OK;
}

int gsr_union_plan(int P, int ranks, const uint32_t* words, int n_bounds, const int* bounds, char* workspace,
                   uint32_t* rows, uint8_t* mask, int* U, int* bound_ranks, gsr_stream_t stream)
{
    if (P < 0) return fail(GSR_ERR_INVALID, "P must be >= 0");
    if (ranks < 1) return fail(GSR_ERR_INVALID, "ranks must be >= 1");
    if (n_bounds < 0 || n_bounds > UNION_MAX_BOUNDS) return fail(GSR_ERR_INVALID, "n_bounds must be in [0, 16]");
    if (!U || (n_bounds > 0 && (!bounds || !bound_ranks))) return fail(GSR_ERR_INVALID, "null pointer");
    for (int k = 0; k < n_bounds; k++)
        if (bounds[k] < 0 || bounds[k] > P || (bounds[k] != P && bounds[k] % UNION_ROWS_PER_WAVE != 0))
            return fail(GSR_ERR_INVALID, "a boundary must be P or a multiple of gsr_union_rows_per_wave() in [0, P]");
    *U = 0;
    for (int k = 0; k < n_bounds; k++) bound_ranks[k] = 0;
    if (P == 0) return GSR_OK;
    if (!words || !workspace || !rows) return fail(GSR_ERR_INVALID, "null pointer");
    uint32_t* h;
    int rc = pinned(MAX_VIEWS, &h);  // (the two slots behind the forward's and the densify plan's)
    if (rc) return rc;
    for (int k = 0; k <= n_bounds; k++) h[k] = L_PENDING;  // (every count is <= P < 2^31)
    HIP_TRY(launch_union_plan(P, ranks, words, n_bounds, bounds, workspace, rows, mask, h, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int k = 0; k <= n_bounds; k++)
        if (__atomic_load_n(&h[k], __ATOMIC_ACQUIRE) == L_PENDING)
            return fail(GSR_ERR_HIP, "the plan did not publish its counts");
    *U = (int)h[0];
    for (int k = 0; k < n_bounds; k++) bound_ranks[k] = (int)h[1 + k];
    return GSR_OK;
}

static int rows_move(bool scatter, int P, int U, int u0, int u1, int n_groups, const int* Ms, float* const* full,
                     const uint32_t* rows, float* compact, gsr_stream_t stream)
{
    if (P < 0 || U < 0 || n_groups < 0) return fail(GSR_ERR_INVALID, "P, U and n_groups must be >= 0");
    if (U > P) return fail(GSR_ERR_INVALID, "U must be <= P");
    if (n_groups > ADAM_MAX_GROUPS) return fail(GSR_ERR_INVALID, "n_groups must be <= 8");
    if (u0 < 0 || u1 > U || u0 > u1) return fail(GSR_ERR_INVALID, "window outside [0, U]");
    if (P == 0 || U == 0 || u0 == u1 || n_groups == 0) return GSR_OK;
    if (!Ms || !full || !rows || !compact) return fail(GSR_ERR_INVALID, "null pointer");
    RowsMoveArgs a = {};
    a.P = P; a.U = U; a.u0 = u0; a.u1 = u1; a.n_groups = n_groups;
    a.rows = rows; a.compact = compact;
    for (int g = 0; g < n_groups; g++) {
        if (Ms[g] < 0) return fail(GSR_ERR_INVALID, "M must be >= 0");
        if ((size_t)U * Ms[g] >= 0xFFFFFFF0ull) return fail(GSR_ERR_INVALID, "U*M must be < 2^32 - 16");
        if (Ms[g] > 0 && !full[g]) return fail(GSR_ERR_INVALID, "null group pointer");
        a.M[g] = Ms[g];
        a.full[g] = full[g];
    }
    HIP_TRY(launch_rows_move(a, scatter, (hipStream_t)stream));
    return GSR_OK;
}

int gsr_rows_gather(int P, int U, int u0, int u1, int n_groups, const int* Ms, const float* const* src,
                    const uint32_t* rows, float* compact, gsr_stream_t stream)
{
    return rows_move(false, P, U, u0, u1, n_groups, Ms, const_cast<float* const*>(src), rows, compact, stream);
}

int gsr_rows_scatter(int P, int U, int u0, int u1, int n_groups, const int* Ms, float* const* dst,
                     const uint32_t* rows, const float* compact, gsr_stream_t stream)
{
    return rows_move(true, P, U, u0, u1, n_groups, Ms, dst, rows, const_cast<float*>(compact), stream);
}

// ---- simple_knn.h ----
size_t gsr_knn_workspace_size(int P) { return knn_workspace_bytes(P); }

int gsr_knn_dist2(int P, const float* points, float* dist2_out, void* workspace, void* stream)
{
    if (P < 0) return fail(GSR_ERR_INVALID, "P must be >= 0");
    if (P == 0) return GSR_OK;
    if (!points || !dist2_out || !workspace) return fail(GSR_ERR_INVALID, "null pointer");
    uint32_t* h;
    int rc = pinned(0, &h);
    if (rc) return rc;
    HIP_TRY(knn_dist2(P, points, dist2_out, static_cast<char*>(workspace), h + 8, (hipStream_t)stream));
    return GSR_OK;
}

int gsr_debug_sorted_keys(const char* geometry_buffer, const char* binning_buffer, const char* image_buffer, int P,
                          int num_rendered, int width, int height, uint64_t* keys_out, uint32_t* vals_out,
                          uint32_t* ranges_out, gsr_stream_t stream)
{
    hipStream_t s = (hipStream_t)stream;
    const GeomLayout g = geom_layout(P);
    const BinLayout b = bin_layout(num_rendered);
    const ImageLayout im = image_layout(width, height);
    const TileGrid tg(width, height);
    if (num_rendered > 0) {
        const uint32_t* point_list = at<uint32_t>(binning_buffer, b.off[BIN_POINT_LIST]);
        if (keys_out && use_tile_diff(tg.gx, tg.gy))  // no tile ids were written: each tile's range carries its id
            HIP_TRY(launch_debug_keys_from_ranges(tg.T, at<uint2>(image_buffer, im.off[IMG_RANGES]),
                                                  point_list, at<uint32_t>(geometry_buffer, g.off[GEOM_DKEY]),
                                                  keys_out, s));
        else if (keys_out)
            HIP_TRY(launch_debug_keys(num_rendered, at<uint32_t>(binning_buffer, b.off[BIN_SORTED_TILES]), point_list,
                                      at<uint32_t>(geometry_buffer, g.off[GEOM_DKEY]), keys_out, s));
        if (vals_out)
            HIP_TRY(hipMemcpyAsync(vals_out, point_list, 4 * (size_t)num_rendered, hipMemcpyDeviceToDevice, s));
    }
    if (ranges_out)
        HIP_TRY(hipMemcpyAsync(ranges_out, image_buffer + im.off[IMG_RANGES], 8 * (size_t)tg.T,
                               hipMemcpyDeviceToDevice, s));
    return GSR_OK;
}

int gsr_debug_depth_wide(void) { return depth_force_wide() ? 1 : 0; }

int gsr_debug_set_depth_wide(int on)
{
    set_depth_force_wide(on != 0);
    return GSR_OK;
}

size_t gsr_debug_depth_sort_workspace_size(int n)
{
    const size_t q = align_up(4 * (size_t)(n > 0 ? n : 0), 256);
    return 4 * q + align_up(radix_status_bytes(n), 256);
}

int gsr_debug_depth_sort(const uint32_t* keys, int n, uint32_t* out_ids, char* workspace, gsr_stream_t stream)
{
    if (n < 0 || (n > 0 && (!keys || !out_ids || !workspace))) return fail(GSR_ERR_INVALID, "bad depth-sort arguments");
    if (n == 0) return GSR_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t q = align_up(4 * (size_t)n, 256);
    uint32_t* k0 = reinterpret_cast<uint32_t*>(workspace);
    uint32_t* v0 = reinterpret_cast<uint32_t*>(workspace + q);
    uint32_t* k1 = reinterpret_cast<uint32_t*>(workspace + 2 * q);
    uint32_t* v1 = reinterpret_cast<uint32_t*>(workspace + 3 * q);
    // the forward's call (forward_geometry) without the rect gather
    HIP_TRY(radix_sort(n, DEPTH_BITS, keys, nullptr, k0, v0, k1, v1, out_ids, nullptr, nullptr, workspace + 4 * q, s));
    if (!depth_force_wide()) {  // three passes: the range word says whether they sufficed (else four, as the forward)
        uint32_t rw[2] = {0u, 1u};
        HIP_TRY(hipMemcpyAsync(rw, workspace + 4 * q + radix_range_offset(n), 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!rw[1]) {
            const SortJob j = {n, keys, nullptr, k0, v0, k1, v1, out_ids, nullptr, nullptr, workspace + 4 * q};
            HIP_TRY(radix_sort_batch(&j, 1, DEPTH_BITS, s, 0, SORT_DEPTH, /*four_pass=*/true));
        }
    }
    return GSR_OK;
}

}  // extern "C"
