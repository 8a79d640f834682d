// ssim.hip -- fused SSIM map forward/backward for gfx950: the drop-in for the reference's
// optional `fused_ssim` (submodule fused-ssim, un-vendored; call site train.py:31-35,121-124)
// and for the `fusedssim` / `fusedssim_backward` ops utils/loss_utils.py:17-38 imports from
// diff_gaussian_rasterization._C.  Semantics are those of the reference's own PyTorch SSIM
// (utils/loss_utils.py:56-86): an 11x11 Gaussian window (sigma 1.5, normalised in float32),
// zero padding ("same"), per channel, C1 = 0.01^2, C2 = 0.03^2:
//   mu = w * x, sigma_xx = w * x^2 - mu_x^2, sigma_xy = w * (x y) - mu_x mu_y,
//   map = (2 mu_x mu_y + C1)(2 sigma_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(sigma_xx + sigma_yy + C2)).
//
// Output tiles of 64x32 pixels of one (batch, channel) plane.  A persistent grid (2 workgroups
// of 256 threads per CU) walks the tiles; each tile's 74x42 halo of both images goes through
// LDS, and the NEXT tile's halo loads are issued into registers before the current tile is
// computed, so HBM latency hides behind the arithmetic.  The window is applied separably
// (horizontal pass for the five moments over the 42 halo rows, then a vertical pass with a
// rolling 4-row window in registers), two columns per thread as packed-f32 pairs: each pixel
// costs 2 x 5 x 11 / 2 packed FMAs and the kernel streams HBM once (2 images in; map + 3
// partial-derivative planes out).
// The backward applies the window to the three partial planes times dL/dmap and finishes
//   dL/dx(p) = (w * (g A))(p) + 2 x(p) (w * (g B))(p) + y(p) (w * (g C))(p)
// with A = dmap/dmu_x (through mu_x in sigma_xx and sigma_xy included), B = dmap/dsigma_xx,
// C = dmap/dsigma_xy.  No atomics: results are bitwise reproducible.
#include "gsr_common.h"
#include "gsr_kernels.h"

#include <cmath>

namespace gsr {

// Thread (p = tid & 31, q = tid >> 5) owns the column PAIR (p, p + 32) of a tile, so every tap of
// both passes is one packed v_pk_fma_f32 on (col p, col p + 32) with the tap weight broadcast;
// ds_read2_b32 brings the two columns' inputs into adjacent registers.  Horizontal-pass rows are
// dealt to the 8 thread rows q, q + 8, ...; in the vertical pass thread row q owns output rows
// 4q .. 4q + 3.
constexpr int SS_TW = 64;                 // output tile width
constexpr int SS_TH = 32;                 // output tile height
constexpr int SS_R = 5;                   // window radius (11 taps)
constexpr int SS_HH = SS_TH + 2 * SS_R;   // halo rows, 42
constexpr int SS_HW = SS_TW + 2 * SS_R;   // halo columns, 74
constexpr int SS_LS = 76;                 // LDS row stride of the staged planes (floats)
constexpr int SS_STAGE = SS_HH * SS_LS;            // staged floats per plane
constexpr int SS_STAGE_IT = (SS_STAGE + 255) / 256;  // per thread, 13
constexpr int SS_BLOCKS_PER_CU = 2;       // LDS-limited (79 KB forward, 70 KB backward)

typedef float f2 __attribute__((ext_vector_type(2)));

struct SsimWeights {
    float w[11];
};

struct SsGrid {
    int H, W, tx, ty, ntiles;
};

struct SsTile {
    size_t plane;  // offset of the tile's plane, z H W
    int x0, y0;
    int z;         // index of the tile's plane
};

// The one decoding of a tile index: tiles run along x, then y, then over the planes.
__device__ __forceinline__ SsTile ss_tile(const SsGrid& g, int t)
{
    const int x = t % g.tx, r = t / g.tx, y = r % g.ty, z = r / g.ty;
    return {(size_t)z * g.H * g.W, x * SS_TW, y * SS_TH, z};
}

__device__ __forceinline__ f2 pk_fma(float w, f2 a, f2 c) { return __builtin_elementwise_fma(f2{w, w}, a, c); }

// ---- the 11x11 window, shared by every kernel below ------------------------------------------------
// Halo registers -> LDS: put(i, j) stores this thread's element j at index i of the staged planes.
template <class Put>
__device__ __forceinline__ void ss_stage(Put put)
{
#pragma unroll
    for (int j = 0; j < SS_STAGE_IT; j++) {
        const int i = threadIdx.x + j * 256;
        if (j == SS_STAGE_IT - 1 && i >= SS_STAGE) break;
        put(i, j);
    }
}

// Horizontal pass over the five moments x, y, xx, yy, xy of the staged planes s1 (x) and s2 (y).
__device__ __forceinline__ void ss_hpass_moments(const SsimWeights& wt, const float (&s1)[SS_STAGE],
                                                 const float (&s2)[SS_STAGE], f2 (&hs)[5][SS_HH][32], int p, int q)
{
    for (int r = q; r < SS_HH; r += 8) {
        f2 mx = {0.f, 0.f}, my = mx, mxx = mx, myy = mx, mxy = mx;
        const float* r1 = s1 + r * SS_LS + p;
        const float* r2 = s2 + r * SS_LS + p;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const f2 a = {r1[k], r1[k + 32]}, b = {r2[k], r2[k + 32]};
            const float w = wt.w[k];
            mx = pk_fma(w, a, mx);
            my = pk_fma(w, b, my);
            mxx = pk_fma(w, a * a, mxx);
            myy = pk_fma(w, b * b, myy);
            mxy = pk_fma(w, a * b, mxy);
        }
        hs[0][r][p] = mx; hs[1][r][p] = my; hs[2][r][p] = mxx; hs[3][r][p] = myy; hs[4][r][p] = mxy;
    }
}

// Horizontal pass over three staged planes.
__device__ __forceinline__ void ss_hpass_planes(const SsimWeights& wt, const float (&gs)[3][SS_STAGE],
                                                f2 (&hs)[3][SS_HH][32], int p, int q)
{
    for (int r = q; r < SS_HH; r += 8) {
        f2 s[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
        for (int k = 0; k < 11; k++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float* row = gs[c] + r * SS_LS + p;
                s[c] = pk_fma(wt.w[k], f2{row[k], row[k + 32]}, s[c]);
            }
        }
        hs[0][r][p] = s[0]; hs[1][r][p] = s[1]; hs[2][r][p] = s[2];
    }
}

// Vertical pass over N planes: each of the 14 halo rows thread row q needs is read once and folded
// into all four of its outputs, out[i] = rows 4q + i of the column pair.
template <int N>
__device__ __forceinline__ void ss_vpass(const SsimWeights& wt, const f2 (&hs)[N][SS_HH][32], int p, int q,
                                         f2 (&out)[4][N])
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < N; k++) out[i][k] = f2{0.f, 0.f};
#pragma unroll
    for (int rr = 0; rr < 14; rr++) {
        f2 v[N];
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = hs[k][4 * q + rr][p];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int tap = rr - i;
            if (tap < 0 || tap > 10) continue;
#pragma unroll
            for (int k = 0; k < N; k++) out[i][k] = pk_fma(wt.w[tap], v[k], out[i][k]);
        }
    }
}

// SSIM of one pixel (column h of the pair) from its five windowed moments; with `partials` also
// d[0..2] = dmap/dmu_x (through sigma_xx and sigma_xy included), dmap/dsigma_xx, dmap/dsigma_xy.
__device__ __forceinline__ float ss_pixel(const f2 (&m)[5], int h, float C1, float C2, bool partials, float (&d)[3])
{
    const float mu1 = m[0][h], mu2 = m[1][h];
    const float s11 = m[2][h] - mu1 * mu1, s22 = m[3][h] - mu2 * mu2;
    const float s12 = m[4][h] - mu1 * mu2;
    const float A = 2.f * mu1 * mu2 + C1, B = 2.f * s12 + C2;
    const float Cc = mu1 * mu1 + mu2 * mu2 + C1, D = s11 + s22 + C2;
    const float inv = 1.f / (Cc * D);
    const float val = A * B * inv;
    if (partials) {
        // d map / d mu1 = 2 mu2 B / (C D) - 2 mu1 val / C, with 1/C = D inv, 1/D = C inv
        const float f_mu1 = 2.f * inv * (mu2 * B - mu1 * val * D);
        const float f_s11 = -val * Cc * inv;
        const float f_s12 = 2.f * A * inv;
        d[0] = f_mu1 - 2.f * mu1 * f_s11 - mu2 * f_s12;
        d[1] = f_s11;
        d[2] = f_s12;
    }
    return val;
}

// dL/dx of one pixel from the three windowed sums: (w * gA) + 2 x (w * gB) + y (w * gC).
__device__ __forceinline__ float ss_bwd_pixel(const f2 (&s)[3], int h, float x, float y)
{
    return s[0][h] + 2.f * x * s[1][h] + y * s[2][h];
}

// This thread's output pixels of the tile at (x0, y0) that lie inside the image: f(i, h, y, x) for row i
// of its four and column h of its pair.
template <class F>
__device__ __forceinline__ void ss_pixels(const SsGrid& g, int x0, int y0, int p, int q, F f)
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int y = y0 + 4 * q + i;
        if (y >= g.H) break;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int x = x0 + p + 32 * h;
            if (x >= g.W) continue;
            f(i, h, y, x);
        }
    }
}

// ... and their values in two planes, read ahead of the window (a pixel outside reads element 0, unused).
__device__ __forceinline__ void ss_load_pixels(const float* a, const float* b, const SsGrid& g, int x0, int y0, int p,
                                               int q, float (&va)[4][2], float (&vb)[4][2])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int y = y0 + 4 * q + j, x = x0 + p + 32 * h;
            const size_t o = (y < g.H && x < g.W) ? (size_t)y * g.W + x : 0;
            va[j][h] = a[o];
            vb[j][h] = b[o];
        }
    }
}

// This thread's NP-plane share of one tile's halo, held in registers between the load (issued one
// tile ahead) and the LDS store.  Elements outside the image / the 74 columns load from the plane
// origin (a valid address) and are zeroed at the store.
template <int NP>
struct SsHalo {
    float v[NP][SS_STAGE_IT];
    uint32_t outside;  // bit j: element j lies outside

    __device__ __forceinline__ void load(const float* const (&src)[NP], const SsGrid& g, const SsTile& t)
    {
        outside = 0;
#pragma unroll
        for (int j = 0; j < SS_STAGE_IT; j++) {
            const int i = threadIdx.x + j * 256;
            const int r = i / SS_LS, c = i - r * SS_LS;
            const int y = t.y0 - SS_R + r, x = t.x0 - SS_R + c;
            const bool in = i < SS_STAGE && c < SS_HW && y >= 0 && y < g.H && x >= 0 && x < g.W;
            const size_t o = t.plane + (in ? (size_t)y * g.W + x : 0);
            outside |= (in ? 0u : 1u) << j;
#pragma unroll
            for (int k = 0; k < NP; k++) v[k][j] = src[k][o];
        }
    }
    __device__ __forceinline__ float get(int k, int j) const { return (outside >> j) & 1 ? 0.f : v[k][j]; }
};

template <bool TRAIN>
__global__ void __launch_bounds__(256) ssim_fwd_kernel(SsGrid g, float C1, float C2, SsimWeights wt,
                                                       const float* img1, const float* img2, float* map, float* dA,
                                                       float* dB, float* dC)
{
    __shared__ float s1[SS_STAGE], s2[SS_STAGE];
    __shared__ f2 hs[5][SS_HH][32];  // horizontal pass per column pair: x, y, xx, yy, xy
    const int p = threadIdx.x & 31, q = threadIdx.x >> 5;
    const float* const src[2] = {img1, img2};
    int t = blockIdx.x;
    if (t >= g.ntiles) return;  // uniform over the workgroup
    SsHalo<2> halo;
    halo.load(src, g, ss_tile(g, t));
    for (; t < g.ntiles; t += gridDim.x) {
        const SsTile cur = ss_tile(g, t);
        __syncthreads();  // the previous tile is done with s1, s2 and hs
        ss_stage([&](int i, int j) {
            s1[i] = halo.get(0, j);
            s2[i] = halo.get(1, j);
        });
        if (t + (int)gridDim.x < g.ntiles) halo.load(src, g, ss_tile(g, t + gridDim.x));
        __syncthreads();
        ss_hpass_moments(wt, s1, s2, hs, p, q);
        __syncthreads();
        f2 m4[4][5];
        ss_vpass(wt, hs, p, q, m4);
        ss_pixels(g, cur.x0, cur.y0, p, q, [&](int i, int h, int y, int x) {
            float d[3];
            const float val = ss_pixel(m4[i], h, C1, C2, TRAIN, d);
            const size_t o = cur.plane + (size_t)y * g.W + x;
            map[o] = val;
            if constexpr (TRAIN) {
                dA[o] = d[0];
                dB[o] = d[1];
                dC[o] = d[2];
            }
        });
    }
}

// dL/dimg1 from dL/dmap and the forward's partial-derivative planes.
__global__ void __launch_bounds__(256) ssim_bwd_kernel(SsGrid g, SsimWeights wt, const float* img1,
                                                       const float* img2, const float* dmap, const float* dA,
                                                       const float* dB, const float* dC, float* dimg1)
{
    __shared__ float gs[3][SS_STAGE];  // g*A, g*B, g*C over the halo (zero outside)
    __shared__ f2 hs[3][SS_HH][32];
    const int p = threadIdx.x & 31, q = threadIdx.x >> 5;
    const float* const src[4] = {dmap, dA, dB, dC};
    int t = blockIdx.x;
    if (t >= g.ntiles) return;
    SsHalo<4> halo;
    halo.load(src, g, ss_tile(g, t));
    for (; t < g.ntiles; t += gridDim.x) {
        const SsTile cur = ss_tile(g, t);
        float i1[4][2], i2[4][2];  // this thread's output pixels' img1 / img2 values
        ss_load_pixels(img1 + cur.plane, img2 + cur.plane, g, cur.x0, cur.y0, p, q, i1, i2);
        __syncthreads();
        ss_stage([&](int i, int j) {
            const float gm = halo.get(0, j);
            gs[0][i] = gm * halo.v[1][j];
            gs[1][i] = gm * halo.v[2][j];
            gs[2][i] = gm * halo.v[3][j];
        });
        if (t + (int)gridDim.x < g.ntiles) halo.load(src, g, ss_tile(g, t + gridDim.x));
        __syncthreads();
        ss_hpass_planes(wt, gs, hs, p, q);
        __syncthreads();
        f2 s4[4][3];
        ss_vpass(wt, hs, p, q, s4);
        ss_pixels(g, cur.x0, cur.y0, p, q, [&](int j, int h, int y, int x) {
            dimg1[cur.plane + (size_t)y * g.W + x] = ss_bwd_pixel(s4[j], h, i1[j][h], i2[j][h]);
        });
    }
}

// ---- fused photometric loss of a batch of views (train.py:119-124) ---------------------------------
// loss[v] = (1 - lambda) mean|x - gt_v| + lambda (1 - mean SSIM(x, gt_v)), x = img or clamp(img, 0, 1).
// The forward is ssim_fwd_kernel's pass over the planes of ALL views in one launch, but instead of
// the map it reduces each tile's sum of SSIM and of |x - gt| (the centre pixels are in LDS already)
// to one pair of doubles per tile; photo_loss_reduce_kernel then adds each view's pairs in a fixed
// order.  The backward applies the window to the three partial planes alone: the upstream gradient
// of the map is the per-view constant -lambda / N * dL/dloss[v], applied after the (linear) window,
// and the L1 term and the clamp mask are finished in the same store.  Per plane-pixel the two
// kernels move 11 floats (img, gt in; 3 planes out -- 3 planes, img, gt in; dL/dimg out).

// Tile t of the loss kernels: plane z = v C + c of the contiguous (V, C, H, W) arrays, and channel c
// of view v's own ground truth.
struct PhotoTile {
    SsTile at;         // plane = the offset into the contiguous arrays
    SsTile local;      // the same tile with plane 0, for loads through img / gt below
    const float* img;  // the tile's plane of img
    const float* gt;   // the tile's plane of the view's ground truth
    int v;
};

__device__ __forceinline__ PhotoTile photo_tile(const SsGrid& g, const PhotoViews& pv, const float* img, int t)
{
    const SsTile a = ss_tile(g, t);
    const int v = a.z / pv.C, c = a.z - v * pv.C;
    return {a, {0, a.x0, a.y0, a.z}, img + a.plane, pv.gt[v] + (size_t)c * g.H * g.W, v};
}

__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// x as the loss sees it, and whether torch's clamp backward passes its gradient
__device__ __forceinline__ float clamped(int clamp, float x) { return clamp ? clamp01(x) : x; }
__device__ __forceinline__ bool clamp_passes(int clamp, float x) { return !clamp || (x >= 0.f && x <= 1.f); }

// The photometric term's gradient at a pixel the clamp passes, from the three windowed sums s:
// dloss[v] (k_ssim (w * A + 2 x w * B + gt w * C) + k_l1 sign(x - gt)).  The callers select 0 where the
// clamp is active (a select, not a product: the view loss's mask factor must not see a 0 to multiply).
__device__ __forceinline__ float photo_bwd_pixel(const f2 (&s)[3], int h, float xv, float gt, float gv, float k_ssim,
                                                 float k_l1)
{
    const float d = xv - gt;
    const float sgn = (float)((d > 0.f) - (d < 0.f));
    const float ssim = ss_bwd_pixel(s, h, xv, gt);
    return gv * (k_ssim * ssim + k_l1 * sgn);
}

// lane 0 of each wave: the sum over its 64 lanes, in a fixed order
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}

// The fixed-order sum over the workgroup's 256 threads, slot by slot of red: red_put (every thread),
// a barrier, then red_total.  The callers place the barriers, also the one that keeps a new put from
// overtaking the reads of the previous round.
template <int K>
__device__ __forceinline__ void red_put(double (&red)[4][K], int slot, double x)
{
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][slot] = x;
}

template <int K>
__device__ __forceinline__ double red_total(const double (&red)[4][K], int slot)
{
    return ((red[0][slot] + red[1][slot]) + red[2][slot]) + red[3][slot];
}

// dA null: the loss alone (no backward will follow).  Two waves per SIMD (= SS_BLOCKS_PER_CU
// workgroups per CU), as a bound: the unbounded allocator has taken 263 registers for this kernel, so that
// one workgroup fitted (246 as the code stands; the bound is what keeps a later change from costing a wave).
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
photo_loss_fwd_kernel(SsGrid g, PhotoViews pv, float C1, float C2, SsimWeights wt, int clamp, const float* img,
                      float* dA, float* dB, float* dC, double2* partial)
{
    __shared__ float s1[SS_STAGE], s2[SS_STAGE];
    __shared__ f2 hs[5][SS_HH][32];  // horizontal pass per column pair: x, y, xx, yy, xy
    __shared__ double red[4][2];
    const int p = threadIdx.x & 31, q = threadIdx.x >> 5;
    int t = blockIdx.x;
    if (t >= g.ntiles) return;  // uniform over the workgroup
    SsHalo<2> halo;
    {
        const PhotoTile n = photo_tile(g, pv, img, t);
        const float* const src[2] = {n.img, n.gt};
        halo.load(src, g, n.local);
    }
    for (; t < g.ntiles; t += gridDim.x) {
        const PhotoTile cur = photo_tile(g, pv, img, t);
        __syncthreads();  // the previous tile is done with s1, s2, hs and red
        ss_stage([&](int i, int j) {
            s1[i] = clamped(clamp, halo.get(0, j));
            s2[i] = halo.get(1, j);
        });
        if (t + (int)gridDim.x < g.ntiles) {
            const PhotoTile n = photo_tile(g, pv, img, t + gridDim.x);
            const float* const src[2] = {n.img, n.gt};
            halo.load(src, g, n.local);
        }
        __syncthreads();
        ss_hpass_moments(wt, s1, s2, hs, p, q);
        __syncthreads();
        f2 m4[4][5];
        ss_vpass(wt, hs, p, q, m4);
        // this thread's 8 pixels (float: 8 terms of at most 1; the sums over threads and tiles are double)
        float ssim8 = 0.f, l18 = 0.f;
        ss_pixels(g, cur.at.x0, cur.at.y0, p, q, [&](int i, int h, int y, int x) {
            float d[3];
            const float val = ss_pixel(m4[i], h, C1, C2, dA != nullptr, d);
            const int c = (4 * q + i + SS_R) * SS_LS + p + 32 * h + SS_R;  // the pixel itself in the halo
            ssim8 += val;
            l18 += fabsf(s1[c] - s2[c]);
            if (dA) {
                const size_t o = cur.at.plane + (size_t)y * g.W + x;
                dA[o] = d[0];
                dB[o] = d[1];
                dC[o] = d[2];
            }
        });
        red_put(red, 0, (double)ssim8);
        red_put(red, 1, (double)l18);
        __syncthreads();
        if (threadIdx.x == 0) partial[t] = double2{red_total(red, 0), red_total(red, 1)};
    }
}

// One workgroup per view: its tiles' pairs, added in an order that depends on nothing but the shape.
__global__ void __launch_bounds__(256) photo_loss_reduce_kernel(const double2* partial, int tiles_per_view,
                                                                double inv_n, double lambda, float* loss)
{
    __shared__ double red[4][2];
    const double2* pv = partial + (size_t)blockIdx.x * tiles_per_view;
    double sum_ssim = 0.0, sum_l1 = 0.0;
    for (int k = threadIdx.x; k < tiles_per_view; k += 256) {
        const double2 e = pv[k];
        sum_ssim += e.x;
        sum_l1 += e.y;
    }
    red_put(red, 0, sum_ssim);
    red_put(red, 1, sum_l1);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double ssim = red_total(red, 0) * inv_n;
        const double l1 = red_total(red, 1) * inv_n;
        loss[blockIdx.x] = (float)((1.0 - lambda) * l1 + lambda * (1.0 - ssim));
    }
}

// dL/dimg = dloss[v] (k_ssim (w * A + 2 x w * B + gt w * C) + k_l1 sign(x - gt)), k_ssim = -lambda / N,
// k_l1 = (1 - lambda) / N; zero where the clamp is active.
__global__ void __launch_bounds__(256) photo_loss_bwd_kernel(SsGrid g, PhotoViews pv, SsimWeights wt, int clamp,
                                                             float k_ssim, float k_l1, const float* img,
                                                             const float* dloss, const float* dA, const float* dB,
                                                             const float* dC, float* dimg)
{
    __shared__ float gs[3][SS_STAGE];  // A, B, C over the halo (zero outside)
    __shared__ f2 hs[3][SS_HH][32];
    const int p = threadIdx.x & 31, q = threadIdx.x >> 5;
    const float* const src[3] = {dA, dB, dC};
    int t = blockIdx.x;
    if (t >= g.ntiles) return;
    SsHalo<3> halo;
    halo.load(src, g, ss_tile(g, t));
    for (; t < g.ntiles; t += gridDim.x) {
        const PhotoTile cur = photo_tile(g, pv, img, t);
        const float gv = dloss[cur.v];
        float i1[4][2], i2[4][2];  // this thread's output pixels' img / gt values
        ss_load_pixels(cur.img, cur.gt, g, cur.at.x0, cur.at.y0, p, q, i1, i2);
        __syncthreads();
        ss_stage([&](int i, int j) {
            gs[0][i] = halo.get(0, j);
            gs[1][i] = halo.get(1, j);
            gs[2][i] = halo.get(2, j);
        });
        if (t + (int)gridDim.x < g.ntiles) halo.load(src, g, ss_tile(g, t + gridDim.x));
        __syncthreads();
        ss_hpass_planes(wt, gs, hs, p, q);
        __syncthreads();
        f2 s4[4][3];
        ss_vpass(wt, hs, p, q, s4);
        ss_pixels(g, cur.at.x0, cur.at.y0, p, q, [&](int j, int h, int y, int x) {
            const float raw = i1[j][h];
            dimg[cur.at.plane + (size_t)y * g.W + x] =
                clamp_passes(clamp, raw) ? photo_bwd_pixel(s4[j], h, clamped(clamp, raw), i2[j][h], gv, k_ssim, k_l1)
                                         : 0.f;
        });
    }
}

// ---- fused view loss: exposure, alpha mask, L1 + D-SSIM and the inverse-depth L1 term (train.py:112-141) ----
// Per view v (gsr_kernels.h ViewLossArgs):
//   e_c = sum_k raw_k E[k, c] + E[c, 3],  x_c = clamp(e_c, 0, 1) * m,  loss = photo(x, gt) + w mean|(inv - t) dm|.
// The exposure couples a pixel's three channels, so the unit of work is one 64x32 tile of a VIEW (of a
// group of up to three channels; C = 3 is one group), not of a plane: the forward holds the tile's halo
// of the three raw planes and the mask in registers (and one channel's ground truth, loaded a channel
// ahead), and the channel loop inside the workgroup stages x_c from them -- the raw planes are read once
// and no exposed image goes to memory.  Each channel is then photo_loss_fwd_kernel's window pass; the tile's (sum SSIM, sum L1)
// over its channels is one pair of doubles.  The backward walks the same tiles: per channel the window
// over the three partial planes gives dL/dx_c, g_c = m pass_c dL/dx_c, and the tile accumulates
// dL/draw_k = sum_c E[k, c] g_c in registers (one store per raw plane) and the 12 sums of dL/dE, which
// leave as 12 doubles per tile.  The inverse-depth term rides in both launches as leading tiles that
// skip the window (one double per tile forward, dL/dinv stored directly backward).  Small reduce kernels
// add each view's partials in an order that depends on the shape alone: no atomics anywhere.
struct VlTile {
    int v, c0, nc;  // the view; first channel and channel count (<= 3) of the tile's channel group
    int x0, y0;
    size_t plane0;  // offset of channel c0 of view v in the contiguous (V, C, H, W) arrays
};

__device__ __forceinline__ VlTile vl_tile(const SsGrid& g, int C, int groups, int t)
{
    const SsTile a = ss_tile(g, t);  // its planes are the channel groups
    const int v = a.z / groups, c0 = 3 * (a.z - v * groups);
    return {v, c0, C - c0 < 3 ? C - c0 : 3, a.x0, a.y0, ((size_t)v * C + c0) * g.H * g.W};
}

// Column c of a view's exposure: e_c = k[0] raw_0 + k[1] raw_1 + k[2] raw_2 + off (uniform: scalar loads).
// Without an exposure: the unit column, so that dL/draw_c = g_c below; e_c itself is then raw_c, selected.
struct VlColumn {
    float k[3], off;
};

__device__ __forceinline__ VlColumn vl_column(const float* exposure, int v, int c)
{
    if (!exposure) return {{c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f}, 0.f};
    const float* E = exposure + v * 12;
    return {{E[c], E[4 + c], E[8 + c]}, E[4 * c + 3]};
}

__device__ __forceinline__ float vl_pick(int c, float a0, float a1, float a2) { return c == 0 ? a0 : (c == 1 ? a1 : a2); }

// the same expression in both passes: the backward's clamp mask is the forward's
__device__ __forceinline__ float vl_expose(bool exposed, const VlColumn& E, int c, float r0, float r1, float r2)
{
    return exposed ? ((r0 * E.k[0] + r1 * E.k[1]) + r2 * E.k[2]) + E.off : vl_pick(c, r0, r1, r2);
}

// A plane's element at a 32-bit BYTE offset (H W < 2^30, checked by the callers): with a uniform base
// this is one load with a scalar base and one offset register, shared by every plane of the tile --
// 64-bit addresses per plane and element are what would not fit the register budget here.
__device__ __forceinline__ float vl_ld(const float* plane, uint32_t byte_off)
{
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(plane) + byte_off);
}

__device__ __forceinline__ void vl_st(float* plane, uint32_t byte_off, float x)
{
    *reinterpret_cast<float*>(reinterpret_cast<char*>(plane) + byte_off) = x;
}

// byte offset in its plane of halo element j of this thread for the tile at (x0, y0); outside the image
// or the 74 columns: 0 (a valid address) and *in = false
__device__ __forceinline__ uint32_t vl_halo_off(const SsGrid& g, int tid, int x0, int y0, int j, bool* in)
{
    const int i = tid + j * 256;
    const int r = i / SS_LS, c = i - r * SS_LS;
    const int y = y0 - SS_R + r, x = x0 - SS_R + c;
    *in = i < SS_STAGE && c < SS_HW && y >= 0 && y < g.H && x >= 0 && x < g.W;
    return *in ? 4u * ((uint32_t)y * (uint32_t)g.W + (uint32_t)x) : 0u;
}

// threadIdx.x, opaque to the optimiser: what is derived from it (13 halo rows and columns per thread) is
// recomputed per tile in a few instructions instead of living in 26 registers across the whole kernel
__device__ __forceinline__ int vl_tid()
{
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    return tid;
}

// This thread's share of one view tile's halo: the raw planes and the mask, which stay for the tile's
// channels, and the ground truth of ONE channel, reloaded per channel (one tile ahead like the rest).
struct VlHalo {
    float raw[3][SS_STAGE_IT], m[SS_STAGE_IT], gt[SS_STAGE_IT];
    uint32_t outside;  // bit j: element j lies outside

    __device__ __forceinline__ void load_view(const SsGrid& g, const ViewLossArgs& a, const float* img, const VlTile& t)
    {
        const size_t hw = (size_t)g.H * g.W;
        const float* mp = a.mask[t.v];
        const float* rp[3];
#pragma unroll
        for (int k = 0; k < 3; k++) rp[k] = img + t.plane0 + (k < t.nc ? k : 0) * hw;  // a short group re-reads
        outside = 0;
        const int tid = vl_tid();
#pragma unroll
        for (int j = 0; j < SS_STAGE_IT; j++) {
            bool in;
            const uint32_t o = vl_halo_off(g, tid, t.x0, t.y0, j, &in);
            outside |= (in ? 0u : 1u) << j;
#pragma unroll
            for (int k = 0; k < 3; k++) raw[k][j] = vl_ld(rp[k], o);
            m[j] = mp ? vl_ld(mp, o) : 1.f;
        }
    }
    __device__ __forceinline__ void load_gt(const SsGrid& g, const ViewLossArgs& a, const VlTile& t, int c)
    {
        const float* gp = a.pv.gt[t.v] + (size_t)(t.c0 + c) * g.H * g.W;
        const int tid = vl_tid();
#pragma unroll
        for (int j = 0; j < SS_STAGE_IT; j++) {
            bool in;
            gt[j] = vl_ld(gp, vl_halo_off(g, tid, t.x0, t.y0, j, &in));
        }
    }
};

// ... and of the backward's three partial planes of one channel: SsHalo<3> in vl_ld's addressing and with
// vl_tid().  Not one template: in this addressing all six kernels keep 0 scratch and 2 waves/SIMD
// (ssim_bwd_kernel 182 VGPRs for 202), but ssim_fwd_kernel / ssim_bwd_kernel ran 2.7 % / 4.9 % slower at 1080p.
struct VlHalo3 {
    float v[3][SS_STAGE_IT];
    uint32_t outside;

    __device__ __forceinline__ void load(const float* dA, const float* dB, const float* dC, const SsGrid& g, int x0,
                                         int y0)
    {
        outside = 0;
        const int tid = vl_tid();
#pragma unroll
        for (int j = 0; j < SS_STAGE_IT; j++) {
            bool in;
            const uint32_t o = vl_halo_off(g, tid, x0, y0, j, &in);
            outside |= (in ? 0u : 1u) << j;
            v[0][j] = vl_ld(dA, o);
            v[1][j] = vl_ld(dB, o);
            v[2][j] = vl_ld(dC, o);
        }
    }
    __device__ __forceinline__ float get(int k, int j) const { return (outside >> j) & 1 ? 0.f : v[k][j]; }
};

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
view_loss_fwd_kernel(SsGrid g, ViewLossArgs a, int groups, int depth_tiles, float C1, float C2, SsimWeights wt,
                     const float* img, float* dA, float* dB, float* dC, double2* partial, double* dpartial)
{
    __shared__ float s1[SS_STAGE], s2[SS_STAGE];
    __shared__ f2 hs[5][SS_HH][32];  // horizontal pass per column pair: x, y, xx, yy, xy
    __shared__ double red[4][2];
    const int p = threadIdx.x & 31, q = threadIdx.x >> 5;
    const size_t hw = (size_t)g.H * g.W;
    int t = blockIdx.x;
    // the inverse-depth tiles (tile t of view t / (tx ty)): no window, one double each
    for (; t < depth_tiles; t += gridDim.x) {
        const SsTile dt = ss_tile(g, t);  // its planes are the views
        const float* tg = a.target[dt.z];
        float d8 = 0.f;
        if (tg) {
            const float* dm = a.dmask[dt.z];
            const float* inv = a.invdepth + dt.plane;
            ss_pixels(g, dt.x0, dt.y0, p, q, [&](int, int, int y, int x) {
                const size_t o = (size_t)y * g.W + x;
                const float d = inv[o] - tg[o];
                d8 += fabsf(dm ? d * dm[o] : d);
            });
        }
        __syncthreads();  // the previous tile is done with red
        red_put(red, 0, (double)d8);
        __syncthreads();
        if (threadIdx.x == 0) dpartial[t] = red_total(red, 0);
    }
    if (t >= g.ntiles) return;  // uniform over the workgroup
    VlHalo halo;
    {
        const VlTile n = vl_tile(g, a.pv.C, groups, t - depth_tiles);
        halo.load_view(g, a, img, n);
        halo.load_gt(g, a, n, 0);
    }
    for (; t < g.ntiles; t += gridDim.x) {
        const VlTile cur = vl_tile(g, a.pv.C, groups, t - depth_tiles);
        // this thread's 8 pixels of up to 3 channels (float: 24 terms of at most 1; the sums over threads
        // and tiles are double)
        float ssim8 = 0.f, l18 = 0.f;
        for (int c = 0; c < cur.nc; c++) {  // uniform
            const VlColumn E = vl_column(a.exposure, cur.v, c);
            __syncthreads();  // the previous channel is done with s1, s2, hs and red
            ss_stage([&](int i, int j) {
                const bool out = (halo.outside >> j) & 1;
                const float e = vl_expose(a.exposure != nullptr, E, c, halo.raw[0][j], halo.raw[1][j], halo.raw[2][j]);
                s1[i] = out ? 0.f : clamped(a.clamp, e) * halo.m[j];
                s2[i] = out ? 0.f : halo.gt[j];
            });
            // the next channel's ground truth, or the next tile
            if (c + 1 < cur.nc) {
                halo.load_gt(g, a, cur, c + 1);
            } else if (t + (int)gridDim.x < g.ntiles) {
                const VlTile n = vl_tile(g, a.pv.C, groups, t + gridDim.x - depth_tiles);
                halo.load_view(g, a, img, n);
                halo.load_gt(g, a, n, 0);
            }
            __syncthreads();
            ss_hpass_moments(wt, s1, s2, hs, p, q);
            __syncthreads();
            f2 m4[4][5];
            ss_vpass(wt, hs, p, q, m4);
            // (the pixels' coordinates and offsets recomputed per channel, not kept across the window passes)
            const int et = vl_tid(), ep = et & 31, eq = et >> 5;
            ss_pixels(g, cur.x0, cur.y0, ep, eq, [&](int i, int h, int y, int x) {
                float d[3];
                const float val = ss_pixel(m4[i], h, C1, C2, dA != nullptr, d);
                const int ci = (4 * eq + i + SS_R) * SS_LS + ep + 32 * h + SS_R;  // the pixel itself in the halo
                ssim8 += val;
                l18 += fabsf(s1[ci] - s2[ci]);
                if (dA) {
                    const size_t pl = cur.plane0 + c * hw;
                    const uint32_t o = 4u * ((uint32_t)y * (uint32_t)g.W + (uint32_t)x);
                    vl_st(dA + pl, o, d[0]);
                    vl_st(dB + pl, o, d[1]);
                    vl_st(dC + pl, o, d[2]);
                }
            });
        }
        red_put(red, 0, (double)ssim8);
        red_put(red, 1, (double)l18);
        __syncthreads();
        if (threadIdx.x == 0) partial[t - depth_tiles] = double2{red_total(red, 0), red_total(red, 1)};
    }
}

// One workgroup per view: its photo tiles' pairs and its depth tiles' sums, each added in an order that
// depends on nothing but the shape.  depth_scale = depth_weight / (H W); dpartial null: no depth term.
__global__ void __launch_bounds__(256) view_loss_reduce_kernel(const double2* partial, int tiles_per_view,
                                                               const double* dpartial, int depth_tiles_per_view,
                                                               double inv_n, double lambda, double depth_scale,
                                                               float* loss)
{
    __shared__ double red[4][3];
    const double2* pv = partial + (size_t)blockIdx.x * tiles_per_view;
    double sum_ssim = 0.0, sum_l1 = 0.0, sum_d = 0.0;
    for (int k = threadIdx.x; k < tiles_per_view; k += 256) {
        const double2 e = pv[k];
        sum_ssim += e.x;
        sum_l1 += e.y;
    }
    if (dpartial)
        for (int k = threadIdx.x; k < depth_tiles_per_view; k += 256)
            sum_d += dpartial[(size_t)blockIdx.x * depth_tiles_per_view + k];
    red_put(red, 0, sum_ssim);
    red_put(red, 1, sum_l1);
    red_put(red, 2, sum_d);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double ssim = red_total(red, 0) * inv_n;
        const double l1 = red_total(red, 1) * inv_n;
        const double depth = red_total(red, 2) * depth_scale;
        loss[blockIdx.x] = (float)((1.0 - lambda) * l1 + lambda * (1.0 - ssim) + depth);
    }
}

// dL/dx_c = dloss[v] (k_ssim (w * A + 2 x w * B + gt w * C) + k_l1 sign(x - gt)) at the masked x (photo_loss_bwd_kernel's
// expression), g_c = m pass_c dL/dx_c, dL/draw_k = sum_c E[k, c] g_c; per tile the sums over its pixels of
// raw_k g_c (at 4 k + c) and g_c (at 4 c + 3) go to epartial.  Depth tiles store
// dL/dinv = dloss[v] k_depth sign((inv - t) dm) dm, zero for a view without a target.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
view_loss_bwd_kernel(SsGrid g, ViewLossArgs a, int groups, int depth_tiles, SsimWeights wt, float k_ssim, float k_l1,
                     float k_depth, const float* img, const float* dloss, const float* dA, const float* dB,
                     const float* dC, float* dimg, float* dinv, double* epartial)
{
    __shared__ float gs[3][SS_STAGE];  // A, B, C over the halo (zero outside)
    __shared__ f2 hs[3][SS_HH][32];
    __shared__ double red[4][12];
    const int p = threadIdx.x & 31, q = threadIdx.x >> 5;
    const size_t hw = (size_t)g.H * g.W;
    int t = blockIdx.x;
    for (; t < depth_tiles; t += gridDim.x) {
        const SsTile dt = ss_tile(g, t);  // its planes are the views
        const float* tg = a.target[dt.z];
        const float* dm = a.dmask[dt.z];
        const float* inv = a.invdepth + dt.plane;
        const float gv = dloss[dt.z] * k_depth;
        ss_pixels(g, dt.x0, dt.y0, p, q, [&](int, int, int y, int x) {
            const size_t o = (size_t)y * g.W + x;
            float out = 0.f;
            if (tg) {
                const float w = dm ? dm[o] : 1.f;
                const float d = (inv[o] - tg[o]) * w;
                out = gv * (float)((d > 0.f) - (d < 0.f)) * w;
            }
            dinv[dt.plane + o] = out;
        });
    }
    if (t >= g.ntiles) return;  // uniform over the workgroup
    VlHalo3 halo;
    {
        const VlTile n = vl_tile(g, a.pv.C, groups, t - depth_tiles);
        halo.load(dA + n.plane0, dB + n.plane0, dC + n.plane0, g, n.x0, n.y0);
    }
    for (; t < g.ntiles; t += gridDim.x) {
        const VlTile cur = vl_tile(g, a.pv.C, groups, t - depth_tiles);
        const float gv = dloss[cur.v];
        const float* gtv = a.pv.gt[cur.v] + (size_t)cur.c0 * hw;
        const float* mp = a.mask[cur.v];
        // this thread's output pixels: the raw channels and the mask (0 outside the image: nothing flows)
        float rw[3][4][2], mk[4][2], draw[3][4][2];
        uint32_t off[4][2];  // byte offsets in a plane; 0 outside the image
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int y = cur.y0 + 4 * q + j, x = cur.x0 + p + 32 * h;
                const bool in = y < g.H && x < g.W;
                off[j][h] = in ? 4u * ((uint32_t)y * (uint32_t)g.W + (uint32_t)x) : 0u;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    rw[k][j][h] = vl_ld(img + cur.plane0 + (k < cur.nc ? k : 0) * hw, off[j][h]);
                    draw[k][j][h] = 0.f;
                }
                mk[j][h] = in ? (mp ? vl_ld(mp, off[j][h]) : 1.f) : 0.f;
            }
        }
        for (int c = 0; c < cur.nc; c++) {  // uniform
            const VlColumn E = vl_column(a.exposure, cur.v, c);
            float gt8[4][2];
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int h = 0; h < 2; h++) gt8[j][h] = vl_ld(gtv + c * hw, off[j][h]);
            }
            __syncthreads();  // the previous channel is done with gs, hs and red
            ss_stage([&](int i, int j) {
                gs[0][i] = halo.get(0, j);
                gs[1][i] = halo.get(1, j);
                gs[2][i] = halo.get(2, j);
            });
            // the next channel's planes, or the next tile's first
            if (c + 1 < cur.nc) {
                const size_t pl = cur.plane0 + (c + 1) * hw;
                halo.load(dA + pl, dB + pl, dC + pl, g, cur.x0, cur.y0);
            } else if (t + (int)gridDim.x < g.ntiles) {
                const VlTile n = vl_tile(g, a.pv.C, groups, t + gridDim.x - depth_tiles);
                halo.load(dA + n.plane0, dB + n.plane0, dC + n.plane0, g, n.x0, n.y0);
            }
            __syncthreads();
            ss_hpass_planes(wt, gs, hs, p, q);
            __syncthreads();
            f2 s4[4][3];
            ss_vpass(wt, hs, p, q, s4);
            float es[4] ={0.f, 0.f, 0.f, 0.f};  // this thread's sums of raw_k g_c and of g_c
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const float m = mk[j][h];
                    const float e = vl_expose(a.exposure != nullptr, E, c, rw[0][j][h], rw[1][j][h], rw[2][j][h]);
                    const float gc =
                        clamp_passes(a.clamp, e)
                            ? m * photo_bwd_pixel(s4[j], h, clamped(a.clamp, e) * m, gt8[j][h], gv, k_ssim, k_l1)
                            : 0.f;
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        draw[k][j][h] += E.k[k] * gc;
                        es[k] += rw[k][j][h] * gc;
                    }
                    es[3] += gc;
                }
            }
            if (a.exposure) {  // uniform; red is read after the channel loop
#pragma unroll
                for (int k = 0; k < 4; k++) red_put(red, k < 3 ? 4 * k + c : 4 * c + 3, (double)es[k]);
            }
        }
        ss_pixels(g, cur.x0, cur.y0, p, q, [&](int j, int h, int, int) {
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (k < cur.nc) vl_st(dimg + cur.plane0 + k * hw, off[j][h], draw[k][j][h]);
        });
        if (a.exposure) {  // uniform
            __syncthreads();
            if (threadIdx.x < 12) epartial[(size_t)(t - depth_tiles) * 12 + threadIdx.x] = red_total(red, threadIdx.x);
        }
    }
}

// One workgroup per view: dL/dE[v] (3x4) from its tiles' 12 sums, in an order that depends on the shape alone.
__global__ void __launch_bounds__(256) view_loss_exposure_reduce_kernel(const double* epartial, int tiles_per_view,
                                                                        float* dexposure)
{
    __shared__ double red[4][12];
    const double* pv = epartial + (size_t)blockIdx.x * tiles_per_view * 12;
    double s[12];
#pragma unroll
    for (int n = 0; n < 12; n++) s[n] = 0.0;
    for (int k = threadIdx.x; k < tiles_per_view; k += 256) {
#pragma unroll
        for (int n = 0; n < 12; n++) s[n] += pv[(size_t)k * 12 + n];
    }
#pragma unroll
    for (int n = 0; n < 12; n++) red_put(red, n, s[n]);
    __syncthreads();
    if (threadIdx.x < 12) dexposure[blockIdx.x * 12 + threadIdx.x] = (float)red_total(red, threadIdx.x);
}

// The reference's window (utils/loss_utils.py:46-53): exp in double, stored as float32,
// normalised in float32 (gauss / gauss.sum()).
static SsimWeights ssim_weights()
{
    SsimWeights w;
    float g[11], sum = 0.f;
    for (int x = 0; x < 11; x++) {
        g[x] = (float)std::exp(-((double)(x - 5) * (double)(x - 5)) / (2.0 * 1.5 * 1.5));
    }
    for (int x = 0; x < 11; x++) sum += g[x];  // torch's float32 sum of 11 terms
    for (int x = 0; x < 11; x++) w.w[x] = g[x] / sum;
    return w;
}

// What every launch starts from: the tile grid of n0 * n1 planes of H x W and the workgroup count of
// the persistent grid.  blocks == 0 with hipSuccess: an empty problem, nothing to launch.
struct SsPlan {
    SsGrid g;
    int blocks;
};

static hipError_t ss_plan(int n0, int n1, int H, int W, SsPlan* p)
{
    p->blocks = 0;
    if (n0 <= 0 || n1 <= 0 || H <= 0 || W <= 0) return hipSuccess;
    if ((size_t)n0 * n1 > 0x7FFFFFFFu) return hipErrorInvalidValue;
    SsGrid& g = p->g;
    g.H = H;
    g.W = W;
    g.tx = (W + SS_TW - 1) / SS_TW;
    g.ty = (H + SS_TH - 1) / SS_TH;
    const long n = (long)g.tx * g.ty * (n0 * n1);
    if (n > 0x7FFFFFFF) return hipErrorInvalidValue;
    g.ntiles = (int)n;
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const long b = (long)(cus > 0 ? cus : 1) * SS_BLOCKS_PER_CU;
    p->blocks = (int)(b < n ? b : n);
    return hipSuccess;
}

// The loss kernels' SSIM constants (the map kernels take their caller's) and, for views of C H W
// elements, the factors of the loss and of its gradient.
constexpr float SS_C1 = (float)(0.01 * 0.01), SS_C2 = (float)(0.03 * 0.03);

struct LossScale {
    double inv_n, depth;  // 1 / (C H W); depth_weight / (H W)
    float k_ssim, k_l1, k_depth;
};

static LossScale loss_scale(int C, int H, int W, float lambda, float depth_weight)
{
    const double n = (double)C * H * W;
    const double depth = (double)depth_weight / ((double)H * W);
    return {1.0 / n, depth, (float)(-(double)lambda / n), (float)((1.0 - (double)lambda) / n), (float)depth};
}

hipError_t launch_ssim_fwd(int planes, int H, int W, float C1, float C2, const float* img1, const float* img2,
                           float* map, float* dA, float* dB, float* dC, hipStream_t s)
{
    SsPlan pl;
    const hipError_t e = ss_plan(planes, 1, H, W, &pl);
    if (e != hipSuccess || !pl.blocks) return e;
    const SsimWeights w = ssim_weights();
    if (dA && dB && dC)
        hipLaunchKernelGGL(ssim_fwd_kernel<true>, dim3(pl.blocks), dim3(256), 0, s, pl.g, C1, C2, w, img1, img2, map,
                           dA, dB, dC);
    else
        hipLaunchKernelGGL(ssim_fwd_kernel<false>, dim3(pl.blocks), dim3(256), 0, s, pl.g, C1, C2, w, img1, img2, map,
                           dA, dB, dC);
    return hipGetLastError();
}

hipError_t launch_ssim_bwd(int planes, int H, int W, const float* img1, const float* img2, const float* dmap,
                           const float* dA, const float* dB, const float* dC, float* dimg1, hipStream_t s)
{
    SsPlan pl;
    const hipError_t e = ss_plan(planes, 1, H, W, &pl);
    if (e != hipSuccess || !pl.blocks) return e;
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3(pl.blocks), dim3(256), 0, s, pl.g, ssim_weights(), img1, img2, dmap, dA,
                       dB, dC, dimg1);
    return hipGetLastError();
}

static size_t photo_tiles_per_view(int C, int H, int W)
{
    return (size_t)C * ((W + SS_TW - 1) / SS_TW) * ((H + SS_TH - 1) / SS_TH);
}

size_t photo_loss_workspace_bytes(int V, int C, int H, int W)
{
    if (V <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)V * photo_tiles_per_view(C, H, W) * sizeof(double2);
}

hipError_t launch_photo_loss_fwd(const PhotoViews& views, int H, int W, float lambda, bool clamp, const float* img,
                                 float* loss, float* dA, float* dB, float* dC, void* workspace, hipStream_t s)
{
    const int V = views.V, C = views.C;
    SsPlan pl;
    hipError_t e = ss_plan(V, C, H, W, &pl);
    if (e != hipSuccess || !pl.blocks) return e;
    const bool train = dA && dB && dC;
    double2* partial = static_cast<double2*>(workspace);
    hipLaunchKernelGGL(photo_loss_fwd_kernel, dim3(pl.blocks), dim3(256), 0, s, pl.g, views, SS_C1, SS_C2,
                       ssim_weights(), clamp ? 1 : 0, img, train ? dA : nullptr, dB, dC, partial);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(photo_loss_reduce_kernel, dim3(V), dim3(256), 0, s, partial, (int)photo_tiles_per_view(C, H, W),
                       loss_scale(C, H, W, lambda, 0.f).inv_n, (double)lambda, loss);
    return hipGetLastError();
}

hipError_t launch_photo_loss_bwd(const PhotoViews& views, int H, int W, float lambda, bool clamp, const float* img,
                                 const float* dloss, const float* dA, const float* dB, const float* dC, float* dimg,
                                 hipStream_t s)
{
    SsPlan pl;
    const hipError_t e = ss_plan(views.V, views.C, H, W, &pl);
    if (e != hipSuccess || !pl.blocks) return e;
    const LossScale k = loss_scale(views.C, H, W, lambda, 0.f);
    hipLaunchKernelGGL(photo_loss_bwd_kernel, dim3(pl.blocks), dim3(256), 0, s, pl.g, views, ssim_weights(),
                       clamp ? 1 : 0, k.k_ssim, k.k_l1, img, dloss, dA, dB, dC, dimg);
    return hipGetLastError();
}

// ---- fused view loss ----
// Workspace, in doubles per view and tile position (txy = tiles of one plane): the forward's (SSIM, L1)
// pair per channel group followed by the depth sums, V groups txy pairs then V txy doubles; the
// backward's 12 exposure-gradient sums (one channel group).
struct VlShape {
    int groups;      // channel groups of up to 3 per view
    size_t txy;      // tile positions of a plane
    bool depth;      // the inverse-depth term runs
};

static VlShape view_loss_shape(const ViewLossArgs& a, int H, int W)
{
    VlShape s = {(a.pv.C + 2) / 3, photo_tiles_per_view(1, H, W), false};
    if (a.invdepth && a.depth_weight > 0.f)
        for (int v = 0; v < a.pv.V; v++) s.depth = s.depth || a.target[v] != nullptr;
    return s;
}

size_t view_loss_workspace_bytes(int V, int C, int H, int W)
{
    if (V <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    const size_t fwd = 2 * (size_t)((C + 2) / 3) + 1;
    return (size_t)V * photo_tiles_per_view(1, H, W) * (fwd > 12 ? fwd : 12) * sizeof(double);
}

hipError_t launch_view_loss_fwd(const ViewLossArgs& a, int H, int W, float lambda, const float* img, float* loss,
                                float* dA, float* dB, float* dC, void* workspace, hipStream_t s)
{
    const int V = a.pv.V, C = a.pv.C;
    if (V <= 0 || C <= 0 || H <= 0 || W <= 0) return hipSuccess;
    const VlShape sh = view_loss_shape(a, H, W);
    if ((size_t)V * (sh.groups + 1) > 0x7FFFFFFFu) return hipErrorInvalidValue;
    SsPlan pl;
    hipError_t e = ss_plan(V, sh.groups + (sh.depth ? 1 : 0), H, W, &pl);
    if (e != hipSuccess) return e;
    const bool train = dA && dB && dC;
    const LossScale k = loss_scale(C, H, W, lambda, a.depth_weight);
    double2* partial = static_cast<double2*>(workspace);
    double* dpartial = static_cast<double*>(workspace) + 2 * (size_t)V * sh.groups * sh.txy;
    hipLaunchKernelGGL(view_loss_fwd_kernel, dim3(pl.blocks), dim3(256), 0, s, pl.g, a, sh.groups,
                       sh.depth ? (int)(V * sh.txy) : 0, SS_C1, SS_C2, ssim_weights(), img, train ? dA : nullptr, dB, dC,
                       partial, dpartial);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(view_loss_reduce_kernel, dim3(V), dim3(256), 0, s, partial, (int)(sh.groups * sh.txy),
                       sh.depth ? dpartial : nullptr, (int)sh.txy, k.inv_n, (double)lambda, k.depth, loss);
    return hipGetLastError();
}

hipError_t launch_view_loss_bwd(const ViewLossArgs& a, int H, int W, float lambda, const float* img,
                                const float* dloss, const float* dA, const float* dB, const float* dC, float* dimg,
                                float* dexposure, float* dinv, void* workspace, hipStream_t s)
{
    const int V = a.pv.V, C = a.pv.C;
    if (V <= 0 || C <= 0 || H <= 0 || W <= 0) return hipSuccess;
    const VlShape sh = view_loss_shape(a, H, W);
    if ((size_t)V * (sh.groups + 1) > 0x7FFFFFFFu) return hipErrorInvalidValue;
    const bool depth = sh.depth && dinv;
    if (dinv && !depth) {
        const hipError_t z = hipMemsetAsync(dinv, 0, (size_t)V * H * W * sizeof(float), s);
        if (z != hipSuccess) return z;
    }
    SsPlan pl;
    hipError_t e = ss_plan(V, sh.groups + (depth ? 1 : 0), H, W, &pl);
    if (e != hipSuccess) return e;
    const LossScale k = loss_scale(C, H, W, lambda, a.depth_weight);
    double* epartial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(view_loss_bwd_kernel, dim3(pl.blocks), dim3(256), 0, s, pl.g, a, sh.groups,
                       depth ? (int)(V * sh.txy) : 0, ssim_weights(), k.k_ssim, k.k_l1, k.k_depth, img, dloss, dA, dB, dC,
                       dimg, dinv, epartial);
    e = hipGetLastError();
    if (e != hipSuccess || !a.exposure) return e;
    hipLaunchKernelGGL(view_loss_exposure_reduce_kernel, dim3(V), dim3(256), 0, s, epartial, (int)sh.txy, dexposure);
    return hipGetLastError();
}

}  // namespace gsr
