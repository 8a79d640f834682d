// compact.hip -- the rows a data-parallel step has to exchange, and their move into and out of a
// compact buffer.  A Gaussian no view of the step saw on any rank has a zero gradient row on every
// rank, so the SUM over the ranks needs the union of the ranks' visible rows only
// (multiview.compact_allreduce).
//
// visibility_pack   one thread per Gaussian: the wave's ballot of count[g] > 0 becomes two 32-bit words
//                   (bit g & 31 of word g >> 5; bits at or beyond P are zero).  4 B in per Gaussian,
//                   1 bit out.
// union_plan        three small launches over the `ranks` gathered word rows, one wave per
//                   UNION_ROWS_PER_WAVE Gaussians (32 words), four waves per workgroup:
//   count    ORs the ranks' words (4 B x ranks in per 32 Gaussians, 4 B out) and counts the set bits of
//            the wave's 32 words;
//   offsets  ONE workgroup turns the per-wave counts into exclusive offsets and stores the total U
//            and the number of union rows below each caller-given boundary (a multiple of
//            UNION_ROWS_PER_WAVE, or P: a wave's offset) in pinned host memory;
//   rows     one thread per Gaussian (ballot + lanes below, as densify's scatter): the ascending list
//            rows[0..U) with consecutive dword stores across lanes, and optionally a byte mask (P,).
//   No float atomics, no inter-workgroup waiting: the launches are the barriers.
// rows_gather / rows_scatter   every group in ONE launch (block_start per group, as
//                   adam_update_multi_kernel), one thread per compact element of the window
//                   [u0, u1) of union rows.  The compact buffer is [group][union row][column]: group k
//                   starts at U * sum(M_j, j < k) floats.  Compact-side accesses are consecutive dwords;
//                   the other side runs along ascending rows.  Per union row and direction:
//                   4 B (the row index, shared by the row's threads) + 8 B per float = 4 + 8 sum(M).
//                   scatter writes the union rows of the window and nothing else.
#include "gsr_common.h"
#include "gsr_kernels.h"

namespace gsr {

namespace {

constexpr int UNION_HDR_WORDS = 64;
constexpr uint32_t WORDS_PER_WAVE = UNION_ROWS_PER_WAVE / 32;  // 32: one word per lane of half a wave
static_assert(WORDS_PER_WAVE == 32, "union_count_kernel reduces 32 lanes");

struct UnionWorkspace {
    uint32_t* hdr;         // [0] = U
    uint32_t* wave_count;  // per wave: count, then (offsets kernel) exclusive offset
    uint32_t* uni;         // (P + 31) / 32 words: the OR of the ranks' rows
};

__host__ __device__ inline size_t uws_align(size_t x) { return (x + 255) & ~(size_t)255; }
__host__ __device__ inline uint32_t union_waves(int P)
{
    return (uint32_t)(((size_t)P + UNION_ROWS_PER_WAVE - 1) / UNION_ROWS_PER_WAVE);
}
__host__ __device__ inline uint32_t union_words(int P) { return (uint32_t)(((size_t)P + 31) / 32); }

inline size_t union_layout(int P, size_t off[3])
{
    const size_t sizes[3] = {4 * (size_t)UNION_HDR_WORDS, 4 * (size_t)union_waves(P), 4 * (size_t)union_words(P)};
    size_t at = 0;
    for (int k = 0; k < 3; k++) {
        off[k] = at;
        at += uws_align(sizes[k]);
    }
    return at;
}
inline UnionWorkspace union_carve(char* w, int P)
{
    size_t off[3];
    union_layout(P, off);
    UnionWorkspace s;
    s.hdr = reinterpret_cast<uint32_t*>(w + off[0]);
    s.wave_count = reinterpret_cast<uint32_t*>(w + off[1]);
    s.uni = reinterpret_cast<uint32_t*>(w + off[2]);
    return s;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot)
{
    const uint32_t lane = threadIdx.x & 63;
    return (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
}

}  // namespace

// ---- pack -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) visibility_pack_kernel(int P, const float* count, uint32_t* words)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    const bool on = g < (size_t)P && count[g] > 0.f;  // (every lane reaches the ballot)
    const uint64_t b = __ballot(on);
    const size_t w = (g - lane) / 32 + lane;  // lanes 0 and 1: the wave's two words
    if (lane < 2 && w < union_words(P)) words[w] = (uint32_t)(b >> (32 * lane));
}

hipError_t launch_visibility_pack(int P, const float* count, uint32_t* words, hipStream_t s)
{
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(visibility_pack_kernel, dim3((uint32_t)(((size_t)P + 255) / 256)), dim3(256), 0, s, P, count,
                       words);
    return hipGetLastError();
}

// ---- plan -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) union_count_kernel(int P, int ranks, const uint32_t* words, uint32_t* uni,
                                                          uint32_t* wave_count)
{
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (gw >= union_waves(P)) return;  // wave-uniform
    const uint32_t nwords = union_words(P);
    const uint32_t wi = gw * WORDS_PER_WAVE + lane;
    uint32_t v = 0;
    if (lane < WORDS_PER_WAVE && wi < nwords) {
        for (int r = 0; r < ranks; r++) v |= words[(size_t)r * nwords + wi];
        // bits at or beyond P never count, whatever the caller's tail holds: U <= P
        if (wi == nwords - 1 && (P & 31)) v &= (1u << (P & 31)) - 1u;
        uni[wi] = v;
    }
    uint32_t c = (uint32_t)__popc(v);
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) c += __shfl_down(c, d);  // lanes >= 32 hold 0
    if (lane == 0) wave_count[gw] = c;
}

struct UnionBounds {
    int n;
    int b[UNION_MAX_BOUNDS];
};

// One workgroup: the per-wave counts become exclusive offsets in place; U goes to the header, U and
// the boundaries' ranks (system-scope stores) to the host's pinned words.
__global__ void __launch_bounds__(256) union_offsets_kernel(uint32_t nw, uint32_t* wave_count, uint32_t* hdr,
                                                            uint32_t* host_out, UnionBounds bounds)
{
    __shared__ uint32_t part[256];
    __shared__ uint32_t total;
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nw + 255) / 256;
    const uint32_t w0 = t * per < nw ? t * per : nw, w1 = w0 + per < nw ? w0 + per : nw;
    uint32_t sum = 0;
    for (uint32_t w = w0; w < w1; w++) sum += wave_count[w];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {  // serial over the 256 partial sums
        uint32_t run = 0;
        for (int k = 0; k < 256; k++) {
            const uint32_t v = part[k];
            part[k] = run;
            run += v;
        }
        total = run;
        hdr[0] = run;
    }
    __syncthreads();
    uint32_t run = part[t];
    for (uint32_t w = w0; w < w1; w++) {
        const uint32_t v = wave_count[w];
        wave_count[w] = run;
        run += v;
    }
    __syncthreads();  // the offsets below were written by other threads of this workgroup
    if (t == 0) __hip_atomic_store(host_out, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (t < (uint32_t)bounds.n) {
        const uint32_t w = (uint32_t)bounds.b[t] / UNION_ROWS_PER_WAVE;  // (b == P past the last full wave: U)
        const uint32_t below = w < nw && (uint32_t)bounds.b[t] % UNION_ROWS_PER_WAVE == 0 ? wave_count[w] : total;
        __hip_atomic_store(host_out + 1 + t, below, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ void __launch_bounds__(256) union_rows_kernel(int P, const uint32_t* uni, const uint32_t* wave_count,
                                                         uint32_t* rows, uint8_t* mask)
{
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (gw >= union_waves(P)) return;  // wave-uniform
    const size_t row0 = (size_t)gw * UNION_ROWS_PER_WAVE;
    uint32_t off = wave_count[gw];
    for (int it = 0; it < UNION_ROWS_PER_WAVE / 64; it++) {
        const size_t i = row0 + (size_t)it * 64 + lane;
        const bool on = i < (size_t)P && ((uni[i >> 5] >> (i & 31)) & 1u);
        const uint64_t b = __ballot(on);
        // off + lanes_below < U <= P: the counts came from the same words
        if (on) rows[off + lanes_below(b)] = (uint32_t)i;
        if (mask && i < (size_t)P) mask[i] = on ? 1 : 0;
        off += (uint32_t)__popcll(b);
    }
}

size_t union_workspace_bytes(int P)
{
    if (P <= 0) return 0;
    size_t off[3];
    return union_layout(P, off);
}

hipError_t launch_union_plan(int P, int ranks, const uint32_t* words, int n_bounds, const int* bounds,
                             char* workspace, uint32_t* rows, uint8_t* mask, uint32_t* host_out, hipStream_t s)
{
    if (P <= 0) return hipSuccess;
    if (ranks < 1 || n_bounds < 0 || n_bounds > UNION_MAX_BOUNDS) return hipErrorInvalidValue;
    const UnionWorkspace ws = union_carve(workspace, P);
    const uint32_t nw = union_waves(P), blocks = (nw + 3) / 4;
    UnionBounds b = {};
    b.n = n_bounds;
    for (int k = 0; k < n_bounds; k++) b.b[k] = bounds[k];
    hipLaunchKernelGGL(union_count_kernel, dim3(blocks), dim3(256), 0, s, P, ranks, words, ws.uni, ws.wave_count);
    hipLaunchKernelGGL(union_offsets_kernel, dim3(1), dim3(256), 0, s, nw, ws.wave_count, ws.hdr, host_out, b);
    hipLaunchKernelGGL(union_rows_kernel, dim3(blocks), dim3(256), 0, s, P, (const uint32_t*)ws.uni,
                       (const uint32_t*)ws.wave_count, rows, mask);
    return hipGetLastError();
}

// ---- gather / scatter -----------------------------------------------------------------------
struct RowsMoveKernelArgs {
    RowsMoveArgs a;
    uint32_t block_start[ADAM_MAX_GROUPS];  // first workgroup of each group
    size_t base[ADAM_MAX_GROUPS];           // first float of each group in the compact buffer
};

template <bool SCATTER>
__global__ void __launch_bounds__(256) rows_move_kernel(RowsMoveKernelArgs k)
{
    const RowsMoveArgs& a = k.a;
    int gi = 0;
#pragma unroll
    for (int g = 1; g < ADAM_MAX_GROUPS; g++)
        if (g < a.n_groups && blockIdx.x >= k.block_start[g]) gi = g;
    const uint32_t M = (uint32_t)a.M[gi];
    const size_t e64 = (size_t)(blockIdx.x - k.block_start[gi]) * 256 + threadIdx.x;
    if (e64 >= (size_t)(a.u1 - a.u0) * M) return;
    const uint32_t e = (uint32_t)e64;  // (u1 - u0) * M < 2^32 - 16: 32-bit division
    const uint32_t ul = e / M, c = e - ul * M;
    const uint32_t r = a.rows[(size_t)a.u0 + ul];
    if (r >= (uint32_t)a.P) return;  // not a row of these tensors: nothing is read or written
    const size_t ci = k.base[gi] + ((size_t)a.u0 * M + e), fi = (size_t)r * M + c;
    if (SCATTER) a.full[gi][fi] = a.compact[ci];
    else a.compact[ci] = a.full[gi][fi];
}

hipError_t launch_rows_move(const RowsMoveArgs& a, bool scatter, hipStream_t s)
{
    if (a.P <= 0 || a.U <= 0 || a.u1 <= a.u0 || a.n_groups <= 0) return hipSuccess;
    if (a.n_groups > ADAM_MAX_GROUPS || a.u0 < 0 || a.u1 > a.U || a.U > a.P) return hipErrorInvalidValue;
    RowsMoveKernelArgs k;
    k.a = a;
    size_t blocks = 0, base = 0;
    for (int g = 0; g < ADAM_MAX_GROUPS; g++) {
        k.block_start[g] = (uint32_t)blocks;
        k.base[g] = base;
        if (g >= a.n_groups) continue;
        if (a.M[g] < 0 || (size_t)a.U * a.M[g] >= 0xFFFFFFF0ull) return hipErrorInvalidValue;  // 32-bit element indices
        blocks += ((size_t)(a.u1 - a.u0) * a.M[g] + 255) / 256;
        base += (size_t)a.U * a.M[g];
        if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    }
    if (blocks == 0) return hipSuccess;
    if (scatter) hipLaunchKernelGGL(rows_move_kernel<true>, dim3((uint32_t)blocks), dim3(256), 0, s, k);
    else hipLaunchKernelGGL(rows_move_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, s, k);
    return hipGetLastError();
}

}  // namespace gsr
