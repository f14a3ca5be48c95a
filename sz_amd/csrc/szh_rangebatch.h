// szh_rangebatch.h -- the value range of MANY arrays of one length in one launch (szhip_minmax_batch of include/szhip.h): what k_minmax
// does for one array, with the array as the grid's second dimension and its base pointer taken from a device table.  And of many same-shape SUB-BOXES with common
// pitches (szhip_minmax_batch_view): k_minmax_batch_view, the same run per row.
// Mapping.  An array of n values is cut at the 16-byte boundaries of ITS OWN address: a head of (16 - address % 16) % 16 bytes (fewer than VW = 16 / sizeof(T)
// values: element alignment is all the contract asks, and with it a head always reaches a boundary), whole 16-byte PIECES, a tail of fewer than VW values.  Lane l of
// the array's workgroups takes the pieces l, l + lanes, ... with one 16-byte load each, SZH_RB_UNROLL of them in flight; the head and the tail are read value by
// value by lanes of the array's first workgroup.  So the arrays of one batch may lie at different offsets from a boundary and still all move 16 bytes per lane.
// The grid (szh_rangebatch_grid) is a function of n alone: ceil(n / share) workgroups per array with share = 256 lanes x SZH_RB_UNROLL pieces x VW values, at most
// SZH_RB_MAX_GRID; beyond n = SZH_RB_MAX_GRID x share a lane sweeps more than once.
// Reduction.  Ordered integers (ord_enc), as k_minmax: min and max do not depend on the order in which values meet, so the result is bit for bit that of the single
// call and no floating-point atomic is needed.  A NaN takes no part.  res[2 a] holds the COMPLEMENT of array a's smallest ordering (so that both words start from
// zero bytes and both are reduced with atomicMax), res[2 a + 1] its largest; an array without a number leaves both 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// (u64, ord_enc, wave_min_u64, wave_max_u64: szhip_kernels.h, included in front of this file by szhip.hip)

constexpr int SZH_RB_UNROLL = 4;        // pieces a lane has in flight; a workgroup is sized for 256 x 4 of them
constexpr int SZH_RB_MAX_GRID = 128;    // workgroups per array (the batch fills the chip through the grid's second dimension)

static inline int szh_rangebatch_grid(uint64_t n, int vw)
{
    const uint64_t share = (uint64_t)256 * SZH_RB_UNROLL * (uint64_t)vw;
    const uint64_t g = (n + share - 1) / share;
    return (int)(g < 1 ? 1 : g > (uint64_t)SZH_RB_MAX_GRID ? (uint64_t)SZH_RB_MAX_GRID : g);
}

// (`tid`: threadIdx.x, read in the KERNEL, whose launch bounds give the compiler its range.)
// One RUN of n contiguous values at `base`, cut at the 16-byte boundaries of its own address, folded into the lane's lmin / lmax.  GRID: the run is shared by all
// lanes of the grid's first dimension, and the first workgroup's lanes 0 .. 2 VW - 1 read the head and the tail value by value (k_minmax_batch: the run is the
// array); else by the group of `gs` lanes (a power of two, at least 2 VW) this lane belongs to (k_minmax_batch_view: the run is a row of the sub-box).
template <class T, bool GRID>
__device__ __forceinline__ void minmax_run_body(const unsigned tid, const T *base, int64_t n, int gs, u64 &lmin, u64 &lmax)
{
    constexpr int VW = 16 / (int)sizeof(T);
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)base & 15u)) & 15u) / (unsigned)sizeof(T));
    head = head < n ? head : n;
    const int64_t pieces = (n - head) / VW, tail0 = head + pieces * VW;          // (tail0 + tail == n, tail < VW)
    auto take = [&](T v) { const u64 e = ord_enc(v); const bool num = v == v; lmin = num && e < lmin ? e : lmin; lmax = num && e > lmax ? e : lmax; };
    const uint4 *__restrict__ vp = reinterpret_cast<const uint4 *>(base + head);
    const int64_t lane = GRID ? (int64_t)blockIdx.x * 256 + (int64_t)tid : (int64_t)(tid & (unsigned)(gs - 1)), lanes = GRID ? (int64_t)gridDim.x * 256 : (int64_t)gs;
    for (int64_t p0 = lane; p0 < pieces; p0 += lanes * SZH_RB_UNROLL) {
        uint4 w[SZH_RB_UNROLL];
        for (int u = 0; u < SZH_RB_UNROLL; ++u) { const int64_t p = p0 + (int64_t)u * lanes; if (p < pieces) w[u] = vp[p]; }
        for (int u = 0; u < SZH_RB_UNROLL; ++u) {
            if (p0 + (int64_t)u * lanes >= pieces) break;
            T v[VW];
            __builtin_memcpy(v, &w[u], 16);
            for (int q = 0; q < VW; ++q) take(v[q]);
        }
    }
    if (!GRID || blockIdx.x == 0) {                                 // the head: lanes 0 .. head - 1; the tail: lanes VW .. VW + tail - 1
        const int64_t t = GRID ? (int64_t)tid : lane;
        if (t < head) take(base[t]);
        else if (t >= VW && t - VW < n - tail0) take(base[tail0 + t - VW]);
    }
}
// the workgroup's 256 lmin / lmax into array blockIdx.y's pair of `res`
__device__ __forceinline__ void minmax_reduce_body(const unsigned tid, u64 lmin, u64 lmax, u64 *red, u64 *res)
{
    lmin = wave_min_u64(lmin); lmax = wave_max_u64(lmax);
    if ((tid & 63) == 0) { red[tid >> 6] = lmin; red[4 + (tid >> 6)] = lmax; }
    __syncthreads();
    if (tid == 0) {
        u64 mn = red[0], mx = red[4];
        for (int w = 1; w < 4; ++w) { mn = red[w] < mn ? red[w] : mn; mx = red[4 + w] > mx ? red[4 + w] : mx; }
        atomicMax(&res[2 * (size_t)blockIdx.y], ~mn); atomicMax(&res[2 * (size_t)blockIdx.y + 1], mx);
    }
}
// (k_minmax_batch keeps its own text, to the letter: as a wrapper of minmax_run_body / minmax_reduce_body it compiled to another schedule and register allocation --
//  the address of the first piece was no longer formed ahead of the loop --, and it is on the path of every range-based batch call; as k_ompb_col repeats k_omp_col's)
template <class T>
__global__ __launch_bounds__(256) void k_minmax_batch(const T *const *__restrict__ bases, int64_t n, u64 *res)
{
    constexpr int VW = 16 / (int)sizeof(T);
    __shared__ u64 red[8];
    const T *__restrict__ base = bases[blockIdx.y];
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)base & 15u)) & 15u) / (unsigned)sizeof(T));
    head = head < n ? head : n;
    const int64_t pieces = (n - head) / VW, tail0 = head + pieces * VW;          // (tail0 + tail == n, tail < VW)
    u64 lmin = ~0ull, lmax = 0ull;
    auto take = [&](T v) { const u64 e = ord_enc(v); const bool num = v == v; lmin = num && e < lmin ? e : lmin; lmax = num && e > lmax ? e : lmax; };
    const uint4 *__restrict__ vp = reinterpret_cast<const uint4 *>(base + head);
    const int64_t lane = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x, lanes = (int64_t)gridDim.x * 256;
    for (int64_t p0 = lane; p0 < pieces; p0 += lanes * SZH_RB_UNROLL) {
        uint4 w[SZH_RB_UNROLL];
        for (int u = 0; u < SZH_RB_UNROLL; ++u) { const int64_t p = p0 + (int64_t)u * lanes; if (p < pieces) w[u] = vp[p]; }
        for (int u = 0; u < SZH_RB_UNROLL; ++u) {
            if (p0 + (int64_t)u * lanes >= pieces) break;
            T v[VW];
            __builtin_memcpy(v, &w[u], 16);
            for (int q = 0; q < VW; ++q) take(v[q]);
        }
    }
    if (blockIdx.x == 0) {                                          // the head: lanes 0 .. head - 1; the tail: lanes VW .. VW + tail - 1
        const int64_t t = (int64_t)threadIdx.x;
        if (t < head) take(base[t]);
        else if (t >= VW && t - VW < n - tail0) take(base[tail0 + t - VW]);
    }
    lmin = wave_min_u64(lmin); lmax = wave_max_u64(lmax);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = lmin; red[4 + (threadIdx.x >> 6)] = lmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 mn = red[0], mx = red[4];
        for (int w = 1; w < 4; ++w) { mn = red[w] < mn ? red[w] : mn; mx = red[4 + w] > mx ? red[4 + w] : mx; }
        atomicMax(&res[2 * (size_t)blockIdx.y], ~mn); atomicMax(&res[2 * (size_t)blockIdx.y + 1], mx);
    }
}

// ... of arrays of DIFFERENT lengths (szhip_minmax_batch_lens): array a has lens[a] values.  The grid's first dimension is sized to the longest array; a workgroup
// beyond the pieces of its own array returns (its lanes would find no piece: they go round the grid from blockIdx.x * 256; the first workgroup, which also reads the
// head and the tail, always stays).  The run and the reduction are the bodies above; min and max do not depend on the order: bit for bit k_minmax_batch per array.
template <class T>
__global__ __launch_bounds__(256) void k_minmax_batch_lens(const T *const *__restrict__ bases, const int64_t *__restrict__ lens, u64 *res)
{
    constexpr int VW = 16 / (int)sizeof(T);
    __shared__ u64 red[8];
    const int64_t n = lens[blockIdx.y];
    if (blockIdx.x > 0 && (int64_t)blockIdx.x * 256 >= n / VW) return;          // (uniform; pieces <= n / VW)
    u64 lmin = ~0ull, lmax = 0ull;
    minmax_run_body<T, true>(threadIdx.x, bases[blockIdx.y], n, 0, lmin, lmax);
    minmax_reduce_body(threadIdx.x, lmin, lmax, red, res);
}

// ... of MANY SUB-BOXES of e0 x e1 x e2 values with the common element pitches p0 / p1 (szhip_minmax_batch_view), each at its own base: every ROW is a run, cut at
// its own 16-byte boundaries.  The workgroup's lanes form groups of `gs` lanes (a power of two, 2 VW .. 256: the host sizes it to the pieces of a row); group q of
// the sub-box's workgroups takes the rows q, q + groups, ...  Min and max do not depend on the order: bit for bit k_minmax_batch on the contiguous copy.
template <class T>
__global__ __launch_bounds__(256) void k_minmax_batch_view(const T *const *__restrict__ bases, int64_t p0, int64_t p1, int64_t rows, int e1, int e2, int gs, u64 *res)
{
    __shared__ u64 red[8];
    const T *__restrict__ base = bases[blockIdx.y];
    u64 lmin = ~0ull, lmax = 0ull;
    const int64_t per_wg = 256 / gs, groups = (int64_t)gridDim.x * per_wg;
    for (int64_t row = (int64_t)blockIdx.x * per_wg + (int64_t)threadIdx.x / gs; row < rows; row += groups) {
        const int64_t k = row / e1, i = row - k * e1;
        minmax_run_body<T, false>(threadIdx.x, base + k * p0 + i * p1, (int64_t)e2, gs, lmin, lmax);
    }
    minmax_reduce_body(threadIdx.x, lmin, lmax, red, res);
}
