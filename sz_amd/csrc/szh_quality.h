// szh_quality.h -- an array against its decoded copy, where both lie (szhip_compare / szhip_compare_view of include/szhip.h): the reference's `sz -a` report
// (example/sz.c:549-620 float, :735-805 double) as ONE read of the two arrays with all its reductions, plus the bound checks a caller makes next.
//   k_quality_pass1   range of `ori`, largest error and where, largest point-wise relative error, the counts of excluded / changed / out-of-bound points, the first
//                     point out of bounds, the sums of ori, dec, dec^2, err^2
//   k_quality_pass2   (SZHIP_Q_CORR) the centred sums of sz.c:595-597 around the two means of pass 1 -- a second read: the one-pass form sum(xy) - n m1 m2 cancels
//                     on a field whose mean dwarfs its spread
//   k_quality_final   the workgroups' partial results, in index order, into one
// Mapping.  The box's points are numbered row-major, 0 .. n - 1, whatever the pitches; consecutive runs of VW = 16 / sizeof(T) numbers are PIECES.  Lane l of the
// grid takes the pieces l, l + lanes, l + 2 lanes, ... and folds their points in increasing number into its own partial result; the 256 partials of a workgroup
// are merged by a fixed tree in LDS and written to the workgroup's slot; k_quality_final merges the slots (lane t: slots t, t + 256, ..., then the same tree).  The
// grid is a function of n alone (szh_quality_grid).  So WHICH values meet in which order depends on n only -- not on the addresses, not on the pitches, not on
// the machine: two calls give the same bits, and a view gives the bits of its contiguous copy.  How a piece is LOADED is free: one 16-byte load where the piece
// lies in one row and starts on a 16-byte boundary (decided per array: the two may be aligned differently), value by value otherwise -- element alignment is all
// the contract asks (szhip.h).  A contiguous array whose address misses the 16-byte boundary is therefore read value by value throughout (consecutive lanes still
// cover consecutive 16 bytes, so the lines are fetched once).
// A slot is SZH_Q_WORDS u64: orderings and counts as integers, the sums as the bits of doubles.  No floating-point atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "szh_store.h"
// (ord_enc: szhip_kernels.h, included in front of this file by szhip.hip)

enum { SZH_Q_OMIN = 0, SZH_Q_OMAX, SZH_Q_EKEY, SZH_Q_EIDX, SZH_Q_PW, SZH_Q_FIRST, SZH_Q_NEX, SZH_Q_NEXD, SZH_Q_NZC, SZH_Q_NOA, SZH_Q_NOP, SZH_Q_NOB,
       SZH_Q_S0, SZH_Q_S1, SZH_Q_S2, SZH_Q_S3, SZH_Q_WORDS };
constexpr int SZH_Q_SHARE = 8;          // pieces per lane that one workgroup is sized for
constexpr int SZH_Q_MAX_GRID = 1024;    // 4 workgroups of 256 on each of 256 CUs: all resident at once (a workgroup's merge tree takes 32 KB of LDS)
constexpr int SZH_Q_UNROLL = 4;         // pieces a lane has in flight

// the launch grid: a function of the point count alone (and of the element size, through VW)
static inline int szh_quality_grid(uint64_t n, int vw)
{
    const uint64_t share = (uint64_t)256 * (uint64_t)vw * SZH_Q_SHARE;
    const uint64_t g = (n + share - 1) / share;
    return (int)(g < 1 ? 1 : g > (uint64_t)SZH_Q_MAX_GRID ? (uint64_t)SZH_Q_MAX_GRID : g);
}

// a box of r0 x r1 x r2 points (n of them) in an array whose planes lie pitch0 and whose rows pitch1 elements apart
struct szh_qview { int64_t r1, r2, pitch0, pitch1; int contiguous; };

__device__ __forceinline__ unsigned long long szh_q_dbits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ double szh_q_dval(unsigned long long u) { return __longlong_as_double((long long)u); }

__device__ __forceinline__ float szh_q_abs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double szh_q_abs(double v) { return __builtin_fabs(v); }

// the neutral partial result
__device__ __forceinline__ void szh_q_neutral(unsigned long long (&a)[SZH_Q_WORDS])
{
    for (int q = 0; q < SZH_Q_WORDS; ++q) a[q] = 0;
    a[SZH_Q_OMIN] = ~0ull; a[SZH_Q_EIDX] = ~0ull; a[SZH_Q_FIRST] = ~0ull;
}
// a <- a (+) b, `a` being the part that covers the smaller lane / slot numbers: sums are added in that order
__device__ __forceinline__ void szh_q_merge(unsigned long long (&a)[SZH_Q_WORDS], const unsigned long long (&b)[SZH_Q_WORDS])
{
    a[SZH_Q_OMIN] = b[SZH_Q_OMIN] < a[SZH_Q_OMIN] ? b[SZH_Q_OMIN] : a[SZH_Q_OMIN];
    a[SZH_Q_OMAX] = b[SZH_Q_OMAX] > a[SZH_Q_OMAX] ? b[SZH_Q_OMAX] : a[SZH_Q_OMAX];
    if (b[SZH_Q_EKEY] > a[SZH_Q_EKEY] || (b[SZH_Q_EKEY] == a[SZH_Q_EKEY] && b[SZH_Q_EIDX] < a[SZH_Q_EIDX])) { a[SZH_Q_EKEY] = b[SZH_Q_EKEY]; a[SZH_Q_EIDX] = b[SZH_Q_EIDX]; }
    a[SZH_Q_PW] = b[SZH_Q_PW] > a[SZH_Q_PW] ? b[SZH_Q_PW] : a[SZH_Q_PW];
    a[SZH_Q_FIRST] = b[SZH_Q_FIRST] < a[SZH_Q_FIRST] ? b[SZH_Q_FIRST] : a[SZH_Q_FIRST];
    for (int q = SZH_Q_NEX; q <= SZH_Q_NOB; ++q) a[q] += b[q];
    for (int q = SZH_Q_S0; q <= SZH_Q_S3; ++q) a[q] = szh_q_dbits(szh_q_dval(a[q]) + szh_q_dval(b[q]));
}

// the workgroup's 256 partial results into one (a fixed tree: lane t takes lane t + s for s = 128, 64, ..., 1), written to `slot` by lane 0
__device__ __forceinline__ void szh_q_block_merge(unsigned long long (&a)[SZH_Q_WORDS], unsigned long long *slot)
{
    __shared__ unsigned long long sh[SZH_Q_WORDS * 256];
    const int t = (int)threadIdx.x;
    for (int q = 0; q < SZH_Q_WORDS; ++q) sh[q * 256 + t] = a[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            unsigned long long b[SZH_Q_WORDS];
            for (int q = 0; q < SZH_Q_WORDS; ++q) b[q] = sh[q * 256 + t + s];
            szh_q_merge(a, b);
            for (int q = 0; q < SZH_Q_WORDS; ++q) sh[q * 256 + t] = a[q];
        }
        __syncthreads();
    }
    if (t == 0) for (int q = 0; q < SZH_Q_WORDS; ++q) slot[q] = a[q];
}

// the `cnt` points from number i0 on (a piece, or the array's last, shorter one) into v[]
template <class T>
__device__ __forceinline__ void szh_q_load(const T *__restrict__ base, const szh_qview &V, int64_t i0, int cnt, T (&v)[16 / sizeof(T)])
{
    constexpr int VW = 16 / (int)sizeof(T);
    if (V.contiguous) {
        const T *p = base + i0;
        if (cnt == VW && ((uintptr_t)p & 15u) == 0) { const uint4 w = *reinterpret_cast<const uint4 *>(p); __builtin_memcpy(v, &w, 16); }
        else for (int q = 0; q < cnt; ++q) v[q] = p[q];
        return;
    }
    const int64_t row = i0 / V.r2;
    int64_t j = i0 - row * V.r2, k = row / V.r1, i = row - k * V.r1;
    const T *p = base + k * V.pitch0 + i * V.pitch1 + j;
    if (cnt == VW && j + VW <= V.r2 && ((uintptr_t)p & 15u) == 0) { const uint4 w = *reinterpret_cast<const uint4 *>(p); __builtin_memcpy(v, &w, 16); return; }
    for (int q = 0; q < cnt; ++q) {                                 // (a piece that crosses the end of a row, or a row that starts off the 16-byte boundaries)
        v[q] = *p;
        ++p;
        if (++j == V.r2) { j = 0; if (++i == V.r1) { i = 0; ++k; } p = base + k * V.pitch0 + i * V.pitch1; }      // (computed, not read, behind the last point)
    }
}

// every point of the lane's pieces, in increasing number: f(ori, dec, number).  SZH_Q_UNROLL pieces of both arrays are loaded before the first is folded.
template <class T, class F>
__device__ __forceinline__ void szh_q_sweep(const T *__restrict__ ori, const szh_qview &VO, const T *__restrict__ dec, const szh_qview &VD, int64_t n, F &&f)
{
    constexpr int VW = 16 / (int)sizeof(T);
    const int64_t lane = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x, lanes = (int64_t)gridDim.x * 256;
    const int64_t pieces = (n + VW - 1) / VW;
    for (int64_t p0 = lane; p0 < pieces; p0 += lanes * SZH_Q_UNROLL) {
        T o[SZH_Q_UNROLL][VW], d[SZH_Q_UNROLL][VW]; int cnt[SZH_Q_UNROLL];
        for (int u = 0; u < SZH_Q_UNROLL; ++u) {
            const int64_t p = p0 + (int64_t)u * lanes, i0 = p * VW;
            cnt[u] = p < pieces ? (int)(n - i0 < VW ? n - i0 : VW) : 0;
            if (cnt[u]) { szh_q_load<T>(ori, VO, i0, cnt[u], o[u]); szh_q_load<T>(dec, VD, i0, cnt[u], d[u]); }
        }
        for (int u = 0; u < SZH_Q_UNROLL; ++u) {
            const int64_t i0 = (p0 + (int64_t)u * lanes) * VW;
            for (int q = 0; q < VW; ++q) if (q < cnt[u]) f(o[u][q], d[u][q], (unsigned long long)(i0 + q));
        }
    }
}

// A point whose ori, dec or error is a NaN is EXCLUDED: counted, and counted again when the two bit patterns differ, and takes part in nothing else.  (inf against
// the same inf: the difference is a NaN.)  abs_bound / pw_rel_bound < 0: not asked, the counts stay 0.
template <class T>
__device__ __forceinline__ void szh_q_pass1_body(const T *__restrict__ ori, const szh_qview &VO, const T *__restrict__ dec, const szh_qview &VD, int64_t n,
                                                 double abs_bound, double pw_rel_bound, unsigned long long *slot)
{
    unsigned long long omin = ~0ull, omax = 0, ekey = 0, eidx = ~0ull, first = ~0ull, n_ex = 0, n_exd = 0, n_zc = 0, n_oa = 0, n_op = 0, n_ob = 0;
    double pw = 0, s_o = 0, s_d = 0, s_dd = 0, s_ee = 0;
    const bool ask_abs = abs_bound >= 0, ask_pwr = pw_rel_bound >= 0;
    szh_q_sweep<T>(ori, VO, dec, VD, n, [&](T o, T d, unsigned long long idx) {
        const T e = szh_q_abs(d - o);                               // |dec - ori| in T, as `float err = fabs(data[i] - ori_data[i])` (sz.c:582)
        if (o != o || d != d || e != e) { ++n_ex; n_exd += szh_bits_of<T>(o) != szh_bits_of<T>(d) ? 1 : 0; return; }
        const double od = (double)o, dd = (double)d, ed = (double)e;
        const unsigned long long oe = ord_enc(o);
        omin = oe < omin ? oe : omin; omax = oe > omax ? oe : omax;
        const unsigned long long key = szh_q_dbits(ed) + 1;         // e >= +0 or +inf: its bits order as it does; 0 stays "no point yet"
        if (key > ekey) { ekey = key; eidx = idx; }                 // (the lane's numbers increase: of equal errors the first stays)
        bool over_abs = ask_abs && ed > abs_bound, over_pwr = false;
        if (o != 0) {
            const double rel = ed / szh_q_abs(od);                  // sz.c:585 (inf / inf: a NaN, which is greater than nothing, there as here)
            if (rel > pw) pw = rel;
            over_pwr = ask_pwr && rel > pw_rel_bound;
        } else if (d != 0) ++n_zc;
        n_oa += over_abs ? 1 : 0; n_op += over_pwr ? 1 : 0; n_ob += over_abs && over_pwr ? 1 : 0;
        if ((over_abs || over_pwr) && idx < first) first = idx;
        s_o += od; s_d += dd; s_dd += dd * dd; s_ee += ed * ed;
    });
    unsigned long long a[SZH_Q_WORDS];
    a[SZH_Q_OMIN] = omin; a[SZH_Q_OMAX] = omax; a[SZH_Q_EKEY] = ekey; a[SZH_Q_EIDX] = eidx; a[SZH_Q_PW] = szh_q_dbits(pw); a[SZH_Q_FIRST] = first;
    a[SZH_Q_NEX] = n_ex; a[SZH_Q_NEXD] = n_exd; a[SZH_Q_NZC] = n_zc; a[SZH_Q_NOA] = n_oa; a[SZH_Q_NOP] = n_op; a[SZH_Q_NOB] = n_ob;
    a[SZH_Q_S0] = szh_q_dbits(s_o); a[SZH_Q_S1] = szh_q_dbits(s_d); a[SZH_Q_S2] = szh_q_dbits(s_dd); a[SZH_Q_S3] = szh_q_dbits(s_ee);
    szh_q_block_merge(a, slot);
}
template <class T>
__global__ __launch_bounds__(256) void k_quality_pass1(const T *__restrict__ ori, szh_qview VO, const T *__restrict__ dec, szh_qview VD, int64_t n,
                                                       double abs_bound, double pw_rel_bound, unsigned long long *slots)
{
    szh_q_pass1_body<T>(ori, VO, dec, VD, n, abs_bound, pw_rel_bound, slots + (size_t)blockIdx.x * SZH_Q_WORDS);
}

// sz.c:595-597 around the means of pass 1, over the points pass 1 took: S0 = sum (ori - m1)(dec - m2), S1 = sum (ori - m1)^2, S2 = sum (dec - m2)^2
template <class T>
__global__ __launch_bounds__(256) void k_quality_pass2(const T *__restrict__ ori, szh_qview VO, const T *__restrict__ dec, szh_qview VD, int64_t n,
                                                       double mean_ori, double mean_dec, unsigned long long *slots)
{
    double s_od = 0, s_oo = 0, s_dd = 0;
    szh_q_sweep<T>(ori, VO, dec, VD, n, [&](T o, T d, unsigned long long) {
        const T diff = d - o;
        if (o != o || d != d || diff != diff) return;
        const double a = (double)o - mean_ori, b = (double)d - mean_dec;
        s_od += a * b; s_oo += a * a; s_dd += b * b;
    });
    unsigned long long a[SZH_Q_WORDS];
    szh_q_neutral(a);
    a[SZH_Q_S0] = szh_q_dbits(s_od); a[SZH_Q_S1] = szh_q_dbits(s_oo); a[SZH_Q_S2] = szh_q_dbits(s_dd);
    szh_q_block_merge(a, slots + (size_t)blockIdx.x * SZH_Q_WORDS);
}

// one workgroup: the slots of `nslots` workgroups, in index order, into `out`
__device__ __forceinline__ void szh_q_final_body(const unsigned long long *__restrict__ slots, int nslots, unsigned long long *out)
{
    unsigned long long a[SZH_Q_WORDS];
    szh_q_neutral(a);
    for (int s = (int)threadIdx.x; s < nslots; s += 256) {
        unsigned long long b[SZH_Q_WORDS];
        for (int q = 0; q < SZH_Q_WORDS; ++q) b[q] = slots[(size_t)s * SZH_Q_WORDS + q];
        szh_q_merge(a, b);
    }
    szh_q_block_merge(a, out);
}
__global__ __launch_bounds__(256) void k_quality_final(const unsigned long long *__restrict__ slots, int nslots, unsigned long long *out)
{
    szh_q_final_body(slots, nslots, out);
}

// ---- MANY PAIRS of one length in one launch (szhip_compare_batch): the bodies above with the pair as the grid's second dimension.  A pair's
// workgroups are blockIdx.x = 0 .. szh_quality_grid(n) - 1 as in the single call and write the pair's own run of slots, which k_quality_final_batch merges with one
// workgroup per pair -- the same values meet in the same order, so a pair's record is bit for bit the single call's.  Contiguous arrays only.
struct szh_qpair { const void *ori, *dec; double abs_bound, pw_rel_bound, mean_ori, mean_dec; };

template <class T>
__global__ __launch_bounds__(256) void k_quality_pass1_batch(const szh_qpair *__restrict__ pairs, int64_t n, unsigned long long *slots)
{
    const szh_qpair P = pairs[blockIdx.y];
    const szh_qview V = {1, n, n, n, 1};
    szh_q_pass1_body<T>((const T *)P.ori, V, (const T *)P.dec, V, n, P.abs_bound, P.pw_rel_bound, slots + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * SZH_Q_WORDS);
}
// (k_quality_pass2's text, repeated: as a wrapper of a shared body the single-call kernel compiled to 110 VGPRs instead of the 112 it had, and its registers are
// pinned -- profiles/r17_quality_batch_kernel_resources.txt; as k_ompb_col repeats k_omp_col's)
template <class T>
__global__ __launch_bounds__(256) void k_quality_pass2_batch(const szh_qpair *__restrict__ pairs, int64_t n, unsigned long long *slots)
{
    const szh_qpair P = pairs[blockIdx.y];
    const szh_qview V = {1, n, n, n, 1};
    const double mean_ori = P.mean_ori, mean_dec = P.mean_dec;
    double s_od = 0, s_oo = 0, s_dd = 0;
    szh_q_sweep<T>((const T *)P.ori, V, (const T *)P.dec, V, n, [&](T o, T d, unsigned long long) {
        const T diff = d - o;
        if (o != o || d != d || diff != diff) return;
        const double a = (double)o - mean_ori, b = (double)d - mean_dec;
        s_od += a * b; s_oo += a * a; s_dd += b * b;
    });
    unsigned long long a[SZH_Q_WORDS];
    szh_q_neutral(a);
    a[SZH_Q_S0] = szh_q_dbits(s_od); a[SZH_Q_S1] = szh_q_dbits(s_oo); a[SZH_Q_S2] = szh_q_dbits(s_dd);
    szh_q_block_merge(a, slots + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * SZH_Q_WORDS);
}
// one workgroup per pair: the pair's `nslots` slots into its record of SZH_Q_WORDS words
__global__ __launch_bounds__(256) void k_quality_final_batch(const unsigned long long *__restrict__ slots, int nslots, unsigned long long *out)
{
    szh_q_final_body(slots + (size_t)blockIdx.y * (size_t)nslots * SZH_Q_WORDS, nslots, out + (size_t)blockIdx.y * SZH_Q_WORDS);
}

// ... of pairs that are VIEWS (szhip_compare_batch_view): every `ori` a box of the view VO, every `dec` a box of the view VD -- the extents and the two pairs of
// pitches are common to the batch, the base pointers per pair.  Siblings of the two kernels above, which keep their code; the points meet in the order the point
// count gives, so a pair's record is bit for bit szhip_compare_view's, which is that of the contiguous copies.
template <class T>
__global__ __launch_bounds__(256) void k_quality_pass1_batch_view(const szh_qpair *__restrict__ pairs, szh_qview VO, szh_qview VD, int64_t n, unsigned long long *slots)
{
    const szh_qpair P = pairs[blockIdx.y];
    szh_q_pass1_body<T>((const T *)P.ori, VO, (const T *)P.dec, VD, n, P.abs_bound, P.pw_rel_bound, slots + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * SZH_Q_WORDS);
}
// (k_quality_pass2's text once more, as k_quality_pass2_batch has it and for its reason)
template <class T>
__global__ __launch_bounds__(256) void k_quality_pass2_batch_view(const szh_qpair *__restrict__ pairs, szh_qview VO, szh_qview VD, int64_t n, unsigned long long *slots)
{
    const szh_qpair P = pairs[blockIdx.y];
    const double mean_ori = P.mean_ori, mean_dec = P.mean_dec;
    double s_od = 0, s_oo = 0, s_dd = 0;
    szh_q_sweep<T>((const T *)P.ori, VO, (const T *)P.dec, VD, n, [&](T o, T d, unsigned long long) {
        const T diff = d - o;
        if (o != o || d != d || diff != diff) return;
        const double a = (double)o - mean_ori, b = (double)d - mean_dec;
        s_od += a * b; s_oo += a * a; s_dd += b * b;
    });
    unsigned long long a[SZH_Q_WORDS];
    szh_q_neutral(a);
    a[SZH_Q_S0] = szh_q_dbits(s_od); a[SZH_Q_S1] = szh_q_dbits(s_oo); a[SZH_Q_S2] = szh_q_dbits(s_dd);
    szh_q_block_merge(a, slots + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * SZH_Q_WORDS);
}
