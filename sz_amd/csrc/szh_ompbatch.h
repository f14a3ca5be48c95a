// szh_ompbatch.h -- the OpenMP container (szh_omp.h, szh_ompcol.h) over the boxes of MANY same-shape arrays in one launch
// (szhip_compress_omp_batch / szhip_decompress_omp_batch, include/szhip.h).
// Every kernel of the container is indexed by box number and its boxes are independent, so a batch is the same kernels with the array as the grid's second
// dimension: blockIdx.x counts what it counts in the single call (boxes, pairs of boxes, groups of boxes), blockIdx.y picks the array.  What differs from array to
// array -- base pointer, bound, interval count, code table, the places of its tables and of its stream -- is ONE record per array in a device table; a workgroup
// reads its record once through list[blockIdx.y] (the record is uniform per workgroup: plain loads through a const __restrict__ pointer, scalar on the GPU) and runs
// the `*_body` function the single call's kernel runs, with the record's values where that kernel has its arguments.  Nothing of a body is repeated here.
// `list`: the arrays a launch covers (all batched ones; those of one sweep form; those with verbatim values), so that one table serves every launch of the call.
// The batched VIEW calls run the same kernels with one of two geometries -- the parents' pitches for the items that are addressed where they
// lie, the contiguous one for the items that were gathered into a copy -- and keep the two kinds in different lists; k_ompb_sample_view, k_ompb_crop and
// k_ompb_view_scatter (below) are theirs alone.
#pragma once

struct szh_ompb_rec {
    const void *data; void *out;               // the array (compress: read; decompress: written)
    double eb, recip;                          // the bound and 1 / bound, both already rounded to the array's type
    unsigned intervals; int rshift;            // interval count; k_omp_hist_box: log2 of the lane-private copies of its bins
    uint16_t *codes;                           // nb * bel codes
    unsigned *ucount; u64 *ucount64; void *first;      // per box: count of verbatim values, first value
    int count_in_hist, maxlen;                 // compress: the histogram pass fills ucount (the column sweep leaves the counting out); longest code word
    unsigned *hist_box, *hist;                 // compress: nb * intervals bins, intervals bins
    unsigned *radius_hist;                     // compress: the interval optimiser's radius histogram of this array
    u64 *box_bytes, *box_off, *uoff;           // per box: payload bytes, payload offset, rank of its first verbatim value (nb + 1 entries)
    u64 *totals;                               // {payload bytes, verbatim values, boxes in error, samples within the bound}: this array's SM_SCRATCH / SM_TOTAL_UNPRED / SM_ERR / SM_WITHIN
    const u64 *packed;                         // compress: the code table `code << 8 | len`
    unsigned char *stream; const unsigned char *hdr; unsigned hdr_len, pad_;     // compress: where its stream is built (4-byte aligned, zeroed); its header bytes
    u64 off_ucount, off_first, off_unpred, off_sizes, off_pay;                   // compress: the stream's tables
    void *unpred;                              // the array's verbatim values at an aligned address (compress: written; decompress: read)
    const unsigned char *payload; unsigned bytes_before; int n_nodes, tab_lds, pad2_;     // decompress: its payloads, what k_omp_hdec_lut takes per stream
    const unsigned *table; uint4 *lut;         // decompress: the node table, the look-up table built from it
    unsigned *vflags;                          // decompress, column form: nb * fw flag words (k_omp_scatter)
};

template <class T>
__global__ __launch_bounds__(256) void k_ompb_sample(szh_geom3 G, const szh_ompb_rec *__restrict__ recs, const int *__restrict__ list, int64_t nrows, int sd, unsigned max_radius)
{
    const szh_ompb_rec &r = recs[list[blockIdx.y]];
    sample_body<T, false>(G, (const T *)r.data, nrows, sd, r.eb, (T)0, max_radius, r.radius_hist, nullptr, r.totals + 3);
}

// ... of arrays that are VIEWS with the common element pitches p0 / p1 (szhip_compress_omp_batch_view): k_sample_view's body; r.data is the view's first value
template <class T>
__global__ __launch_bounds__(256) void k_ompb_sample_view(szh_geom3 G, const szh_ompb_rec *__restrict__ recs, const int *__restrict__ list, int64_t p0, int64_t p1, int64_t nrows, int sd,
                                                          unsigned max_radius)
{
    const szh_ompb_rec &r = recs[list[blockIdx.y]];
    sample_view_body<T>(threadIdx.x, G, (const T *)r.data, p0, p1, nrows, sd, r.eb, max_radius, r.radius_hist, r.totals + 3);
}

template <class T> __device__ __forceinline__ void ompb_sweep_args(const szh_omp_geom &g, const szh_ompb_rec &r, bool dec, int fw, szh_oc::sweep_args<T> &a)
{
    a.g = g; a.data = dec ? nullptr : (const T *)r.data; a.out = dec ? (T *)r.out : nullptr;
    a.eb = (T)r.eb; a.recip = (T)r.recip; a.intervals = (int)r.intervals; a.codes = r.codes;
    a.ucount = dec ? (unsigned *)(r.totals + 2) : r.ucount; a.ucount64 = dec ? nullptr : r.ucount64; a.first = (T *)r.first;
    a.uoff = dec ? r.uoff : nullptr; a.vflags = dec ? r.vflags : nullptr; a.fw = dec ? fw : 0;
}
// two boxes of the SAME array per wavefront (the box count of an array is even: omp_col_applies).  The sweep itself is szh_oc::sweep; these are the dozen lines of
// k_omp_col around it once more (k_omp_col stays as it is, to the letter: its register allocation is what two wavefronts per SIMD hang on)
template <class T, int C1, int C2, bool DEC, bool COUNT>
__global__ __launch_bounds__(64, (sizeof(T) == 4 ? 2 : 1)) void k_ompb_col(szh_omp_geom g, const szh_ompb_rec *__restrict__ recs, const int *__restrict__ list, int fw)
{
    typedef szh_oc::shape<T, C1, C2> S;
    __shared__ __attribute__((aligned(16))) unsigned char ring_raw[S::RS * S::PITCH];
    __shared__ unsigned flags_raw[DEC ? S::NB * OC_FLAG_WORDS : 1];
    OC_LDS unsigned char *ring = (OC_LDS unsigned char *)ring_raw;
    OC_LDS unsigned *fl = (OC_LDS unsigned *)flags_raw;
    szh_oc::sweep_args<T> a;
    ompb_sweep_args<T>(g, recs[list[blockIdx.y]], DEC, fw, a);
    if (!DEC) { szh_oc::sweep<T, C1, C2, szh_oc::M_CMP, COUNT> s(ring, fl, a); s.run(); }
    else {
        const int b0 = (int)blockIdx.x * S::NB;
        const bool verb = a.uoff[b0 + S::NB] != a.uoff[b0];          // (uniform)
        if (verb) { szh_oc::sweep<T, C1, C2, szh_oc::M_DECV> s(ring, fl, a); s.run(); }
        else { szh_oc::sweep<T, C1, C2, szh_oc::M_DEC> s(ring, fl, a); s.run(); }
    }
}
template <class T, bool DEC, bool VEC>
__global__ __launch_bounds__(1024) void k_ompb_box(szh_omp_geom g, const szh_ompb_rec *__restrict__ recs, const int *__restrict__ list)
{
    const szh_ompb_rec &r = recs[list[blockIdx.y]];
    omp_box_body<T, DEC, VEC>(g, DEC ? nullptr : (const T *)r.data, DEC ? (T *)r.out : nullptr, (T)r.eb, (T)r.recip, (int)r.intervals, r.codes,
                              DEC ? (unsigned *)(r.totals + 2) : r.ucount, DEC ? nullptr : r.ucount64, (T *)r.first, DEC ? (const T *)r.unpred : nullptr, DEC ? r.uoff : nullptr);
}

__global__ __launch_bounds__(256) void k_ompb_hist_box(int bel, const szh_ompb_rec *__restrict__ recs, const int *__restrict__ list, int nb, int per_wg)
{
    const szh_ompb_rec &r = recs[list[blockIdx.y]];
    omp_hist_box_body(bel, r.codes, r.intervals, r.rshift, r.hist_box, r.hist, r.count_in_hist ? r.ucount : nullptr, r.count_in_hist ? r.ucount64 : nullptr, nb, per_wg);
}
// one workgroup per array: every box its size and its place inside its OWN stream, the array's totals
__global__ __launch_bounds__(1024) void k_ompb_layout(int nb, const szh_ompb_rec *__restrict__ recs, const int *__restrict__ list)
{
    const szh_ompb_rec &r = recs[list[blockIdx.y]];
    omp_layout_body(nb, r.intervals, r.hist_box, r.packed, r.ucount64, r.box_bytes, r.box_off, r.uoff, r.totals, r.totals + 1, 0);
}
template <class T>
__global__ __launch_bounds__(256) void k_ompb_encode_box3(szh_omp_geom g, const szh_ompb_rec *__restrict__ recs, const int *__restrict__ list)
{
    const szh_ompb_rec &r = recs[list[blockIdx.y]];
    szh_omp_tables tb;
    tb.stream = r.stream; tb.hdr = r.hdr; tb.hdr_len = r.hdr_len;
    tb.off_ucount = r.off_ucount; tb.off_first = r.off_first; tb.off_unpred = r.off_unpred; tb.off_sizes = r.off_sizes; tb.first = r.first;
    omp_encode_box3_body<T>(g, (const T *)r.data, r.codes, r.packed, r.intervals, (unsigned)r.maxlen, r.box_off, r.box_bytes, r.uoff, r.ucount, r.off_pay * 8,
                            (unsigned *)r.stream, (T *)r.unpred, (unsigned *)(r.totals + 2), tb);
}

__global__ __launch_bounds__(256) void k_ompb_build_lut(const szh_ompb_rec *__restrict__ recs, const int *__restrict__ list)
{
    const szh_ompb_rec &r = recs[list[blockIdx.y]];
    hdec_build_lut_body(r.table, r.lut);
}
__global__ __launch_bounds__(256) void k_ompb_hdec_lut(int bel, const szh_ompb_rec *__restrict__ recs, const int *__restrict__ list, unsigned stage_bytes)
{
    const szh_ompb_rec &r = recs[list[blockIdx.y]];
    omp_hdec_lut_body(bel, r.payload, r.bytes_before, r.box_off, r.box_bytes, r.table, r.n_nodes, r.tab_lds, r.lut, stage_bytes, r.codes, (unsigned *)(r.totals + 2));
}
template <class T>
__global__ __launch_bounds__(256) void k_ompb_scatter(szh_omp_geom g, const szh_ompb_rec *__restrict__ recs, const int *__restrict__ list, int fw)
{
    const szh_ompb_rec &r = recs[list[blockIdx.y]];
    omp_scatter_body<T>(g, r.codes, r.uoff, (const T *)r.unpred, (T *)r.out, (unsigned *)(r.totals + 2), r.vflags, fw);
}

// Pieces of byte arrays that lie anywhere (the caller's streams, the tables inside them) to places in ONE destination buffer, a workgroup per span
// {source address, destination offset, bytes}: 16 bytes per lane where source and destination are aligned alike, else byte by byte (as k_omp_gather)
__global__ __launch_bounds__(256) void k_ompb_fetch(unsigned char *__restrict__ dst, const u64 *__restrict__ spans)
{
    const u64 *sp = spans + 3 * (u64)blockIdx.x;
    const unsigned char *s = reinterpret_cast<const unsigned char *>((uintptr_t)sp[0]);
    unsigned char *d = dst + sp[1];
    const u64 n = sp[2], tid = threadIdx.x;
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15u) == 0) {
        u64 head = (16u - (unsigned)((uintptr_t)s & 15u)) & 15u;
        if (head > n) head = n;
        const u64 n16 = (n - head) / 16, tail = head + n16 * 16;
        if (tid < head) d[tid] = s[tid];
        for (u64 i = tid; i < n16; i += 256) reinterpret_cast<uint4 *>(d + head)[i] = reinterpret_cast<const uint4 *>(s + head)[i];
        if (tail + tid < n) d[tail + tid] = s[tail + tid];            // (fewer than 16 bytes)
    } else for (u64 i = tid; i < n; i += 256) d[i] = s[i];
}

// MANY VIEWS of one shape and one pair of element pitches, each at its own base (the batched view calls): blockIdx.y picks the pair {view base, contiguous copy} of
// `pairs` (two addresses per view), blockIdx.x x 256 + lane the 16-byte piece inside it -- the pieces of k_omp_crop (gather: view -> copy, `per_row` = cpr) and of
// k_view_scatter (scatter: copy -> view, `per_row` = ppr; rows cut at the 16-byte boundaries of the view, which is never read), whose bodies these run.
template <class T>
__global__ __launch_bounds__(256) void k_ompb_crop(const u64 *__restrict__ pairs, int64_t p0, int64_t p1, int e1, int e2, int per_row, int64_t pieces)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (idx >= pieces) return;
    const u64 *pr = pairs + 2 * (u64)blockIdx.y;
    omp_crop_body<T>(reinterpret_cast<const T *>((uintptr_t)pr[0]), p0, p1, reinterpret_cast<T *>((uintptr_t)pr[1]), e1, e2, per_row, idx);
}
template <class T>
__global__ __launch_bounds__(256) void k_ompb_view_scatter(const u64 *__restrict__ pairs, int64_t p0, int64_t p1, int e1, int e2, int per_row, int64_t pieces)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (idx >= pieces) return;
    const u64 *pr = pairs + 2 * (u64)blockIdx.y;
    view_scatter_body<T>(reinterpret_cast<const T *>((uintptr_t)pr[1]), reinterpret_cast<T *>((uintptr_t)pr[0]), p0, p1, e1, e2, per_row, idx);
}

// =====================================================================================================================
// Arrays of DIFFERENT shapes in one launch (szhip_compress_omp_batch_shapes / szhip_decompress_omp_batch_shapes).
// What the kernels above take as an argument -- the box grid, the sampler's geometry and row limit, the boxes per histogram workgroup, the flag words -- is here a
// second per-array record (szh_ompb_geo) beside the first; a workgroup reads both through list[blockIdx.y] (uniform: scalar loads, as the record's).  The grid's first
// dimension is sized to the LARGEST array of the launch's list; a workgroup whose blockIdx.x lies beyond its own array's count returns at once (a uniform test).
// The bodies are the single call's once more; k_ompbs_col repeats k_ompb_col's dozen lines, which repeat k_omp_col's (both stay as they are, to the letter).
// One launch has one block size and one dynamic-LDS size, so k_ompbs_box is launched once per distinct box (c0 x c1 x c2) among the items of a form; the column
// form takes every item with 32 x 32 faces in one launch, whatever its plane count and box count.
struct szh_ompb_geo {
    szh_omp_geom g;                            // the array's own box grid (omp_box_grid of its shape and thread_num)
    szh_geom3 G; int64_t nrows;                // compress: the sampler's geometry and row limit
    int per_wg, fw;                            // compress: boxes per workgroup of the histogram pass; decompress, column form: flag words per box (0: none)
};

template <class T>
__global__ __launch_bounds__(256) void k_ompbs_sample(const szh_ompb_rec *__restrict__ recs, const szh_ompb_geo *__restrict__ geos, const int *__restrict__ list, int sd,
                                                      unsigned max_radius)
{
    const int a = list[blockIdx.y];
    const szh_ompb_geo &e = geos[a];
    if ((int64_t)blockIdx.x * 256 >= e.nrows) return;           // (rows go round the grid: a workgroup beyond the array's rows has none)
    const szh_ompb_rec &r = recs[a];
    sample_body<T, false>(e.G, (const T *)r.data, e.nrows, sd, r.eb, (T)0, max_radius, r.radius_hist, nullptr, r.totals + 3);
}
template <class T, int C1, int C2, bool DEC, bool COUNT>
__global__ __launch_bounds__(64, (sizeof(T) == 4 ? 2 : 1)) void k_ompbs_col(const szh_ompb_rec *__restrict__ recs, const szh_ompb_geo *__restrict__ geos, const int *__restrict__ list)
{
    typedef szh_oc::shape<T, C1, C2> S;
    __shared__ __attribute__((aligned(16))) unsigned char ring_raw[S::RS * S::PITCH];
    __shared__ unsigned flags_raw[DEC ? S::NB * OC_FLAG_WORDS : 1];
    const int ai = list[blockIdx.y];
    const szh_ompb_geo &e = geos[ai];
    if ((int)blockIdx.x * S::NB >= e.g.nb) return;
    OC_LDS unsigned char *ring = (OC_LDS unsigned char *)ring_raw;
    OC_LDS unsigned *fl = (OC_LDS unsigned *)flags_raw;
    szh_oc::sweep_args<T> a;
    ompb_sweep_args<T>(e.g, recs[ai], DEC, e.fw, a);
    if (!DEC) { szh_oc::sweep<T, C1, C2, szh_oc::M_CMP, COUNT> s(ring, fl, a); s.run(); }
    else {
        const int b0 = (int)blockIdx.x * S::NB;
        const bool verb = a.uoff[b0 + S::NB] != a.uoff[b0];          // (uniform)
        if (verb) { szh_oc::sweep<T, C1, C2, szh_oc::M_DECV> s(ring, fl, a); s.run(); }
        else { szh_oc::sweep<T, C1, C2, szh_oc::M_DEC> s(ring, fl, a); s.run(); }
    }
}
// (every array of the list has the launch's box: blockDim.x = c0 * c1 rows, the dynamic LDS of 4 * c0 * pitch values)
template <class T, bool DEC, bool VEC>
__global__ __launch_bounds__(1024) void k_ompbs_box(const szh_ompb_rec *__restrict__ recs, const szh_ompb_geo *__restrict__ geos, const int *__restrict__ list)
{
    const int a = list[blockIdx.y];
    const szh_ompb_geo &e = geos[a];
    if ((int)blockIdx.x >= e.g.nb) return;
    const szh_ompb_rec &r = recs[a];
    omp_box_body<T, DEC, VEC>(e.g, DEC ? nullptr : (const T *)r.data, DEC ? (T *)r.out : nullptr, (T)r.eb, (T)r.recip, (int)r.intervals, r.codes,
                              DEC ? (unsigned *)(r.totals + 2) : r.ucount, DEC ? nullptr : r.ucount64, (T *)r.first, DEC ? (const T *)r.unpred : nullptr, DEC ? r.uoff : nullptr);
}
__global__ __launch_bounds__(256) void k_ompbs_hist_box(const szh_ompb_rec *__restrict__ recs, const szh_ompb_geo *__restrict__ geos, const int *__restrict__ list)
{
    const int a = list[blockIdx.y];
    const szh_ompb_geo &e = geos[a];
    if ((int)blockIdx.x * e.per_wg >= e.g.nb) return;
    const szh_ompb_rec &r = recs[a];
    omp_hist_box_body(e.g.bel, r.codes, r.intervals, r.rshift, r.hist_box, r.hist, r.count_in_hist ? r.ucount : nullptr, r.count_in_hist ? r.ucount64 : nullptr, e.g.nb, e.per_wg);
}
__global__ __launch_bounds__(1024) void k_ompbs_layout(const szh_ompb_rec *__restrict__ recs, const szh_ompb_geo *__restrict__ geos, const int *__restrict__ list)
{
    const int a = list[blockIdx.y];
    const szh_ompb_rec &r = recs[a];
    omp_layout_body(geos[a].g.nb, r.intervals, r.hist_box, r.packed, r.ucount64, r.box_bytes, r.box_off, r.uoff, r.totals, r.totals + 1, 0);
}
template <class T>
__global__ __launch_bounds__(256) void k_ompbs_encode_box3(const szh_ompb_rec *__restrict__ recs, const szh_ompb_geo *__restrict__ geos, const int *__restrict__ list)
{
    const int a = list[blockIdx.y];
    const szh_ompb_geo &e = geos[a];
    if ((int)blockIdx.x >= e.g.nb) return;
    const szh_ompb_rec &r = recs[a];
    szh_omp_tables tb;
    tb.stream = r.stream; tb.hdr = r.hdr; tb.hdr_len = r.hdr_len;
    tb.off_ucount = r.off_ucount; tb.off_first = r.off_first; tb.off_unpred = r.off_unpred; tb.off_sizes = r.off_sizes; tb.first = r.first;
    omp_encode_box3_body<T>(e.g, (const T *)r.data, r.codes, r.packed, r.intervals, (unsigned)r.maxlen, r.box_off, r.box_bytes, r.uoff, r.ucount, r.off_pay * 8,
                            (unsigned *)r.stream, (T *)r.unpred, (unsigned *)(r.totals + 2), tb);
}
__global__ __launch_bounds__(256) void k_ompbs_hdec_lut(const szh_ompb_rec *__restrict__ recs, const szh_ompb_geo *__restrict__ geos, const int *__restrict__ list, unsigned stage_bytes)
{
    const int a = list[blockIdx.y];
    const szh_ompb_geo &e = geos[a];
    if ((int)blockIdx.x >= e.g.nb) return;
    const szh_ompb_rec &r = recs[a];
    omp_hdec_lut_body(e.g.bel, r.payload, r.bytes_before, r.box_off, r.box_bytes, r.table, r.n_nodes, r.tab_lds, r.lut, stage_bytes, r.codes, (unsigned *)(r.totals + 2));
}
template <class T>
__global__ __launch_bounds__(256) void k_ompbs_scatter(const szh_ompb_rec *__restrict__ recs, const szh_ompb_geo *__restrict__ geos, const int *__restrict__ list)
{
    const int a = list[blockIdx.y];
    const szh_ompb_geo &e = geos[a];
    if ((int)blockIdx.x >= e.g.nb) return;
    const szh_ompb_rec &r = recs[a];
    omp_scatter_body<T>(e.g, r.codes, r.uoff, (const T *)r.unpred, (T *)r.out, (unsigned *)(r.totals + 2), r.vflags, e.fw);
}

// =====================================================================================================================
// SUB-BOXES of many streams in one call (szhip_decompress_omp_batch_region).  Every item's "array" is the sub-array of the boxes its region
// meets: the decode and the sweeps are the k_ompbs_* kernels above over compact tables and a sub-geometry per item, into a staging array in the context.  What is new
// is the step behind them: ONE launch that puts every item's region out of its staging array into its destination -- a contiguous array, a view of a padded parent
// (a ghost layer), or a contiguous device buffer that the host then copies out through the pitches.
// A third per-item record, read uniformly per workgroup through list[blockIdx.y] as the other two.  The grid's first dimension is sized to the item with the most
// pieces; the surplus workgroups of a smaller item return at once.  A workgroup whose item's error counter (the sweeps' totals[2]) is not zero returns without writing:
// no host synchronisation lies between the sweeps and the placement, and a damaged item leaves its destination as it was.
struct szh_ompb_place {
    const void *src;                           // the region's FIRST VALUE inside the item's staging array (staging base + the region's offset in its covered boxes)
    void *dst;                                 // the destination's first value
    int64_t s0, s1, d0, d1;                    // element pitches of the staging array (those of the covered boxes) and of the destination
    int e0, e1, e2, ppr;                       // the region's extents; pieces per row: the head and (e2 + VW - 1) / VW more
    const u64 *err;                            // the item's error counter
    u64 pad_;
};
// Piece `idx` of an item: the discipline of view_scatter_body -- every row is cut at the 16-byte boundaries of its DESTINATION, whole pieces are one uint4 store, a
// head and a tail go value by value, nothing outside a row's e2 values is written and no value of the destination is read -- with a source that is itself strided:
// row (k, i) starts at src + k s0 + i s1, which in general sits at another offset modulo 16 than the destination's row.  The source side of a whole piece is one
// uint4 load where its address happens to be aligned, else VW element loads: the lanes of a wavefront read neighbouring pieces of a row, so the element loads of a
// piece hit the lines its neighbours fetch; it is the store that must not straddle a boundary or touch a byte outside the row.
template <class T>
__device__ __forceinline__ void ompb_place_body(const szh_ompb_place &r, int64_t idx)
{
    constexpr int VW = 16 / (int)sizeof(T);
    const int64_t row = idx / r.ppr, k = row / r.e1;
    const int p = (int)(idx - row * r.ppr), i = (int)(row - k * r.e1), e2 = r.e2;
    const T *s = (const T *)r.src + k * r.s0 + (int64_t)i * r.s1;
    T *d = (T *)r.dst + k * r.d0 + (int64_t)i * r.d1;
    int head = (int)(((16u - (unsigned)((uintptr_t)d & 15u)) & 15u) / (unsigned)sizeof(T));      // (`d` is aligned to its element)
    if (head > e2) head = e2;
    const int j0 = p == 0 ? 0 : head + (p - 1) * VW, j1 = p == 0 ? head : (j0 + VW < e2 ? j0 + VW : e2);
    if (p > 0 && j1 - j0 == VW) {
        uint4 v;
        if ((((uintptr_t)(s + j0)) & 15u) == 0) v = *reinterpret_cast<const uint4 *>(s + j0);
        else { T t[VW]; for (int q = 0; q < VW; ++q) t[q] = s[j0 + q]; __builtin_memcpy(&v, t, 16); }
        *reinterpret_cast<uint4 *>(d + j0) = v;
    } else
        for (int j = j0; j < j1; ++j) d[j] = s[j];
}
template <class T>
__global__ __launch_bounds__(256) void k_ompbr_place(const szh_ompb_place *__restrict__ places, const int *__restrict__ list)
{
    const szh_ompb_place &r = places[list[blockIdx.y]];
    const int64_t pieces = (int64_t)r.e0 * r.e1 * r.ppr;
    if ((int64_t)blockIdx.x * 256 >= pieces) return;            // (uniform: a smaller item than the launch's largest)
    if ((unsigned)r.err[0] != 0u) return;                       // (uniform: a box of this item did not decode)
    const int64_t idx = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (idx < pieces) ompb_place_body<T>(r, idx);
}
