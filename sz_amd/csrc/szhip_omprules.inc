// szhip_omprules.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace, in front of szhip_omp.inc): the RULES of the OpenMP container,
// once, for the single calls (szhip_omp.inc), the batch calls (szhip_ompbatch.inc) and the region batch (szhip_ompregion.inc).  Plain host code, no device calls.
// Stream, behind the caller's 4 + MetaDataByteLength parameter bytes (`meta`):
//   u32be thread_num | T eb (big endian) | u32be intervals | u32be tree_bytes | u32be nodes | tree
//   | u32 ucount[nb] | T first[nb] | the boxes' verbatim values, box after box | u64 payload_bytes[nb] | the boxes' Huffman payloads
// (the tables behind the tree in the host's byte order, as the reference memcpy's them).
// =====================================================================================================================
static size_t up16(size_t v) { return (v + 15) / 16 * 16; }
static size_t up64(size_t v) { return (v + 63) / 64 * 64; }
// a box has fewer than 2^28 values, and its payload fewer than 2^28 bytes (the kernels count both in 32 bits, bits included)
static const u64 OMP_BOX_LIMIT = (u64)1 << 28;
// ---- the decode side.  One stream's front in three steps, each on a host pointer to the bytes fetched so far; a step returns null or the reason the stream is refused
// for (the caller makes a FAIL of it, or fails that item of a batch).  Between the steps the caller fetches what the next one needs -- and, after the first, decides
// the box grid: that rule differs between the calls.
template <class T>
struct omp_stream {
    const unsigned char *src = nullptr; size_t len = 0, body_off = 0;       // a batch call: where the caller has the stream (host or device)
    int thread_num = 0; T eb = 0; unsigned intervals = 0; size_t tree_bytes = 0; int node_count = 0;
    size_t fixed = 0, off_ucount = 0, off_first = 0, off_unpred = 0, off_sizes = 0, off_pay = 0, pos = 0;      // (`pos`: where a batch's copy of the stream lies in the context's buffer)
    u64 E = 0, max_box = 0;
    dec_table D;
    std::vector<u64> uoff, bbytes, boff;
    std::vector<unsigned char> hbuf;                          // a device-resident stream of a batch: its first bytes on the host, as far as the rounds have fetched them
    size_t have = 0;

    // 0. how many bytes step 1 needs
    const char *begin(size_t body, size_t stream_len) { body_off = body; len = stream_len; fixed = body + 4 + sizeof(T) + 12; return fixed > len ? "truncated stream" : nullptr; }
    // 1. the fixed fields (hs: the stream's first `fixed` bytes)
    const char *read_fixed(const unsigned char *hs) {
        const unsigned char *q = hs + body_off;
        thread_num = (int)szhost_get_u32be(q); q += 4;
        eb = sizeof(T) == 8 ? (T)szhost_get_f64be(q) : (T)szhost_get_f32be(q); q += sizeof(T);
        intervals = szhost_get_u32be(q); q += 4;
        tree_bytes = szhost_get_u32be(q); q += 4;
        node_count = (int)szhost_get_u32be(q);
        if (intervals < 4 || intervals > 65536 || !(eb > 0)) return "bad OpenMP-container header";
        if (node_count <= 0 || tree_bytes > len || szhost_huff_serial_size(node_count) > tree_bytes) return "truncated stream";
        return nullptr;
    }
    // ... with the grid known: where the tables behind the tree lie; step 2 needs off_unpred bytes
    const char *place_tables(const szh_omp_geom &g) {
        off_ucount = fixed + tree_bytes; off_first = off_ucount + (size_t)g.nb * 4; off_unpred = off_first + (size_t)g.nb * sizeof(T);
        return off_unpred > len ? "truncated stream" : nullptr;
    }
    // 2. the tree, the walk over the boxes' counts of verbatim values (hs: the first off_unpred bytes); step 3 needs the size table at off_sizes .. off_pay
    const char *read_tree_and_counts(const unsigned char *hs, const szh_omp_geom &g) {
        if (!read_tree(hs + fixed, node_count, intervals, D)) return "bad Huffman tree";
        uoff.assign((size_t)g.nb + 1, 0);
        for (int b = 0; b < g.nb; ++b) { uint32_t c; memcpy(&c, hs + off_ucount + (size_t)b * 4, 4); if (c > (uint32_t)g.bel) return "bad verbatim-value count"; uoff[b + 1] = uoff[b] + c; }
        E = uoff[g.nb];
        off_sizes = off_unpred + (size_t)E * sizeof(T); off_pay = off_sizes + (size_t)g.nb * 8;
        return off_pay > len ? "truncated stream" : nullptr;
    }
    // 3. the size table: the caller copies the stream's bytes [off_sizes, off_pay) to size_table(), then the walk
    u64 *size_table(const szh_omp_geom &g) { bbytes.resize((size_t)g.nb); boff.resize((size_t)g.nb); return bbytes.data(); }
    const char *walk_sizes() {
        u64 acc = 0;
        for (size_t b = 0; b < bbytes.size(); ++b) { boff[b] = acc; if (bbytes[b] > len || bbytes[b] >= OMP_BOX_LIMIT) return "bad payload size"; acc += bbytes[b]; max_box = std::max(max_box, bbytes[b]); }
        return off_pay + acc > len ? "truncated stream" : nullptr;
    }
    // the host's bytes of a batch's stream
    const unsigned char *hs(bool on_device) const { return on_device ? hbuf.data() : src; }
};
// the look-up-table decoder (hdec_run_lut) takes boxes whose largest payload, the look-up table and the node table fit a workgroup's LDS; a node table above 13 KiB stays
// in global memory
enum { HDEC_LDS_MAX = 64 * 1024 };
static size_t hdec_stage_lds(size_t stage_bytes) { return ((size_t)SZH_HDEC_SWZ((stage_bytes + 16) / 4) * 4 + 15) / 16 * 16; }
static size_t hdec_tab_lds(int n_nodes) { return (size_t)n_nodes * 8 <= 13 * 1024 ? ((size_t)n_nodes * 8 + 15) / 16 * 16 : 0; }      // the node table's bytes in LDS; 0: not there
static bool hdec_lut_book(int single_symbol, int bel) { return single_symbol < 0 && bel % 8 == 0; }                                  // (what does not depend on the payloads)
struct hdec_fit { bool takes; unsigned stage_bytes; size_t tab_lds; };
static hdec_fit hdec_lut_fit(u64 max_box, int n_nodes, int single_symbol, int bel)
{
    const unsigned stage_bytes = (unsigned)((max_box + 30 + 15) / 16 * 16 + 16);
    const size_t tab_lds = hdec_tab_lds(n_nodes);
    return {hdec_lut_book(single_symbol, bel) && hdec_stage_lds(stage_bytes) + SZH_LUT_BYTES + tab_lds <= HDEC_LDS_MAX, stage_bytes, tab_lds};
}
// one launch has one LDS size: the largest payload's stage, the look-up table, the largest node table that goes to LDS -- or none of them there, if that is too much
struct hdec_launch {
    size_t stage_max = 0, tab_max = 0, lds_lut = 0; bool tabs_in_lds = true;
    void add(const hdec_fit &f) { stage_max = std::max<size_t>(stage_max, f.stage_bytes); tab_max = std::max(tab_max, f.tab_lds); }
    void close() {
        const size_t stage_lds = hdec_stage_lds(stage_max);
        if (stage_lds + SZH_LUT_BYTES + tab_max > HDEC_LDS_MAX) { tabs_in_lds = false; tab_max = 0; }
        lds_lut = stage_lds + SZH_LUT_BYTES + tab_max;
    }
    int tab_lds(int n_nodes) const { return tabs_in_lds && hdec_tab_lds(n_nodes) ? 1 : 0; }
};
// flag words per box: a bit per group of rows one load of the column sweep covers; 0: more than the sweep keeps, it goes without
template <class T> int omp_flag_words(const szh_omp_geom &g) { const int w = (g.c0 * g.c1 / (16 / (int)sizeof(T)) + 31) / 32; return w > OC_FLAG_WORDS ? 0 : w; }
// The boxes that meet [lo, hi): a rectangular sub-grid of the box grid `g`, in sub-grid order (box (i0, i1, i2) is number (i0 n1 + i1) n2 + i2).  Compact tables, the
// pieces of the stream the boxes need (three per run -- for a fixed (dim 0, dim 1) box coordinate the covered boxes are consecutive: their first values, verbatim values,
// payloads; `dst` counted inside its own part of the caller's blob), and the sub-geometry `gs`: the sub-grid's box counts, the pitches of an array of exactly these boxes.
template <class T>
struct omp_subgrid {
    int b0[3] = {0, 0, 0}, cn[3] = {0, 0, 0}, nbc = 0; size_t ext[3] = {0, 0, 0}, n_out = 0; bool direct = false;      // (`direct`: the region ends on box boundaries)
    std::vector<u64> cbytes, coff, cu; u64 Ec = 0, max_box = 0;
    struct piece { size_t src, dst, len; };
    std::vector<piece> pieces;
    size_t pay_len = 0;
    szh_omp_geom gs; int64_t lo_off = 0;                     // (`lo_off`: the element of the staging array -- pitches gs.d0 / gs.d1 -- where the region starts)
    // `dev_base`: the stream's address when it lies on the device (its payloads are then placed at the source's address modulo 16: k_omp_gather / k_ompb_fetch), else null
    void cover(const szh_omp_geom &g, const size_t *lo, const size_t *hi, const omp_stream<T> &s, const unsigned char *dev_base) {
        const int c[3] = {g.c0, g.c1, g.c2};
        direct = true;
        for (int k = 0; k < 3; ++k) {
            b0[k] = (int)(lo[k] / c[k]); cn[k] = (int)((hi[k] - 1) / c[k]) + 1 - b0[k]; ext[k] = hi[k] - lo[k];
            if (lo[k] % c[k] || hi[k] % c[k]) direct = false;
        }
        nbc = cn[0] * cn[1] * cn[2]; n_out = ext[0] * ext[1] * ext[2];
        const size_t runs = (size_t)cn[0] * cn[1];
        cbytes.resize((size_t)nbc); coff.resize((size_t)nbc); cu.assign((size_t)nbc + 1, 0);
        pieces.reserve(runs * 3);
        u64 pos = 0;
        for (size_t r = 0; r < runs; ++r) {
            const int bi = b0[0] + (int)(r / cn[1]), bj = b0[1] + (int)(r % cn[1]);
            const size_t bf = ((size_t)bi * g.ny + bj) * g.nz + b0[2], i0 = r * cn[2];
            for (int q = 0; q < cn[2]; ++q) {
                cbytes[i0 + q] = s.bbytes[bf + q]; max_box = std::max(max_box, s.bbytes[bf + q]);
                cu[i0 + q + 1] = cu[i0 + q] + (s.uoff[bf + q + 1] - s.uoff[bf + q]);
            }
            // the run's payloads lie one behind the other in the stream
            const size_t src = s.off_pay + (size_t)s.boff[bf], len = (size_t)(s.boff[bf + cn[2] - 1] + s.bbytes[bf + cn[2] - 1] - s.boff[bf]);
            if (dev_base) pos += (((uintptr_t)(dev_base + src) & 15u) - (pos & 15u)) & 15u;
            for (int q = 0; q < cn[2]; ++q) coff[i0 + q] = pos + (s.boff[bf + q] - s.boff[bf]);
            pieces.push_back({s.off_first + bf * sizeof(T), i0 * sizeof(T), (size_t)cn[2] * sizeof(T)});
            pieces.push_back({s.off_unpred + (size_t)s.uoff[bf] * sizeof(T), (size_t)cu[i0] * sizeof(T), (size_t)(cu[i0 + cn[2]] - cu[i0]) * sizeof(T)});
            pieces.push_back({src, (size_t)pos, len});
            pos += len;
        }
        Ec = cu[(size_t)nbc]; pay_len = (size_t)pos;
        gs = g;
        gs.nx = cn[0]; gs.ny = cn[1]; gs.nz = cn[2]; gs.nb = nbc;
        gs.d1 = (int64_t)cn[2] * g.c2; gs.d0 = (int64_t)cn[1] * g.c1 * gs.d1;
        gs.vec = g.c2 % 4 == 0 ? 1 : 0;
        lo_off = (int64_t)(lo[0] - (size_t)b0[0] * g.c0) * gs.d0 + (int64_t)(lo[1] - (size_t)b0[1] * g.c1) * gs.d1 + (int64_t)(lo[2] - (size_t)b0[2] * g.c2);
    }
    // the pieces' places in a blob whose three parts start at o_first, o_unp, o_pay
    void place_pieces(size_t o_first, size_t o_unp, size_t o_pay) { for (size_t p = 0; p < pieces.size(); ++p) pieces[p].dst += p % 3 == 0 ? o_first : p % 3 == 1 ? o_unp : o_pay; }
};
// ---- the compress side.  Everything up to the payloads has a known size; the payloads take at most a byte of padding per box
template <class T>
struct omp_layout {
    size_t hdr_len, off_ucount, off_first, off_unpred, off_sizes, off_pay, cap_len;
    omp_layout(size_t meta_len, size_t nb, u64 E, size_t tree_bytes, u64 total_bits) {
        hdr_len = meta_len + 4 + sizeof(T) + 4 + 4 + 4 + tree_bytes;
        off_ucount = hdr_len; off_first = off_ucount + nb * 4; off_unpred = off_first + nb * sizeof(T);
        off_sizes = off_unpred + (size_t)E * sizeof(T); off_pay = off_sizes + nb * 8;
        cap_len = off_pay + (size_t)((total_bits + 7) / 8) + nb;
    }
};
// the header (hdr_len bytes at q): the parameter bytes, the fixed fields, the tree
template <class T>
void omp_write_header(unsigned char *q, const unsigned char *meta, size_t meta_len, size_t nb, T eb, unsigned intervals, const szhost_huff *hf, size_t tree_bytes)
{
    memcpy(q, meta, meta_len); q += meta_len;
    szhost_put_u32be(q, (uint32_t)nb); q += 4;                // (`thread_num` after the grid has been cut: sz_omp.c:122)
    if (sizeof(T) == 8) szhost_put_f64be(q, (double)eb); else szhost_put_f32be(q, (float)eb);
    q += sizeof(T);
    szhost_put_u32be(q, intervals); q += 4;
    szhost_put_u32be(q, (uint32_t)tree_bytes); q += 4;
    szhost_put_u32be(q, (uint32_t)hf->n_nodes); q += 4;
    szhost_huff_tree_write(hf, q);
}
// the packed code table of the fast packer: `code << 8 | len` per symbol
static void omp_packed_table(const std::vector<u64> &tab_code, const std::vector<uint8_t> &tab_len, unsigned intervals, u64 *out)
{
    for (unsigned s = 0; s < intervals; ++s) out[s] = ((tab_code[s] & (tab_len[s] >= 64 ? ~0ull : (1ull << tab_len[s]) - 1)) << 8) | tab_len[s];
}
// a histogram per box (k_omp_hist_box): boxes of a multiple of 8 codes, small alphabets, at most 64 MiB of bins
static bool omp_box_hist_shape(int bel) { return bel % 8 == 0; }
static bool omp_box_hist_book(unsigned intervals, size_t nb) { return intervals <= 1024 && nb * intervals * 4 <= ((size_t)64 << 20); }
// lane-private copies of the bins against same-address atomics -- but no more copies than the box has codes to spread over them
// (a box of 4096 codes with 64 copies of 32 bins spent its time clearing and summing 32 KB: 0.40 ms for 32 768 such boxes)
static int omp_hist_rshift(unsigned intervals, int bel)
{
    int rshift = 0;
    while ((intervals << (rshift + 1)) <= 8192u && rshift < 6 && ((size_t)intervals << (rshift + 1)) * 16 <= (size_t)bel) ++rshift;
    return rshift;
}
static int omp_hist_per_wg(int bel) { return std::max(1, std::min(16, 32768 / std::max(1, bel))); }
// the fast packer (k_omp_layout + k_omp_encode_box3): its LDS, and the books it takes.  (The single call also asks for at most 2048 intervals; a batch has sent more
// than 1024 to the single call before.)
static size_t omp_fast_lds3(unsigned intervals, unsigned maxlen) { return (size_t)intervals * 8 + ((size_t)SZH_OMP_R3 * maxlen / 32 + 4) * 4 + 16; }
static bool omp_fast_packs(unsigned maxlen, size_t lds3) { return maxlen <= 32 && lds3 <= 60 * 1024; }
// the device's totals of one array against its book: the verbatim values, the kernels' error count, the payload bytes (a byte of padding per box at most)
static bool omp_totals_ok(u64 total_unpred, u64 err, u64 pay_bytes, u64 E, u64 total_bits, size_t nb)
{
    const u64 bytes = (total_bits + 7) / 8;
    return total_unpred == E && (unsigned)err == 0 && pay_bytes >= bytes && pay_bytes <= bytes + (u64)nb;
}
