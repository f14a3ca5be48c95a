// szhip_ompregion.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace, behind szhip_ompbatch.inc): SUB-BOXES of many OpenMP-container
// streams in one call (include/szhip.h: szhip_decompress_omp_batch_region; kernels: szh_ompbatch.h; DESIGN section 4.5.8).
// Every item's "array" is the sub-array of the boxes its region meets (omp_region<T>::tables / decode of the single call, per item): compact tables in sub-grid order
// and a sub-geometry in a szh_ompb_geo, so that the decode and the sweeps are the k_ompbs_* launches of the different-shapes call.  Every item is swept into a staging
// array in the context; ONE k_ompbr_place launch then puts all regions into their destinations.  Items that name the same stream share its header read, table walk,
// tree, node table and look-up table.  An item the shared launches do not cover goes through decompress_omp_region_impl from inside the call.
// =====================================================================================================================
// what the host knows of one item's region
struct ompbr_item {
    int slot = -1;                                           // its stream among the call's distinct streams
    int b0[3] = {0, 0, 0}, cn[3] = {0, 0, 0}; size_t ext[3] = {0, 0, 0}, n_out = 0, p0 = 0, p1 = 0;      // first covered box, covered boxes, extents, destination pitches
    int nbc = 0; u64 Ec = 0, max_box = 0;
    szh_omp_geom gs;
    std::vector<u64> cbytes, coff, cu;
    struct piece { size_t src, dst, len; };                 // (src: offset in the stream; dst: offset in the call's data buffer)
    std::vector<piece> pieces;
    size_t o_first = 0, o_unp = 0, o_pay = 0, o_tab = 0, o_code = 0, o_stage = 0, o_dst = 0, o_flag = 0;
    int fw = 0;
};

template <class T>
int decompress_omp_batch_region_impl(szhip_ctx *ctx, szhip_batch_item *items, const szhip_batch_shape *shapes, szhip_batch_region *regions, int count, int stream_on_device,
                                     int out_on_device, szhip_stats *stats)
{
    call_base cb(ctx); szhip_stats &S = cb.S; const hipStream_t st = cb.st;
    enum { BATCH, SINGLE, FAILED };
    // ---- the distinct streams: items with the same (stream, stream_len, body_off) and shape share everything that is read from the stream's front
    std::vector<int> order((size_t)count), slot_of((size_t)count, 0), rep;
    for (int i = 0; i < count; ++i) order[i] = i;
    auto key_less = [&](int a, int b) {
        const szhip_batch_item &x = items[a], &y = items[b];
        if (x.stream != y.stream) return x.stream < y.stream;
        if (x.stream_len != y.stream_len) return x.stream_len < y.stream_len;
        if (x.body_off != y.body_off) return x.body_off < y.body_off;
        if (shapes[a].r0 != shapes[b].r0) return shapes[a].r0 < shapes[b].r0;
        if (shapes[a].r1 != shapes[b].r1) return shapes[a].r1 < shapes[b].r1;
        return shapes[a].r2 < shapes[b].r2;
    };
    std::stable_sort(order.begin(), order.end(), key_less);
    for (int k = 0; k < count; ++k) {
        if (k == 0 || key_less(order[k - 1], order[k])) rep.push_back(order[k]);      // (stable: the first item that names the stream)
        slot_of[order[k]] = (int)rep.size() - 1;
        regions[order[k]].shares = rep.back();
    }
    const int ns = (int)rep.size();
    std::vector<ompb_stream<T>> ps((size_t)ns);
    std::vector<ompb_shape> sh((size_t)ns);
    std::vector<int> sstate((size_t)ns, BATCH);
    std::vector<const char *> why((size_t)ns, "");
    for (int u = 0; u < ns; ++u) {
        ompb_shape &s = sh[u];
        s.r0 = shapes[rep[u]].r0; s.r1 = shapes[rep[u]].r1; s.r2 = shapes[rep[u]].r2; s.n = s.r0 * s.r1 * s.r2; s.nb = 0; s.thread_num = 0; s.rc = SZHIP_OK;
    }
    auto sfail = [&](int u, const char *w) { sstate[u] = FAILED; why[u] = w; };
    // pieces of the callers' device streams to the host, one round for all streams: spans up, one k_ompb_fetch into the context's staging array, one copy down
    TRY(ensure(ctx, ctx->batch_rec, 64));
    std::vector<u64> spans;
    auto fetch_round = [&](const std::vector<size_t> &want) -> int {           // want[u]: bytes of stream u the host needs (0: none)
        if (!stream_on_device) return SZHIP_OK;
        spans.clear();
        size_t bytes = 0;
        std::vector<size_t> at((size_t)ns, 0);
        for (int u = 0; u < ns; ++u) {
            if (sstate[u] == FAILED || want[u] <= ps[u].have) continue;
            at[u] = bytes;
            spans.push_back((u64)(uintptr_t)(items[rep[u]].stream + ps[u].have)); spans.push_back((u64)bytes); spans.push_back((u64)(want[u] - ps[u].have));
            bytes += want[u] - ps[u].have;
        }
        if (spans.empty()) return SZHIP_OK;
        const size_t o_data = up16(spans.size() * 8);
        TRY(ensure(ctx, ctx->seg_hist, o_data + bytes + 64));
        TRY(ensure_pinned(ctx, bytes + 64));
        unsigned char *d = (unsigned char *)ctx->seg_hist.p;
        HIPCHK(hipMemcpyAsync(d, spans.data(), spans.size() * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_ompb_fetch, dim3((unsigned)(spans.size() / 3)), dim3(256), 0, st, d + o_data, (const u64 *)d);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ctx->pinned, d + o_data, bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int u = 0; u < ns; ++u) {
            if (sstate[u] == FAILED || want[u] <= ps[u].have) continue;
            ps[u].hbuf.resize(want[u]);
            memcpy(ps[u].hbuf.data() + ps[u].have, (const unsigned char *)ctx->pinned + at[u], want[u] - ps[u].have);
            ps[u].have = want[u];
        }
        return SZHIP_OK;
    };
    auto hs = [&](int u) { return stream_on_device ? (const unsigned char *)ps[u].hbuf.data() : items[rep[u]].stream; };
    HIPCHK(hipEventRecord(ctx->ev[0], st));
    // ---- 1. headers, trees and per-box tables of the DISTINCT streams: three rounds of fetches at most, the walks of read_header per stream
    const double h0 = now_ms();
    std::vector<size_t> want((size_t)ns, 0);
    for (int u = 0; u < ns; ++u) {
        const szhip_batch_item &it = items[rep[u]];
        ps[u].fixed = it.body_off + 4 + sizeof(T) + 12;
        if (ps[u].fixed > it.stream_len) sfail(u, "truncated stream"); else want[u] = ps[u].fixed;
    }
    TRY(fetch_round(want));
    for (int u = 0; u < ns; ++u) {
        if (sstate[u] == FAILED) { want[u] = 0; continue; }
        const szhip_batch_item &it = items[rep[u]];
        ompb_stream<T> &p = ps[u];
        const unsigned char *q = hs(u) + it.body_off;
        p.thread_num = (int)szhost_get_u32be(q); q += 4;
        p.eb = sizeof(T) == 8 ? (T)szhost_get_f64be(q) : (T)szhost_get_f32be(q); q += sizeof(T);
        p.intervals = szhost_get_u32be(q); q += 4;
        p.tree_bytes = szhost_get_u32be(q); q += 4;
        p.node_count = (int)szhost_get_u32be(q);
        if (p.intervals < 4 || p.intervals > 65536 || !(p.eb > 0)) { sfail(u, "bad OpenMP-container header"); want[u] = 0; continue; }
        if (p.node_count <= 0 || p.tree_bytes > it.stream_len || szhost_huff_serial_size(p.node_count) > p.tree_bytes) { sfail(u, "truncated stream"); want[u] = 0; continue; }
        szh_omp_geom gi;
        if (p.thread_num >= 1 && omp_box_grid(ctx, p.thread_num, sh[u].r0, sh[u].r1, sh[u].r2, &gi) == SZHIP_OK && gi.nb == p.thread_num) {
            sh[u].g = gi; sh[u].nb = (size_t)gi.nb; sh[u].thread_num = p.thread_num;
        }
        if (sh[u].nb == 0) { sstate[u] = SINGLE; want[u] = 0; continue; }      // (no grid of this shape: the single call says what is wrong with it)
        const size_t nb = sh[u].nb;
        p.off_ucount = p.fixed + p.tree_bytes; p.off_first = p.off_ucount + nb * 4; p.off_unpred = p.off_first + nb * sizeof(T);
        if (p.off_unpred > it.stream_len) { sfail(u, "truncated stream"); want[u] = 0; continue; }
        want[u] = p.off_unpred;
    }
    TRY(fetch_round(want));
    for (int u = 0; u < ns; ++u) {
        if (sstate[u] != BATCH) { want[u] = 0; continue; }
        const szhip_batch_item &it = items[rep[u]];
        ompb_stream<T> &p = ps[u];
        if (!read_tree(hs(u) + p.fixed, p.node_count, p.intervals, p.D)) { sfail(u, "bad Huffman tree"); want[u] = 0; continue; }
        p.uoff.assign(sh[u].nb + 1, 0);
        bool ok = true;
        for (int b = 0; b < sh[u].g.nb; ++b) { uint32_t c; memcpy(&c, hs(u) + p.off_ucount + (size_t)b * 4, 4); if (c > (uint32_t)sh[u].g.bel) { ok = false; break; } p.uoff[b + 1] = p.uoff[b] + c; }
        if (!ok) { sfail(u, "bad verbatim-value count"); want[u] = 0; continue; }
        p.E = p.uoff[sh[u].g.nb];
        p.off_sizes = p.off_unpred + (size_t)p.E * sizeof(T); p.off_pay = p.off_sizes + sh[u].nb * 8;
        if (p.off_pay > it.stream_len) { sfail(u, "truncated stream"); want[u] = 0; continue; }
        want[u] = p.off_pay;
    }
    if (stream_on_device)                                      // (the third round wants the box sizes only: not the verbatim values in front of them)
        for (int u = 0; u < ns; ++u) if (sstate[u] == BATCH) { ps[u].hbuf.resize(ps[u].off_sizes); ps[u].have = ps[u].off_sizes; }
    TRY(fetch_round(want));
    for (int u = 0; u < ns; ++u) {
        if (sstate[u] != BATCH) continue;
        const szhip_batch_item &it = items[rep[u]];
        ompb_stream<T> &p = ps[u];
        p.bbytes.resize(sh[u].nb); p.boff.resize(sh[u].nb);
        memcpy(p.bbytes.data(), hs(u) + p.off_sizes, sh[u].nb * 8);
        u64 acc = 0; bool ok = true;
        for (int b = 0; b < sh[u].g.nb; ++b) { p.boff[b] = acc; if (p.bbytes[b] > it.stream_len || p.bbytes[b] >= ((u64)1 << 28)) { ok = false; break; } acc += p.bbytes[b]; }
        if (!ok) { sfail(u, "bad payload size"); continue; }
        if (p.off_pay + acc > it.stream_len) { sfail(u, "truncated stream"); continue; }
        if (!(p.D.single_symbol < 0 && sh[u].g.bel % 8 == 0)) sstate[u] = SINGLE;      // (the look-up-table decoder's conditions on the stream)
    }
    // ---- 2. per item: the covered sub-grid, its compact tables, the pieces of the stream it needs (omp_region<T>::tables), the sub-geometry (omp_region<T>::decode)
    std::vector<ompbr_item> it((size_t)count);
    std::vector<int> state((size_t)count, BATCH);
    std::vector<ompb_shape> ish((size_t)count);               // (what ompb_box_runs / ompb_most_boxes look at: the sub-geometry and its box count)
    size_t data_len = 0, sum_nbc = 0, sum_stage = 0, stage_max = 0, tab_max = 0;
    for (int i = 0; i < count; ++i) {
        ompbr_item &e = it[i];
        const int u = e.slot = slot_of[i];
        state[i] = sstate[u];
        const szhip_batch_region &rg = regions[i];
        for (int k = 0; k < 3; ++k) e.ext[k] = rg.hi[k] - rg.lo[k];
        e.n_out = e.ext[0] * e.ext[1] * e.ext[2];
        e.p1 = rg.pitch1 ? rg.pitch1 : e.ext[2]; e.p0 = rg.pitch1 ? rg.pitch0 : e.ext[1] * e.ext[2];
        memset(&ish[i], 0, sizeof(ish[i]));
        if (state[i] == FAILED) { items[i].rc = SZHIP_ERR_STREAM; snprintf(ctx->err, sizeof(ctx->err), "stream %d of the batch: %s", i, why[u]); continue; }
        if (state[i] != BATCH) continue;
        const szh_omp_geom &g = sh[u].g;
        const ompb_stream<T> &p = ps[u];
        const int c[3] = {g.c0, g.c1, g.c2};
        for (int k = 0; k < 3; ++k) { e.b0[k] = (int)(rg.lo[k] / c[k]); e.cn[k] = (int)((rg.hi[k] - 1) / c[k]) + 1 - e.b0[k]; }
        e.nbc = e.cn[0] * e.cn[1] * e.cn[2];
        const size_t runs = (size_t)e.cn[0] * e.cn[1];
        e.cbytes.resize((size_t)e.nbc); e.coff.resize((size_t)e.nbc); e.cu.assign((size_t)e.nbc + 1, 0);
        e.pieces.reserve(runs * 3);
        u64 pos = 0;
        for (size_t r = 0; r < runs; ++r) {                     // (for a fixed (dim 0, dim 1) box coordinate the covered boxes are consecutive: a run)
            const int bi = e.b0[0] + (int)(r / e.cn[1]), bj = e.b0[1] + (int)(r % e.cn[1]);
            const size_t bf = ((size_t)bi * g.ny + bj) * g.nz + e.b0[2], i0 = r * e.cn[2];
            for (int q = 0; q < e.cn[2]; ++q) {
                e.cbytes[i0 + q] = p.bbytes[bf + q]; e.max_box = std::max(e.max_box, p.bbytes[bf + q]);
                e.cu[i0 + q + 1] = e.cu[i0 + q] + (p.uoff[bf + q + 1] - p.uoff[bf + q]);
            }
            // the run's payloads lie one behind the other in the stream; in the buffer they start at the source's place modulo 16 (k_ompb_fetch)
            const size_t src = p.off_pay + (size_t)p.boff[bf], len = (size_t)(p.boff[bf + e.cn[2] - 1] + p.bbytes[bf + e.cn[2] - 1] - p.boff[bf]);
            if (stream_on_device) pos += (((uintptr_t)(items[i].stream + src) & 15u) - (pos & 15u)) & 15u;
            for (int q = 0; q < e.cn[2]; ++q) e.coff[i0 + q] = pos + (p.boff[bf + q] - p.boff[bf]);
            e.pieces.push_back({p.off_first + bf * sizeof(T), i0 * sizeof(T), (size_t)e.cn[2] * sizeof(T)});
            e.pieces.push_back({p.off_unpred + (size_t)p.uoff[bf] * sizeof(T), (size_t)e.cu[i0] * sizeof(T), (size_t)(e.cu[i0 + e.cn[2]] - e.cu[i0]) * sizeof(T)});
            e.pieces.push_back({src, (size_t)pos, len});
            pos += len;
        }
        e.Ec = e.cu[(size_t)e.nbc];
        regions[i].n_boxes = (uint64_t)e.nbc;
        // the look-up-table decoder's conditions (omp_dec::huffman_decode) on the COVERED payloads
        const unsigned stage_bytes = (unsigned)((e.max_box + 30 + 15) / 16 * 16 + 16);
        const size_t stage_lds = ((size_t)SZH_HDEC_SWZ((stage_bytes + 16) / 4) * 4 + 15) / 16 * 16;
        const int tab_lds = (size_t)p.D.n_nodes * 8 <= 13 * 1024;
        if (stage_lds + SZH_LUT_BYTES + (tab_lds ? ((size_t)p.D.n_nodes * 8 + 15) / 16 * 16 : 0) > 64 * 1024) { state[i] = SINGLE; continue; }
        stage_max = std::max<size_t>(stage_max, stage_bytes);
        if (tab_lds) tab_max = std::max(tab_max, ((size_t)p.D.n_nodes * 8 + 15) / 16 * 16);
        // [first values][verbatim values][64 bytes, the payloads, 64 zero bytes] of this item in the call's data buffer
        e.o_first = data_len; e.o_unp = e.o_first + up16((size_t)e.nbc * sizeof(T)); e.o_pay = e.o_unp + up16((size_t)e.Ec * sizeof(T)) + 64;
        data_len = up16(e.o_pay + (size_t)pos + 64);
        for (size_t k = 0; k < e.pieces.size(); ++k) e.pieces[k].dst += k % 3 == 0 ? e.o_first : k % 3 == 1 ? e.o_unp : e.o_pay;
        // the sub-geometry: the sub-grid's box counts, the pitches of an array of exactly these boxes
        e.gs = g;
        e.gs.nx = e.cn[0]; e.gs.ny = e.cn[1]; e.gs.nz = e.cn[2]; e.gs.nb = e.nbc;
        e.gs.d1 = (int64_t)e.cn[2] * g.c2; e.gs.d0 = (int64_t)e.cn[1] * g.c1 * e.gs.d1;
        e.gs.vec = g.c2 % 4 == 0 ? 1 : 0;
        e.fw = (g.c0 * g.c1 / (16 / (int)sizeof(T)) + 31) / 32;
        if (e.fw > OC_FLAG_WORDS) e.fw = 0;
        ish[i].g = e.gs; ish[i].nb = (size_t)e.nbc;
        sum_nbc += (size_t)e.nbc; sum_stage += (size_t)e.nbc * g.bel;
    }
    // one launch has one LDS size: the largest payload's stage, the look-up table, the largest node table that goes to LDS -- or none of them there, if that is too much
    const size_t stage_lds = ((size_t)SZH_HDEC_SWZ((stage_max + 16) / 4) * 4 + 15) / 16 * 16;
    bool tabs_in_lds = true;
    if (stage_lds + SZH_LUT_BYTES + tab_max > 64 * 1024) { tabs_in_lds = false; tab_max = 0; }
    const size_t lds_lut = stage_lds + SZH_LUT_BYTES + tab_max;
    cb.host_ms += now_ms() - h0;
    TRY(ompb_limits(ctx, count, sum_nbc, sum_stage));
    // ---- 3. the places of the work arrays, the table
    ompb_table tab(ctx, count, true);
    std::vector<size_t> o_str((size_t)ns, 0);                  // per distinct stream: [node table][look-up table] behind the lists
    std::vector<int> lut_item((size_t)ns, -1);                 // ... and the batched item that builds its look-up table
    size_t ex = 0, n_codes = 0, stage_bytes_all = 0, dst_bytes = 0, n_flags = 0, n_spans = 0, most_pieces = 1;
    for (int i = 0; i < count; ++i) {
        if (state[i] != BATCH) continue;
        ompbr_item &e = it[i];
        const int u = e.slot;
        if (lut_item[u] < 0) { lut_item[u] = i; o_str[u] = ex; ex += up64(ps[u].D.dtab.size() * 4) + SZH_LUT_BYTES + 64; tab.list[OMPB_L_ALL].push_back(i); }
        e.o_tab = ex; ex += up16((size_t)e.nbc * 8) * 2 + up16(((size_t)e.nbc + 1) * 8);
        e.o_code = n_codes; n_codes += (size_t)e.nbc * sh[u].g.bel;
        e.o_stage = stage_bytes_all; stage_bytes_all += up16((size_t)e.nbc * sh[u].g.bel * sizeof(T));
        e.o_dst = dst_bytes; dst_bytes += up16(e.n_out * sizeof(T));
        e.o_flag = n_flags; n_flags += (size_t)e.nbc * e.fw;
        if (stream_on_device) for (const ompbr_item::piece &pc : e.pieces) if (pc.len) ++n_spans;
        tab.list[OMPB_L_ENT].push_back(i);
    }
    const int n_ent = (int)tab.list[OMPB_L_ENT].size(), n_lut = (int)tab.list[OMPB_L_ALL].size();
    if (n_ent > 0) {
        const size_t o_spans = ex;
        ex += n_spans * 24;
        const size_t o_place = up64(ex);
        ex = o_place + (size_t)count * sizeof(szh_ompb_place);
        TRY(tab.reserve(ex));
        TRY(ensure(ctx, ctx->stream_buf, data_len + 64));
        TRY(ensure(ctx, ctx->codes_nat, n_codes * 2 + 64));
        TRY(ensure(ctx, ctx->out, stage_bytes_all + 16));
        if (!out_on_device) TRY(ensure(ctx, ctx->codes_blk, dst_bytes + 16));
        if (n_flags > 0) TRY(ensure(ctx, ctx->chunk_bits, n_flags * 4));
        unsigned char *d_data = (unsigned char *)ctx->stream_buf.p;
        std::vector<unsigned char> extra(ex, 0);
        u64 *sp = (u64 *)(extra.data() + o_spans);
        szh_ompb_place *pl = (szh_ompb_place *)(extra.data() + o_place);
        bool any_flags = false;
        for (int u = 0; u < ns; ++u) if (lut_item[u] >= 0) memcpy(extra.data() + o_str[u], ps[u].D.dtab.data(), ps[u].D.dtab.size() * 4);
        for (int i : tab.list[OMPB_L_ENT]) {
            ompbr_item &e = it[i];
            const int u = e.slot;
            const ompb_stream<T> &p = ps[u];
            const szh_omp_geom &g = sh[u].g;
            szh_ompb_rec &r = tab.rec[i];
            unsigned char *dx = tab.dev() + tab.o_extra, *hx = extra.data() + e.o_tab;
            r.table = (const unsigned *)(dx + o_str[u]); r.lut = (uint4 *)(dx + o_str[u] + up64(p.D.dtab.size() * 4));
            size_t o = e.o_tab;
            memcpy(hx, e.cbytes.data(), (size_t)e.nbc * 8); r.box_bytes = (u64 *)(dx + o); o += up16((size_t)e.nbc * 8); hx = extra.data() + o;
            memcpy(hx, e.coff.data(), (size_t)e.nbc * 8); r.box_off = (u64 *)(dx + o); o += up16((size_t)e.nbc * 8); hx = extra.data() + o;
            memcpy(hx, e.cu.data(), ((size_t)e.nbc + 1) * 8); r.uoff = (u64 *)(dx + o);
            T *stage = (T *)((char *)ctx->out.p + e.o_stage);
            r.out = stage;
            r.eb = (double)p.eb; r.recip = (double)(T)(1 / p.eb); r.intervals = p.intervals;
            r.codes = (uint16_t *)ctx->codes_nat.p + e.o_code;
            r.first = d_data + e.o_first; r.unpred = d_data + e.o_unp;
            r.totals = tab.totals(i);
            r.payload = d_data + e.o_pay; r.bytes_before = (unsigned)std::min<size_t>(e.o_pay, 0x7fffffffu);
            r.n_nodes = p.D.n_nodes; r.tab_lds = tabs_in_lds && (size_t)p.D.n_nodes * 8 <= 13 * 1024 ? 1 : 0;
            // the sweep form: the single region call's rule (omp_dec::sweep) on the sub-geometry and the staging array
            const int form = omp_form(e.gs, stage, sizeof(T), (size_t)e.gs.d0, (size_t)e.gs.d1);
            items[i].quant_kernel = form; items[i].intervals = p.intervals; items[i].n_unpred = e.Ec; items[i].batched = 1;
            tab.geo[i].g = e.gs; tab.geo[i].fw = e.fw;
            tab.list[form == 3 ? OMPB_L_F3 : form == 4 ? OMPB_L_F4 : OMPB_L_F5].push_back(i);
            if (form == 3 && e.Ec > 0) {
                tab.list[OMPB_L_PACKD].push_back(i);           // (here: the items k_omp_scatter runs for)
                if (e.fw > 0) { r.vflags = (unsigned *)ctx->chunk_bits.p + e.o_flag; any_flags = true; }
            }
            if (stream_on_device) for (const ompbr_item::piece &pc : e.pieces) if (pc.len) { *sp++ = (u64)(uintptr_t)(items[i].stream + pc.src); *sp++ = (u64)pc.dst; *sp++ = (u64)pc.len; }
            // the placement: out of the staging array -- the region starts inside its first covered box -- into the destination, or (a host destination) contiguous
            // into the context's buffer, out of which its rows are copied
            szh_ompb_place &q = pl[i];
            const szhip_batch_region &rg = regions[i];
            q.src = stage + (int64_t)(rg.lo[0] - (size_t)e.b0[0] * g.c0) * e.gs.d0 + (int64_t)(rg.lo[1] - (size_t)e.b0[1] * g.c1) * e.gs.d1 + (int64_t)(rg.lo[2] - (size_t)e.b0[2] * g.c2);
            q.s0 = e.gs.d0; q.s1 = e.gs.d1;
            if (out_on_device) { q.dst = items[i].out; q.d0 = (int64_t)e.p0; q.d1 = (int64_t)e.p1; }
            else { q.dst = (char *)ctx->codes_blk.p + e.o_dst; q.d0 = (int64_t)(e.ext[1] * e.ext[2]); q.d1 = (int64_t)e.ext[2]; }
            q.e0 = (int)e.ext[0]; q.e1 = (int)e.ext[1]; q.e2 = (int)e.ext[2];
            q.ppr = 1 + (int)((e.ext[2] + 16 / sizeof(T) - 1) / (16 / sizeof(T)));
            q.err = tab.totals(i) + 2;
            most_pieces = std::max(most_pieces, e.ext[0] * e.ext[1] * (size_t)q.ppr);
            S.n_elements += (uint64_t)e.n_out; S.n_blocks += (uint64_t)e.nbc; S.n_unpred += e.Ec;
        }
        // ---- 4. one upload of the table; the covered boxes' first values, verbatim values and payloads: one pinned blob and one upload (host streams), or one gather
        // launch over all items' spans (device streams)
        TRY(tab.clear_totals());
        if (any_flags) HIPCHK(hipMemsetAsync(ctx->chunk_bits.p, 0, n_flags * 4, st));
        std::vector<int> box_runs[2];                           // where the runs of equal boxes end in the lists of forms 4 and 5
        box_runs[0] = ompb_box_runs(tab.list[OMPB_L_F4], ish); box_runs[1] = ompb_box_runs(tab.list[OMPB_L_F5], ish);
        TRY(tab.upload(0, extra));
        if (stream_on_device) {
            HIPCHK(hipMemsetAsync(d_data, 0, data_len + 64, st));
            if (n_spans) {
                hipLaunchKernelGGL(k_ompb_fetch, dim3((unsigned)n_spans), dim3(256), 0, st, d_data, (const u64 *)(tab.dev() + tab.o_extra + o_spans));
                HIPCHK(hipGetLastError());
            }
        } else {
            TRY(ensure_pinned3(ctx, data_len + 64));
            unsigned char *hb = (unsigned char *)ctx->pinned3;
            memset(hb, 0, data_len + 64);
            for (int i : tab.list[OMPB_L_ENT]) for (const ompbr_item::piece &pc : it[i].pieces) memcpy(hb + pc.dst, items[i].stream + pc.src, pc.len);
            HIPCHK(hipMemcpyAsync(d_data, hb, data_len + 64, hipMemcpyHostToDevice, st));
        }
        // ---- 5. the look-up tables (one per distinct stream), the Huffman decode of all covered boxes
        hipLaunchKernelGGL(k_ompb_build_lut, dim3(SZH_LUT_SIZE / 256, (unsigned)n_lut), dim3(256), 0, st, tab.d_rec(), tab.d_list(OMPB_L_ALL));
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ompbs_hdec_lut, dim3((unsigned)ompb_most_boxes(tab.list[OMPB_L_ENT], 0, n_ent, ish), (unsigned)n_ent), dim3(256), lds_lut, st, tab.d_rec(), tab.d_geo(),
                           tab.d_list(OMPB_L_ENT), (unsigned)stage_max);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[1], st));
        // ---- 6. the sweeps into the staging arrays: one column launch, one box launch per distinct box of a form (as szhip_decompress_omp_batch_shapes)
        HIPCHK(hipEventRecord(ctx->ev[2], st));
        const int n3 = (int)tab.list[OMPB_L_F3].size(), nsc = (int)tab.list[OMPB_L_PACKD].size();
        if (nsc) hipLaunchKernelGGL((k_ompbs_scatter<T>), dim3((unsigned)ompb_most_boxes(tab.list[OMPB_L_PACKD], 0, nsc, ish), (unsigned)nsc), dim3(256), 0, st, tab.d_rec(), tab.d_geo(),
                                    tab.d_list(OMPB_L_PACKD));
        if (n3) hipLaunchKernelGGL((k_ompbs_col<T, 32, 32, true, true>), dim3((unsigned)(ompb_most_boxes(tab.list[OMPB_L_F3], 0, n3, ish) / 2), (unsigned)n3), dim3(64), 0, st, tab.d_rec(),
                                   tab.d_geo(), tab.d_list(OMPB_L_F3));
        S.quant_kernel_launches += n3 ? 1 : 0;
        for (int form = 4; form <= 5; ++form) {
            const int which = form == 4 ? OMPB_L_F4 : OMPB_L_F5;
            int from = 0;
            for (int to : box_runs[form - 4]) {
                const szh_omp_geom &gb = ish[tab.list[which][from]].g;
                const dim3 grid((unsigned)ompb_most_boxes(tab.list[which], from, to, ish), (unsigned)(to - from)), block((unsigned)(gb.c0 * gb.c1));
                const size_t lds = (size_t)4 * gb.c0 * gb.pitch * sizeof(T);
                if (form == 4) hipLaunchKernelGGL((k_ompbs_box<T, true, true>), grid, block, lds, st, tab.d_rec(), tab.d_geo(), tab.d_list(which) + from);
                else hipLaunchKernelGGL((k_ompbs_box<T, true, false>), grid, block, lds, st, tab.d_rec(), tab.d_geo(), tab.d_list(which) + from);
                ++S.quant_kernel_launches;
                from = to;
            }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[3], st));
        S.quant_kernel = items[tab.list[OMPB_L_ENT][0]].quant_kernel;
        // ---- 7. ONE placing launch: every item whose boxes all decoded (the sweeps' counts are read on the device: no synchronisation in front of it)
        hipLaunchKernelGGL((k_ompbr_place<T>), dim3((unsigned)((most_pieces + 255) / 256), (unsigned)n_ent), dim3(256), 0, st,
                           (const szh_ompb_place *)(tab.dev() + tab.o_extra + o_place), tab.d_list(OMPB_L_ENT));
        HIPCHK(hipGetLastError());
        ++S.packing;
        // ---- 8. the items' error counts; host destinations: one copy down, then the rows of the items that decoded
        TRY(ensure_pinned(ctx, (size_t)count * 32));
        HIPCHK(hipMemcpyAsync(ctx->pinned, tab.dev(), (size_t)count * 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const u64 *h_tot = (const u64 *)ctx->pinned;
        float ms = 0;
        hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); S.ms_entropy = ms;
        hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]); S.ms_quant = ms;
        for (int i : tab.list[OMPB_L_ENT])
            if ((unsigned)h_tot[4 * (size_t)i + 2] != 0) {
                state[i] = FAILED; items[i].rc = SZHIP_ERR_STREAM;
                snprintf(ctx->err, sizeof(ctx->err), "stream %d of the batch: boxes of the region whose payload or verbatim-value count does not fit their codes", i);
            }
        if (!out_on_device) {
            std::vector<unsigned char> tmp(dst_bytes);
            TRY(staged_copy(ctx, tmp.data(), ctx->codes_blk.p, tmp.size(), false));
            for (int i : tab.list[OMPB_L_ENT]) {
                if (state[i] != BATCH) continue;
                const ompbr_item &e = it[i];
                const host_view hv = {e.ext[1], e.ext[2] * sizeof(T), e.p0 * sizeof(T), e.p1 * sizeof(T)};
                host_view_move(hv, (char *)items[i].out, (char *)tmp.data() + e.o_dst, 0, e.n_out * sizeof(T), false);
            }
        }
    } else HIPCHK(hipStreamSynchronize(st));
    // ---- the items the shared launches do not cover: the single region call; a view is placed behind it (szhip_scatter_view on the device, its rows on the host)
    for (int i = 0; i < count; ++i) {
        if (state[i] != SINGLE) continue;
        const ompbr_item &e = it[i];
        const ompb_shape &s = sh[e.slot];
        const szhip_batch_item &m = items[i];
        szhip_stats s1; memset(&s1, 0, sizeof(s1));
        const bool contiguous = e.p1 == e.ext[2] && e.p0 == e.ext[1] * e.ext[2];
        int rc;
        if (contiguous) rc = decompress_omp_region_impl<T>(ctx, m.stream, stream_on_device, m.stream_len, m.body_off, s.r0, s.r1, s.r2, regions[i].lo, regions[i].hi, m.out, out_on_device, &s1);
        else if (out_on_device) {
            rc = ensure(ctx, ctx->in, e.n_out * sizeof(T));
            if (rc == SZHIP_OK) rc = decompress_omp_region_impl<T>(ctx, m.stream, stream_on_device, m.stream_len, m.body_off, s.r0, s.r1, s.r2, regions[i].lo, regions[i].hi, ctx->in.p, 1, &s1);
            if (rc == SZHIP_OK) rc = scatter_view_impl<T>(ctx, ctx->in.p, e.ext[0], e.ext[1], e.ext[2], m.out, 1, e.p0, e.p1);
        } else {
            std::vector<T> tmp(e.n_out);
            rc = decompress_omp_region_impl<T>(ctx, m.stream, stream_on_device, m.stream_len, m.body_off, s.r0, s.r1, s.r2, regions[i].lo, regions[i].hi, tmp.data(), 0, &s1);
            const host_view hv = {e.ext[1], e.ext[2] * sizeof(T), e.p0 * sizeof(T), e.p1 * sizeof(T)};
            if (rc == SZHIP_OK) host_view_move(hv, (char *)m.out, (char *)tmp.data(), 0, e.n_out * sizeof(T), false);
        }
        items[i].rc = rc; items[i].batched = 0;
        if (rc != SZHIP_OK) { hipStreamSynchronize(st); continue; }
        items[i].intervals = s1.intervals; items[i].n_unpred = s1.n_unpred; items[i].quant_kernel = s1.quant_kernel;
        regions[i].n_boxes = s1.n_blocks;
        S.n_elements += s1.n_elements; S.n_blocks += s1.n_blocks; S.n_unpred += s1.n_unpred;
    }
    int rc_all = SZHIP_OK;
    for (int i = 0; i < count; ++i) if (items[i].rc != SZHIP_OK && rc_all == SZHIP_OK) rc_all = items[i].rc;
    S.out_bytes = S.n_elements * sizeof(T);
    S.ms_host = cb.host_ms; S.ms_total = now_ms() - cb.t_begin;
    if (stats) *stats = S;
    return rc_all;
}
