// szhip_ompregion.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace, behind szhip_ompbatch.inc): SUB-BOXES of many OpenMP-container
// streams in one call (include/szhip.h: szhip_decompress_omp_batch_region; kernels: szh_ompbatch.h; DESIGN section 4.5.8).
// Every item's "array" is the sub-array of the boxes its region meets (omp_region<T>::tables / decode of the single call, per item): compact tables in sub-grid order
// and a sub-geometry in a szh_ompb_geo, so that the decode and the sweeps are the k_ompbs_* launches of the different-shapes call.  Every item is swept into a staging
// array in the context; ONE k_ompbr_place launch then puts all regions into their destinations.  Items that name the same stream share its header read, table walk,
// tree, node table and look-up table.  An item the shared launches do not cover goes through decompress_omp_region_impl from inside the call.
// =====================================================================================================================
// what the host knows of one item's region: the covered sub-grid (omp_subgrid), and where its parts lie in the call's buffers
template <class T>
struct ompbr_item : omp_subgrid<T> {
    int slot = -1;                                           // its stream among the call's distinct streams
    size_t p0 = 0, p1 = 0;                                   // destination pitches
    size_t o_first = 0, o_unp = 0, o_pay = 0, o_tab = 0, o_code = 0, o_stage = 0, o_dst = 0, o_flag = 0;      // (o_first .. o_pay: in the call's data buffer, where the pieces go)
    int fw = 0;
};
// One szhip_decompress_omp_batch_region call: its state, and one member function per step (decompress_omp_batch_region_impl is their sequence).  What they rely on:
//  - Context buffers.  seg_hist and the pinned block serve the fetch rounds of read_fronts alone.  fill_table sizes batch_rec (the table), stream_buf (the covered boxes'
//    values and payloads), codes_nat, out (the staging arrays), codes_blk (host destinations) and chunk_bits ONCE, before the records that point into them are filled.  The
//    single region calls use stream_buf, codes_nat, out and codes_blk themselves: they run in finish(), after launches() has read back what the shared launches left there.
//  - The table is reserved once and uploaded once; records are filled after that reserve, so no address in them moves.
//  - `tab` is a member: its image[version] vectors, the pageable sources of the asynchronous uploads, outlive the upload; launches() ends synchronised.
template <class T>
struct ompbr_call : call_base {
    szhip_batch_item *const items; const szhip_batch_shape *const shapes; szhip_batch_region *const regions; const int count, stream_on_device, out_on_device;
    std::vector<int> slot_of, rep; int ns = 0;                // the distinct streams: item -> stream, stream -> its first item
    std::vector<omp_stream<T>> ps; std::vector<ompb_shape> sh; std::vector<int> sstate; std::vector<const char *> why;
    std::vector<ompbr_item<T>> it; std::vector<int> state; size_t data_len = 0; hdec_launch hl;      // the items
    std::vector<ompb_shape> ish;                              // (what ompb_box_runs / ompb_most_boxes look at: the sub-geometry and its box count)
    ompb_table tab{ctx, count, true};
    std::vector<size_t> o_str;                                // per distinct stream: [node table][look-up table] behind the lists
    std::vector<int> lut_item;                                // ... and the batched item that builds its look-up table
    size_t ex = 0, n_codes = 0, stage_bytes_all = 0, dst_bytes = 0, n_flags = 0, n_spans = 0, most_pieces = 1, o_spans = 0, o_place = 0;
    int n_ent = 0, n_lut = 0; bool any_flags = false; std::vector<unsigned char> extra; unsigned char *d_data = nullptr;
    // ---- the distinct streams: items with the same (stream, stream_len, body_off) and shape share everything that is read from the stream's front
    int read_fronts() {
        std::vector<int> order((size_t)count);
        slot_of.assign((size_t)count, 0);
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
        ns = (int)rep.size();
        ps.resize((size_t)ns); sh.resize((size_t)ns); sstate.assign((size_t)ns, OMPB_BATCH); why.assign((size_t)ns, "");
        for (int u = 0; u < ns; ++u) sh[u] = ompb_shape_of(shapes[rep[u]].r0, shapes[rep[u]].r1, shapes[rep[u]].r2);
        // 1. headers, trees and per-box tables of the DISTINCT streams (every stream's own grid, as in the different-shapes call)
        TRY(ensure(ctx, ctx->batch_rec, 64));
        HIPCHK(hipEventRecord(ctx->ev[0], st));
        const double h0 = now_ms();                            // (szhip_stats.ms_host: the fronts read and walked here, the compact tables built in cover_regions)
        auto sfail = [&](int u, const char *w) { sstate[u] = OMPB_FAILED; why[u] = w; };
        for (int u = 0; u < ns; ++u) {
            ps[u].src = items[rep[u]].stream;
            if (const char *w = ps[u].begin(items[rep[u]].body_off, items[rep[u]].stream_len)) sfail(u, w);
        }
        TRY(batch_read_fronts<T>(ctx, st, stream_on_device != 0, ps, sh, sstate, [&](int u) { ompb_own_grid(ctx, ps[u].thread_num, sh[u]); }, sfail));
        for (int u = 0; u < ns; ++u)
            if (sstate[u] == OMPB_BATCH && !hdec_lut_book(ps[u].D.single_symbol, sh[u].g.bel)) sstate[u] = OMPB_SINGLE;      // (the look-up-table decoder's conditions on the stream)
        host_ms += now_ms() - h0;
        return SZHIP_OK;
    }
    // ---- 2. per item (3.: the places of its work arrays): the covered sub-grid, its compact tables, the pieces of the stream it needs, the sub-geometry (omp_subgrid, as the single region call)
    int cover_regions() {
        const double h0 = now_ms();
        it.resize((size_t)count); state.assign((size_t)count, OMPB_BATCH); ish.resize((size_t)count);
        size_t sum_nbc = 0, sum_stage = 0;
        for (int i = 0; i < count; ++i) {
            ompbr_item<T> &e = it[i];
            const int u = e.slot = slot_of[i];
            state[i] = sstate[u];
            const szhip_batch_region &rg = regions[i];
            for (int k = 0; k < 3; ++k) e.ext[k] = rg.hi[k] - rg.lo[k];      // (the single calls want them of every item)
            e.n_out = e.ext[0] * e.ext[1] * e.ext[2];
            e.p1 = rg.pitch1 ? rg.pitch1 : e.ext[2]; e.p0 = rg.pitch1 ? rg.pitch0 : e.ext[1] * e.ext[2];
            memset(&ish[i], 0, sizeof(ish[i]));
            if (state[i] == OMPB_FAILED) { items[i].rc = SZHIP_ERR_STREAM; snprintf(ctx->err, sizeof(ctx->err), "stream %d of the batch: %s", i, why[u]); continue; }
            if (state[i] != OMPB_BATCH) continue;
            const szh_omp_geom &g = sh[u].g;
            const omp_stream<T> &p = ps[u];
            e.cover(g, rg.lo, rg.hi, p, stream_on_device ? items[i].stream : nullptr);
            regions[i].n_boxes = (uint64_t)e.nbc;
            // the look-up-table decoder's conditions on the COVERED payloads
            const hdec_fit fit = hdec_lut_fit(e.max_box, p.D.n_nodes, p.D.single_symbol, g.bel);
            if (!fit.takes) { state[i] = OMPB_SINGLE; continue; }
            hl.add(fit);
            // [first values][verbatim values][64 bytes, the payloads, 64 zero bytes] of this item in the call's data buffer
            e.o_first = data_len; e.o_unp = e.o_first + up16((size_t)e.nbc * sizeof(T)); e.o_pay = e.o_unp + up16((size_t)e.Ec * sizeof(T)) + 64;
            data_len = up16(e.o_pay + e.pay_len + 64);
            e.place_pieces(e.o_first, e.o_unp, e.o_pay);
            e.fw = omp_flag_words<T>(g);
            ish[i].g = e.gs; ish[i].nb = (size_t)e.nbc;
            sum_nbc += (size_t)e.nbc; sum_stage += (size_t)e.nbc * g.bel;
        }
        hl.close();
        host_ms += now_ms() - h0;
        TRY(ompb_limits(ctx, count, sum_nbc, sum_stage));
        // 3. the places of the work arrays, the lists of the decode
        o_str.assign((size_t)ns, 0); lut_item.assign((size_t)ns, -1);
        for (int i = 0; i < count; ++i) {
            if (state[i] != OMPB_BATCH) continue;
            ompbr_item<T> &e = it[i];
            const int u = e.slot;
            if (lut_item[u] < 0) { lut_item[u] = i; o_str[u] = ex; ex += up64(ps[u].D.dtab.size() * 4) + SZH_LUT_BYTES + 64; tab.list[OMPB_L_ALL].push_back(i); }
            e.o_tab = ex; ex += up16((size_t)e.nbc * 8) * 2 + up16(((size_t)e.nbc + 1) * 8);
            e.o_code = n_codes; n_codes += (size_t)e.nbc * sh[u].g.bel;
            e.o_stage = stage_bytes_all; stage_bytes_all += up16((size_t)e.nbc * sh[u].g.bel * sizeof(T));
            e.o_dst = dst_bytes; dst_bytes += up16(e.n_out * sizeof(T));
            e.o_flag = n_flags; n_flags += (size_t)e.nbc * e.fw;
            if (stream_on_device) for (const auto &pc : e.pieces) if (pc.len) ++n_spans;
            tab.list[OMPB_L_ENT].push_back(i);
        }
        n_ent = (int)tab.list[OMPB_L_ENT].size(); n_lut = (int)tab.list[OMPB_L_ALL].size();
        return SZHIP_OK;
    }
    // ... the buffers, every item's record, sweep form and placement
    int fill_table() {
        if (n_ent == 0) return SZHIP_OK;
        o_spans = ex;
        ex += n_spans * 24;
        o_place = up64(ex);
        ex = o_place + (size_t)count * sizeof(szh_ompb_place);
        TRY(tab.reserve(ex));
        TRY(ensure(ctx, ctx->stream_buf, data_len + 64));
        TRY(ensure(ctx, ctx->codes_nat, n_codes * 2 + 64));
        TRY(ensure(ctx, ctx->out, stage_bytes_all + 16));
        if (!out_on_device) TRY(ensure(ctx, ctx->codes_blk, dst_bytes + 16));
        if (n_flags > 0) TRY(ensure(ctx, ctx->chunk_bits, n_flags * 4));
        d_data = (unsigned char *)ctx->stream_buf.p;
        extra.assign(ex, 0);
        u64 *sp = (u64 *)(extra.data() + o_spans);
        szh_ompb_place *pl = (szh_ompb_place *)(extra.data() + o_place);
        for (int u = 0; u < ns; ++u) if (lut_item[u] >= 0) memcpy(extra.data() + o_str[u], ps[u].D.dtab.data(), ps[u].D.dtab.size() * 4);
        for (int i : tab.list[OMPB_L_ENT]) {
            ompbr_item<T> &e = it[i];
            const int u = e.slot;
            const omp_stream<T> &p = ps[u];
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
            r.n_nodes = p.D.n_nodes; r.tab_lds = hl.tab_lds(p.D.n_nodes);
            // the sweep form: the single region call's rule (omp_dec::sweep) on the sub-geometry and the staging array
            const int form = omp_form(e.gs, stage, sizeof(T), (size_t)e.gs.d0, (size_t)e.gs.d1);
            items[i].quant_kernel = form; items[i].intervals = p.intervals; items[i].n_unpred = e.Ec; items[i].batched = 1;
            tab.geo[i].g = e.gs; tab.geo[i].fw = e.fw;
            tab.list[ompb_form_list(false, form)].push_back(i);
            if (form == 3 && e.Ec > 0) {
                tab.list[OMPB_L_PACKD].push_back(i);           // (here: the items k_omp_scatter runs for)
                if (e.fw > 0) { r.vflags = (unsigned *)ctx->chunk_bits.p + e.o_flag; any_flags = true; }
            }
            if (stream_on_device) for (const auto &pc : e.pieces) if (pc.len) { *sp++ = (u64)(uintptr_t)(items[i].stream + pc.src); *sp++ = (u64)pc.dst; *sp++ = (u64)pc.len; }
            // the placement: out of the staging array -- the region starts inside its first covered box -- into the destination, or (a host destination) contiguous
            // into the context's buffer, out of which its rows are copied
            szh_ompb_place &q = pl[i];
            q.src = stage + e.lo_off;
            q.s0 = e.gs.d0; q.s1 = e.gs.d1;
            if (out_on_device) { q.dst = items[i].out; q.d0 = (int64_t)e.p0; q.d1 = (int64_t)e.p1; }
            else { q.dst = (char *)ctx->codes_blk.p + e.o_dst; q.d0 = (int64_t)(e.ext[1] * e.ext[2]); q.d1 = (int64_t)e.ext[2]; }
            q.e0 = (int)e.ext[0]; q.e1 = (int)e.ext[1]; q.e2 = (int)e.ext[2];
            q.ppr = 1 + (int)((e.ext[2] + 16 / sizeof(T) - 1) / (16 / sizeof(T)));
            q.err = tab.totals(i) + 2;
            most_pieces = std::max(most_pieces, e.ext[0] * e.ext[1] * (size_t)q.ppr);
            S.n_elements += (uint64_t)e.n_out; S.n_blocks += (uint64_t)e.nbc; S.n_unpred += e.Ec;
        }
        return SZHIP_OK;
    }
    // ---- 4. one upload of the table; the covered boxes' first values, verbatim values and payloads: one pinned blob and one upload (host streams), or one gather
    // launch over all items' spans (device streams).  5. the look-up tables (one per distinct stream), the Huffman decode of all covered boxes.  6. the sweeps into the
    // staging arrays (as szhip_decompress_omp_batch_shapes).  7. ONE placing launch: every item whose boxes all decoded (the sweeps' counts are read on the device: no
    // synchronisation in front of it)
    int launches() {
        if (n_ent == 0) { HIPCHK(hipStreamSynchronize(st)); return SZHIP_OK; }
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
            for (int i : tab.list[OMPB_L_ENT]) for (const auto &pc : it[i].pieces) memcpy(hb + pc.dst, items[i].stream + pc.src, pc.len);
            HIPCHK(hipMemcpyAsync(d_data, hb, data_len + 64, hipMemcpyHostToDevice, st));
        }
        hipLaunchKernelGGL(k_ompb_build_lut, dim3(SZH_LUT_SIZE / 256, (unsigned)n_lut), dim3(256), 0, st, tab.d_rec(), tab.d_list(OMPB_L_ALL));
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ompbs_hdec_lut, dim3((unsigned)ompb_most_boxes(tab.list[OMPB_L_ENT], 0, n_ent, ish), (unsigned)n_ent), dim3(256), hl.lds_lut, st, tab.d_rec(), tab.d_geo(),
                           tab.d_list(OMPB_L_ENT), (unsigned)hl.stage_max);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[1], st));
        HIPCHK(hipEventRecord(ctx->ev[2], st));
        const int nsc = (int)tab.list[OMPB_L_PACKD].size();
        if (nsc) hipLaunchKernelGGL((k_ompbs_scatter<T>), dim3((unsigned)ompb_most_boxes(tab.list[OMPB_L_PACKD], 0, nsc, ish), (unsigned)nsc), dim3(256), 0, st, tab.d_rec(), tab.d_geo(),
                                    tab.d_list(OMPB_L_PACKD));
        S.quant_kernel_launches += ompb_sweep_mixed<T, true>(st, tab, ish, box_runs);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[3], st));
        S.quant_kernel = items[tab.list[OMPB_L_ENT][0]].quant_kernel;
        hipLaunchKernelGGL((k_ompbr_place<T>), dim3((unsigned)((most_pieces + 255) / 256), (unsigned)n_ent), dim3(256), 0, st,
                           (const szh_ompb_place *)(tab.dev() + tab.o_extra + o_place), tab.d_list(OMPB_L_ENT));
        HIPCHK(hipGetLastError());
        ++S.packing;
        // 8. the items' error counts; host destinations: one copy down, then the rows of the items that decoded
        const u64 *h_tot = nullptr;
        TRY(ompb_read_totals(*this, tab, &h_tot));
        for (int i : tab.list[OMPB_L_ENT])
            if ((unsigned)h_tot[4 * (size_t)i + 2] != 0) {
                state[i] = OMPB_FAILED; items[i].rc = SZHIP_ERR_STREAM;
                snprintf(ctx->err, sizeof(ctx->err), "stream %d of the batch: boxes of the region whose payload or verbatim-value count does not fit their codes", i);
            }
        if (!out_on_device) {
            std::vector<unsigned char> tmp(dst_bytes);
            TRY(staged_copy(ctx, tmp.data(), ctx->codes_blk.p, tmp.size(), false));
            for (int i : tab.list[OMPB_L_ENT]) {
                if (state[i] != OMPB_BATCH) continue;
                const ompbr_item<T> &e = it[i];
                const host_view hv = {e.ext[1], e.ext[2] * sizeof(T), e.p0 * sizeof(T), e.p1 * sizeof(T)};
                host_view_move(hv, (char *)items[i].out, (char *)tmp.data() + e.o_dst, 0, e.n_out * sizeof(T), false);
            }
        }
        return SZHIP_OK;
    }
    // ---- the items the shared launches do not cover: the single region call; a view is placed behind it (szhip_scatter_view on the device, its rows on the host)
    int finish(szhip_stats *stats) {
        for (int i = 0; i < count; ++i) {
            if (state[i] != OMPB_SINGLE) continue;
            const ompbr_item<T> &e = it[i];
            const ompb_shape &s = sh[e.slot];
            const szhip_batch_item &m = items[i];
            szhip_stats s1; memset(&s1, 0, sizeof(s1));
            const bool contiguous = e.p1 == e.ext[2] && e.p0 == e.ext[1] * e.ext[2];
            auto decode = [&](void *dst, int on_device) { return decompress_omp_region_impl<T>(ctx, m.stream, stream_on_device, m.stream_len, m.body_off, s.r0, s.r1, s.r2, regions[i].lo, regions[i].hi, dst, on_device, &s1); };
            int rc;
            if (contiguous) rc = decode(m.out, out_on_device);
            else if (out_on_device) {                            // a view on the device: decoded contiguous into the context's input buffer, scattered from there
                rc = ensure(ctx, ctx->in, e.n_out * sizeof(T));
                if (rc == SZHIP_OK) rc = decode(ctx->in.p, 1);
                if (rc == SZHIP_OK) rc = scatter_view_impl<T>(ctx, ctx->in.p, e.ext[0], e.ext[1], e.ext[2], m.out, 1, e.p0, e.p1);
            } else {                                             // a view on the host: decoded into a contiguous host array, its rows moved from there
                std::vector<T> tmp(e.n_out);
                rc = decode(tmp.data(), 0);
                if (rc == SZHIP_OK) host_view_move({e.ext[1], e.ext[2] * sizeof(T), e.p0 * sizeof(T), e.p1 * sizeof(T)}, (char *)m.out, (char *)tmp.data(), 0, e.n_out * sizeof(T), false);
            }
            items[i].rc = rc; items[i].batched = 0;
            if (rc != SZHIP_OK) { hipStreamSynchronize(st); continue; }
            items[i].intervals = s1.intervals; items[i].n_unpred = s1.n_unpred; items[i].quant_kernel = s1.quant_kernel;
            regions[i].n_boxes = s1.n_blocks;
            S.n_elements += s1.n_elements; S.n_blocks += s1.n_blocks; S.n_unpred += s1.n_unpred;
        }
        int rc_all = SZHIP_OK;                                  // the first failed item's code; the statistics
        for (int i = 0; i < count; ++i) if (items[i].rc != SZHIP_OK && rc_all == SZHIP_OK) rc_all = items[i].rc;
        S.out_bytes = S.n_elements * sizeof(T);
        S.ms_host = host_ms; S.ms_total = now_ms() - t_begin;
        if (stats) *stats = S;
        return rc_all;
    }
};

template <class T>
int decompress_omp_batch_region_impl(szhip_ctx *ctx, szhip_batch_item *items, const szhip_batch_shape *shapes, szhip_batch_region *regions, int count, int stream_on_device,
                                     int out_on_device, szhip_stats *stats)
{
    ompbr_call<T> c{call_base(ctx), items, shapes, regions, count, stream_on_device, out_on_device};
    TRY(c.read_fronts());
    TRY(c.cover_regions());
    TRY(c.fill_table());
    TRY(c.launches());
    return c.finish(stats);
}
