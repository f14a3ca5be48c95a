// szhip_omp.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace): the reference's OpenMP container.
// =====================================================================================================================
// The reference's OpenMP container for 3-D arrays (szh_omp.h; sz/src/sz_omp.c:63-358, inverse :366-566).  The stream's layout and every rule of the format that
// the batch calls share with the calls below: szhip_omprules.inc.
// =====================================================================================================================
static int omp_box_grid(szhip_ctx *ctx, int thread_num, size_t r0, size_t r1, size_t r2, szh_omp_geom *g)
{
    if (thread_num < 1) FAIL(SZHIP_ERR_ARG, "thread_num %d", thread_num);
    // sz_omp.c:88-117: the exponent of two is spread over the three dimensions, dim 0 first; the rest of thread_num goes to dim 2
    int order = 0; while ((2 << order) <= thread_num) ++order;
    const int bb = order / 3;
    size_t nx, ny;
    switch (order % 3) { case 0: nx = (size_t)1 << bb; ny = (size_t)1 << bb; break; case 1: nx = (size_t)1 << (bb + 1); ny = (size_t)1 << bb; break; default: nx = (size_t)1 << (bb + 1); ny = (size_t)1 << (bb + 1); }
    const size_t nz = (size_t)thread_num / (nx * ny);
    if (r0 == 0 || r1 == 0 || r2 == 0 || r0 * r1 * r2 >= ((size_t)1 << 40)) FAIL(SZHIP_ERR_UNSUP, "OpenMP container: a 3-D array is needed");
    if (r0 % nx || r1 % ny || r2 % nz)
        FAIL(SZHIP_ERR_UNSUP, "OpenMP container: the %zu x %zu x %zu box grid of thread_num %d does not divide %zu x %zu x %zu (on an uneven grid the "
             "reference's code book depends on uninitialised memory)", nx, ny, nz, thread_num, r0, r1, r2);
    g->nx = (int)nx; g->ny = (int)ny; g->nz = (int)nz;
    g->c0 = (int)(r0 / nx); g->c1 = (int)(r1 / ny); g->c2 = (int)(r2 / nz);
    g->d0 = (int64_t)(r1 * r2); g->d1 = (int64_t)r2;
    g->nb = (int)(nx * ny * nz);
    const size_t bel = (size_t)g->c0 * g->c1 * g->c2;
    if ((size_t)g->c0 * g->c1 > SZH_OMP_MAX_ROWS || bel >= OMP_BOX_LIMIT)
        FAIL(SZHIP_ERR_UNSUP, "OpenMP container: a box face of %d x %d rows (at most %d; raise thread_num)", g->c0, g->c1, SZH_OMP_MAX_ROWS);
    g->bel = (int)bel;
    g->cpb = (int)((bel + SZH_ENC_CHUNK - 1) / SZH_ENC_CHUNK);
    g->vec = (g->c2 % 4 == 0 && r2 % 4 == 0) ? 1 : 0;          // (the base address is looked at by the caller)
    g->tile8 = (g->c0 % 8 == 0 && g->c1 % 8 == 0) ? 1 : 0;
    g->pitch = g->c1;
    if (g->tile8) while (g->pitch % 16 != 8) ++g->pitch;       // 8 or 24 modulo 32
    return SZHIP_OK;
}

// the column-per-lane sweep of szh_ompcol.h serves 32 x 32 box faces (any number of planes), two boxes to a wavefront, rows read 16 bytes at a time
static bool omp_col_applies(const szh_omp_geom &g, const void *base, size_t row_pitch_bytes, size_t plane_pitch_bytes)
{
    return g.c1 == 32 && g.c2 == 32 && g.nb % 2 == 0 && ((uintptr_t)base & 15u) == 0 && row_pitch_bytes % 16 == 0 && plane_pitch_bytes % 16 == 0;
}
// A VIEW (szhip_compress_omp_view / szhip_decompress_omp_view): the boxes of `g` lie in an array whose planes are pitch0 and whose rows pitch1 elements apart.  The
// sweeps, the encoders' reads of verbatim values and k_omp_scatter address the array through g.d0 / g.d1; rows may be taken 16 bytes at a time only where every row
// of every plane starts on such a boundary (the base address is looked at by the caller, as for a contiguous array)
static void omp_view_pitches(szh_omp_geom *g, size_t pitch0, size_t pitch1, size_t elem)
{
    g->d0 = (int64_t)pitch0; g->d1 = (int64_t)pitch1;
    g->vec = (g->c2 % 4 == 0 && pitch1 * elem % 16 == 0 && pitch0 * elem % 16 == 0) ? 1 : 0;
}

// ---- views (szhip.h): what szhip_pack_view / szhip_scatter_view and the host-view form of szhip_compress_omp_view run
// the gather (k_omp_crop, or the rows of a host view through the staging buffers) into `d_dst`, n0 x r1 x r2 values, contiguous
template <class T>
int pack_view_impl(szhip_ctx *ctx, const void *data, int data_on_device, size_t n0, size_t r1, size_t r2, size_t pitch0, size_t pitch1, void *d_dst)
{
    const size_t n = n0 * r1 * r2;
    if (!data_on_device) {
        const host_view hv = {r1, r2 * sizeof(T), pitch0 * sizeof(T), pitch1 * sizeof(T)};
        return staged_copy(ctx, d_dst, data, n * sizeof(T), true, &hv);
    }
    const int cpr = (int)((r2 + 16 / sizeof(T) - 1) / (16 / sizeof(T)));
    const int64_t total = (int64_t)(n0 * r1) * cpr;
    hipLaunchKernelGGL((k_omp_crop<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, (const T *)data, (int64_t)pitch0, (int64_t)pitch1, (T *)d_dst, (int)r1, (int)r2, cpr, total);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SZHIP_OK;
}
template <class T>
int scatter_view_impl(szhip_ctx *ctx, const void *d_packed, size_t n0, size_t r1, size_t r2, void *out, int out_on_device, size_t pitch0, size_t pitch1)
{
    if (!out_on_device) {
        const host_view hv = {r1, r2 * sizeof(T), pitch0 * sizeof(T), pitch1 * sizeof(T)};
        return staged_copy(ctx, out, d_packed, n0 * r1 * r2 * sizeof(T), false, &hv);
    }
    const int ppr = 1 + (int)((r2 + 16 / sizeof(T) - 1) / (16 / sizeof(T)));
    const int64_t total = (int64_t)(n0 * r1) * ppr;
    hipLaunchKernelGGL((k_view_scatter<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, (const T *)d_packed, (T *)out, (int64_t)pitch0, (int64_t)pitch1, (int)r1, (int)r2, ppr, total);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SZHIP_OK;
}
// A device view that misses the 16-byte conditions while a packed copy of it would take the column form: value by value it costs 4.3 x (compress) / 2.7 x (decode) the
// packing pass plus the column sweep (512^3 float32, DESIGN 4.5.2), so such a view is gathered into / decoded in the context's contiguous buffer.  Same stream, same values.
// (`g`: the grid of the sub-box.)  Shapes whose packed copy takes k_omp_box either way run where they lie: that pair was not measured.
static bool omp_view_packs(const szh_omp_geom &g, const void *base, size_t pitch0, size_t pitch1, size_t elem)
{
    const bool aligned = ((uintptr_t)base & 15u) == 0 && pitch1 * elem % 16 == 0 && pitch0 * elem % 16 == 0;
    return !aligned && g.c1 == 32 && g.c2 == 32 && g.nb % 2 == 0;
}

// One compress call into the OpenMP container: its state, and one member function per phase (compress_omp_impl is their sequence).
template <class T>
struct omp_call : call_base {
    // ---- arguments, geometry
    const szhip_params *const prm; const unsigned char *const meta; const size_t meta_len;
    const int out_on_device; unsigned char **const out; size_t *const out_size;
    const T eb;                                                // `float realPrecision` of sz_omp.c:63 (double: :578)
    szh_omp_geom g; const szh_geom3 G; const size_t row_bytes, plane_bytes; const int64_t n = G.n;      // (`G`: the box of values, contiguous; `g`, the pitches in bytes: the array they lie in)
    // ---- device arrays
    const T *d_in = nullptr; u64 *sm = nullptr; uint16_t *d_codes = nullptr; unsigned char *d_stream = nullptr;
    unsigned *d_ucount = nullptr, *d_hist_box = nullptr; T *d_first = nullptr; u64 *d_ucount64 = nullptr, *d_uoff = nullptr, *d_box_bytes = nullptr, *d_box_off = nullptr;
    // ---- decisions
    unsigned intervals = 0; bool box_hist = false, sweep_counted = true;
    // ---- the code book and the stream's layout
    std::vector<u64> tab_code; std::vector<uint8_t> tab_len; unsigned maxlen = 0; u64 total_bits = 0, E = 0;
    std::vector<unsigned char> hdr;
    omp_layout<T> L{0, 0, 0, 0, 0};

    // ---- the array staged; interval count (sz_omp.c:73-82: optimize_intervals_float_3D_opt over the whole array when it is not fixed)
    int choose_intervals(const void *data, int data_on_device) {
        S.n_elements = (uint64_t)n; S.n_blocks = (uint64_t)g.nb;
        TRY(stage_input(ctx, data, data_on_device, (size_t)n, &d_in));
        if ((uintptr_t)d_in & 15u) g.vec = 0;
        TRY(clear_small(ctx, &sm));
        HIPCHK(hipEventRecord(ctx->ev[0], st));
        intervals = prm->quantization_intervals;
        if (intervals == 0) TRY(sampled_intervals<T>(ctx, G, false, d_in, prm, eb, sm, &intervals, &host_ms, g.d0, g.d1));
        if (intervals > 65536 || intervals < 4) FAIL(SZHIP_ERR_UNSUP, "quantization interval count %u outside [4,65536]", intervals);
        S.intervals = intervals;
        HIPCHK(hipEventRecord(ctx->ev[1], st));
        return SZHIP_OK;
    }
    // ---- the boxes: predict + quantise
    int quantise() {
        TRY(ensure(ctx, ctx->codes_nat, (size_t)n * 2 + 64));
        d_codes = (uint16_t *)ctx->codes_nat.p;
        TRY(ensure(ctx, ctx->zcnt, (size_t)g.nb * 4));
        TRY(ensure(ctx, ctx->samples, (size_t)g.nb * sizeof(T)));
        TRY(ensure(ctx, ctx->col_zeros64, (size_t)g.nb * 8)); TRY(ensure(ctx, ctx->col_off, (size_t)g.nb * 8 + 8));
        d_ucount = (unsigned *)ctx->zcnt.p; d_first = (T *)ctx->samples.p;
        d_ucount64 = (u64 *)ctx->col_zeros64.p; d_uoff = (u64 *)ctx->col_off.p;
        const int rows = g.c0 * g.c1, box_threads = rows;      // one lane per row
        box_hist = omp_box_hist_book(intervals, (size_t)g.nb) && omp_box_hist_shape(g.bel);
        HIPCHK(hipEventRecord(ctx->ev[2], st));
        if (omp_col_applies(g, d_in, row_bytes, plane_bytes)) {             // the column-per-lane sweep (szh_ompcol.h): a wavefront per pair of boxes
            szh_oc::sweep_args<T> oa;
            oa.g = g; oa.data = d_in; oa.out = nullptr; oa.eb = eb; oa.recip = (T)(1 / eb); oa.intervals = (int)intervals; oa.codes = d_codes;
            oa.ucount = d_ucount; oa.ucount64 = d_ucount64; oa.first = d_first; oa.uoff = nullptr; oa.vflags = nullptr; oa.fw = 0;
            // (with a histogram per box coming anyway, the boxes' counts of verbatim values are its bins 0: the sweep leaves the counting out --
            //  two vector instructions per step of a kernel that is bound by exactly those)
            if (box_hist) { sweep_counted = false; hipLaunchKernelGGL((k_omp_col<T, 32, 32, false, false>), dim3((unsigned)(g.nb / 2)), dim3(64), 0, st, oa); }
            else hipLaunchKernelGGL((k_omp_col<T, 32, 32, false, true>), dim3((unsigned)(g.nb / 2)), dim3(64), 0, st, oa);
        } else hipLaunchKernelGGL((g.vec ? k_omp_box<T, false, true> : k_omp_box<T, false, false>), dim3((unsigned)g.nb), dim3((unsigned)box_threads), (size_t)4 * g.c0 * g.pitch * sizeof(T), st, g, d_in,
                                  (T *)nullptr, eb, (T)(1 / eb), (int)intervals, d_codes, d_ucount, d_ucount64, d_first, (const T *)nullptr, (const u64 *)nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[3], st));
        S.quant_kernel_launches = 1;
        S.quant_kernel = omp_col_applies(g, d_in, row_bytes, plane_bytes) ? 3 : (g.vec ? 4 : 5);      // (szhip.h: which form the address and the box shape allowed)
        return SZHIP_OK;
    }
    // ---- ONE histogram over all boxes -> code book (host); the ranks of the boxes' verbatim values meanwhile.  Small alphabets: a
    // histogram per box on the way (k_omp_hist_box), from which the boxes' payload sizes follow without another pass over the codes.
    // Then the container: everything up to the payloads has a known size; the payloads take at most a byte of padding per box
    int hist_and_book() {
        TRY(ensure(ctx, ctx->hist, (size_t)(65536 + 8192) * 4 + 64));
        unsigned *d_hist = (unsigned *)ctx->hist.p;
        TRY(ensure_pinned(ctx, (size_t)intervals * 4 + 64));
        unsigned *h_hist = (unsigned *)ctx->pinned;
        HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)intervals * 4, st));
        if (box_hist) {
            TRY(ensure(ctx, ctx->chunk_bits, (size_t)g.nb * intervals * 4));
            d_hist_box = (unsigned *)ctx->chunk_bits.p;
            const int rshift = omp_hist_rshift(intervals, g.bel), hist_per_wg = omp_hist_per_wg(g.bel);
            hipLaunchKernelGGL(k_omp_hist_box, dim3((unsigned)((g.nb + hist_per_wg - 1) / hist_per_wg)), dim3(256), ((size_t)intervals << rshift) * 4, st, g.bel, (const uint16_t *)d_codes, intervals, rshift,
                               d_hist_box, d_hist, sweep_counted ? (unsigned *)nullptr : d_ucount, sweep_counted ? (u64 *)nullptr : d_ucount64, g.nb, hist_per_wg);
            HIPCHK(hipGetLastError());
        } else
            TRY(launch_hist_u16(ctx, st, d_codes, 0, n, intervals, d_hist));
        HIPCHK(hipMemcpyAsync(h_hist, d_hist, (size_t)intervals * 4, hipMemcpyDeviceToHost, st));
        if (!box_hist) TRY(scan_u64(ctx, (const u64 *)d_ucount64, g.nb, d_uoff, sm + SM_TOTAL_UNPRED));      // (with per-box histograms: in k_omp_layout, below)
        HIPCHK(hipStreamSynchronize(st));
        E = h_hist[0];
        S.n_unpred = E;
        const double h0 = now_ms();
        const huff_ptr hf = host_book(h_hist, intervals, tab_code, tab_len, &maxlen);
        if (!hf) FAIL(SZHIP_ERR_INTERNAL, "Huffman build failed");
        const size_t tree_bytes = szhost_huff_tree_size(hf.get());
        total_bits = hf->total_bits;
        L = omp_layout<T>(meta_len, (size_t)g.nb, E, tree_bytes, total_bits);
        hdr.assign(L.hdr_len, 0);
        omp_write_header<T>(hdr.data(), meta, meta_len, (size_t)g.nb, eb, intervals, hf.get(), tree_bytes);
        host_ms += now_ms() - h0;
        return SZHIP_OK;
    }
    // ---- packing: the boxes' payloads and every table of the stream into the stream buffer
    int pack() {
        TRY(ensure(ctx, ctx->stream_buf, L.cap_len + 64));
        d_stream = (unsigned char *)ctx->stream_buf.p;
        HIPCHK(hipMemsetAsync(d_stream, 0, L.cap_len + 64, st));
        TRY(ensure(ctx, ctx->reg_flags, (size_t)g.nb * 8)); TRY(ensure(ctx, ctx->reg_rank, (size_t)g.nb * 8));
        d_box_bytes = (u64 *)ctx->reg_flags.p; d_box_off = (u64 *)ctx->reg_rank.p;
        const size_t lds3 = omp_fast_lds3(intervals, maxlen);
        const bool fast = box_hist && intervals <= 2048 && omp_fast_packs(maxlen, lds3);      // (`intervals <= 2048`: this call's own; box_hist has asked for 1024 already)
        return fast ? pack_fast(lds3) : pack_general();
    }
    // the usual case (code words of at most 32 bits, a histogram per box): ONE upload -- the header and the packed code table
    // `code << 8 | len` --, one launch for the boxes' sizes and places (k_omp_layout), one that packs the codes and writes every table
    // of the stream itself (k_omp_encode_box3).  (Round 4, first form: 8 copies / fills and 8 small launches here, ~0.1 ms of gaps.)
    int pack_fast(size_t lds3) {
        const size_t hdr_pad = (L.hdr_len + 7) / 8 * 8, blob = hdr_pad + (size_t)intervals * 8;
        TRY(ensure_pinned3(ctx, blob));
        unsigned char *hb = (unsigned char *)ctx->pinned3;
        memcpy(hb, hdr.data(), L.hdr_len);
        u64 *hp = (u64 *)(hb + hdr_pad);
        omp_packed_table(tab_code, tab_len, intervals, hp);
        TRY(ensure(ctx, ctx->code_tab, blob));
        TRY(ensure(ctx, ctx->unpred, (size_t)E * sizeof(T) + 16));
        HIPCHK(hipMemcpyAsync(ctx->code_tab.p, hb, blob, hipMemcpyHostToDevice, st));
        const u64 *d_packed = (const u64 *)((const unsigned char *)ctx->code_tab.p + hdr_pad);
        const int many = g.nb > tune_int("SZ_HIP_OMP_MANY", 8192);     // (one workgroup reading every box's histogram: 0.22 ms for 32 768 boxes)
        if (many) hipLaunchKernelGGL(k_omp_box_bits_p, dim3((unsigned)((g.nb + 3) / 4)), dim3(256), 0, st, g.nb, intervals, (const unsigned *)d_hist_box, d_packed, d_box_bytes);
        hipLaunchKernelGGL(k_omp_layout, dim3(1), dim3(1024), 0, st, g.nb, intervals, (const unsigned *)d_hist_box, d_packed, (const u64 *)d_ucount64, d_box_bytes, d_box_off, d_uoff,
                           sm + SM_SCRATCH, sm + SM_TOTAL_UNPRED, many);
        HIPCHK(hipGetLastError());
        szh_omp_tables tb;
        tb.stream = d_stream; tb.hdr = (const unsigned char *)ctx->code_tab.p; tb.hdr_len = (unsigned)L.hdr_len;
        tb.off_ucount = L.off_ucount; tb.off_first = L.off_first; tb.off_unpred = L.off_unpred; tb.off_sizes = L.off_sizes; tb.first = d_first;
        hipLaunchKernelGGL((k_omp_encode_box3<T>), dim3((unsigned)g.nb), dim3(256), lds3, st, g, d_in, (const uint16_t *)d_codes, d_packed, intervals, maxlen, (const u64 *)d_box_off,
                           (const u64 *)d_box_bytes, (const u64 *)d_uoff, (const unsigned *)d_ucount, (u64)L.off_pay * 8, (unsigned *)d_stream,
                           (T *)ctx->unpred.p, (unsigned *)(sm + SM_ERR), tb);
        HIPCHK(hipGetLastError());
        // (the verbatim values go through an aligned buffer: their table lies at whatever byte offset the tree's size gives it, and byte
        //  stores from the kernel were half of its 0.1 ms for them)
        if (E > 0) HIPCHK(hipMemcpyAsync(d_stream + L.off_unpred, ctx->unpred.p, (size_t)E * sizeof(T), hipMemcpyDeviceToDevice, st));
        return SZHIP_OK;
    }
    // the first form: tables copied one by one; the boxes' payload sizes (from their histograms, or one more pass over the codes), their places, then
    // ONE pass that packs every box's codes behind a running bit position and drops its verbatim values into the table on the way
    int pack_general() {
        TRY(upload_code_tables(ctx, tab_code, tab_len));
        HIPCHK(hipMemcpyAsync(d_stream, hdr.data(), L.hdr_len, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_stream + L.off_ucount, d_ucount, (size_t)g.nb * 4, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(d_stream + L.off_first, d_first, (size_t)g.nb * sizeof(T), hipMemcpyDeviceToDevice, st));
        if (box_hist) TRY(scan_u64(ctx, (const u64 *)d_ucount64, g.nb, d_uoff, sm + SM_TOTAL_UNPRED));
        TRY(ensure(ctx, ctx->unpred, (size_t)E * sizeof(T) + 16));
        if (box_hist) hipLaunchKernelGGL(k_omp_box_bits_h, dim3((unsigned)((g.nb + 3) / 4)), dim3(256), 0, st, g.nb, intervals, (const unsigned *)d_hist_box, (const uint8_t *)ctx->len_tab.p, d_box_bytes);
        else hipLaunchKernelGGL(k_omp_box_bits_c, dim3((unsigned)g.nb), dim3(256), 0, st, g.bel, (const uint16_t *)d_codes, (const uint8_t *)ctx->len_tab.p, d_box_bytes);
        HIPCHK(hipGetLastError());
        TRY(scan_u64(ctx, (const u64 *)d_box_bytes, g.nb, d_box_off, sm + SM_SCRATCH));
        HIPCHK(hipMemcpyAsync(d_stream + L.off_sizes, d_box_bytes, (size_t)g.nb * 8, hipMemcpyDeviceToDevice, st));
        const bool tab_lds = intervals <= 2048;                  // the code table in LDS when it fits
        hipLaunchKernelGGL((tab_lds ? k_omp_encode_box<T, true> : k_omp_encode_box<T, false>), dim3((unsigned)g.nb), dim3(256), (tab_lds ? (size_t)intervals * 9 : 0) + 16, st, g, d_in, (const uint16_t *)d_codes,
                           (const u64 *)ctx->code_tab.p, (const uint8_t *)ctx->len_tab.p, intervals, (const u64 *)d_box_off, (const u64 *)d_box_bytes, (const u64 *)d_uoff, (const unsigned *)d_ucount, (u64)L.off_pay * 8,
                           (unsigned *)d_stream, (T *)ctx->unpred.p, (unsigned *)(sm + SM_ERR));
        HIPCHK(hipGetLastError());
        if (E > 0) HIPCHK(hipMemcpyAsync(d_stream + L.off_unpred, ctx->unpred.p, (size_t)E * sizeof(T), hipMemcpyDeviceToDevice, st));
        return SZHIP_OK;
    }
    // ---- the end of the entropy stage; the device's counts against the book's, delivery, the statistics
    int check_and_deliver() {
        HIPCHK(hipEventRecord(ctx->ev[4], st));
        u64 h_small[SM_COUNT];
        HIPCHK(hipMemcpyAsync(h_small, sm, SM_COUNT * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!omp_totals_ok(h_small[SM_TOTAL_UNPRED], h_small[SM_ERR], h_small[SM_SCRATCH], E, total_bits, (size_t)g.nb))
            FAIL(SZHIP_ERR_INTERNAL, "OpenMP container: entropy stage mismatch");
        const size_t total_len = L.off_pay + (size_t)h_small[SM_SCRATCH];
        if (total_len > L.cap_len) FAIL(SZHIP_ERR_INTERNAL, "OpenMP container: payloads larger than their bound");
        TRY(deliver_stream(ctx, d_stream, total_len, out_on_device, out, out_size, false, true));
        if (!out_on_device && hipStreamSynchronize(st) != hipSuccess) FAIL_PUBLISHED(SZHIP_ERR_NODEVICE, "copying the stream to the host failed");
        compress_times(ctx, S, host_ms, t_begin, total_len);
        return SZHIP_OK;
    }
};

template <class T>
int compress_omp_impl(szhip_ctx *ctx, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1, double eb_in, int thread_num,
                      const szhip_params *prm, const unsigned char *meta, size_t meta_len, int out_on_device, unsigned char **out, size_t *out_size,
                      szhip_stats *stats)
{
    szh_omp_geom g;
    TRY(omp_box_grid(ctx, thread_num, r0, r1, r2, &g));
    if (!((T)eb_in > 0)) FAIL(SZHIP_ERR_ARG, "error bound %g", eb_in);
    if ((pitch1 != r2 || pitch0 != r1 * r2) && omp_view_packs(g, data, pitch0, pitch1, sizeof(T))) {      // (a view on the device; one on the host was packed by the caller)
        TRY(ensure(ctx, ctx->in, r0 * r1 * r2 * sizeof(T)));
        TRY(pack_view_impl<T>(ctx, data, 1, r0, r1, r2, pitch0, pitch1, ctx->in.p));
        data = ctx->in.p; pitch0 = r1 * r2; pitch1 = r2;
    }
    if (pitch1 != r2 || pitch0 != r1 * r2) omp_view_pitches(&g, pitch0, pitch1, sizeof(T));
    omp_call<T> c{call_base(ctx), prm, meta, meta_len, out_on_device, out, out_size, (T)eb_in, g, szh_make_geom3((int)r0, (int)r1, (int)r2), pitch1 * sizeof(T), pitch0 * sizeof(T)};
    TRY(c.choose_intervals(data, data_on_device));
    TRY(c.quantise());
    TRY(c.hist_and_book());
    TRY(c.pack());
    TRY(c.check_and_deliver());
    return c.done(stats);
}

// One decompress call of the OpenMP container.  `body_off`: offset of the thread_num field (4 + MetaDataByteLength: what decompressDataSeries_*_3D_openmp is handed)
template <class T>
struct omp_dec : call_base {
    // ---- arguments
    const size_t stream_len, body_off, r0, r1, r2; void *const out; const int out_on_device;
    stream_intake in;
    bool packed = false;
    size_t pitch0 = 0, pitch1 = 0;                             // a view (szhip_decompress_omp_view): the element pitches of the array `out` lies in; 0: contiguous
    // ---- the header and the tables behind it
    omp_stream<T> s;
    szh_omp_geom g; int64_t n = 0; u64 E = 0;                   // (`g`, `E`: of the boxes the sweep runs over -- a region call's are its sub-grid's)
    // ---- device arrays
    u64 *sm = nullptr; uint16_t *d_codes = nullptr; T *d_out = nullptr;
    const u64 *d_uoff = nullptr; const T *d_first = nullptr, *d_unpred = nullptr;      // per box: ranks of its verbatim values, its first value; the verbatim values

    // ---- the stream taken in; the fixed fields, the box grid, the tree, the boxes' counts of verbatim values and payload sizes: on the host
    int read_header() {
        const char *why;
        TRY(in.open());
        if ((why = s.begin(body_off, stream_len))) FAIL(SZHIP_ERR_STREAM, "%s", why);
        TRY(in.fetch(s.fixed));
        if ((why = s.read_fixed(in.hs))) FAIL(SZHIP_ERR_STREAM, "%s", why);
        TRY(omp_box_grid(ctx, s.thread_num, r0, r1, r2, &g));
        if (g.nb != s.thread_num) FAIL(SZHIP_ERR_STREAM, "thread_num %d is not a box grid", s.thread_num);
        n = (int64_t)r0 * r1 * r2;
        S.n_elements = (uint64_t)n; S.n_blocks = (uint64_t)g.nb; S.intervals = s.intervals;
        if ((why = s.place_tables(g))) FAIL(SZHIP_ERR_STREAM, "%s", why);
        TRY(in.fetch(s.off_unpred));
        if ((why = s.read_tree_and_counts(in.hs, g))) FAIL(SZHIP_ERR_STREAM, "%s", why);
        E = s.E;
        S.n_unpred = E;
        u64 *sizes = s.size_table(g);
        if (in.on_device) { HIPCHK(hipMemcpyAsync(sizes, in.d_stream + s.off_sizes, (size_t)g.nb * 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st)); }
        else memcpy(sizes, in.stream_in + s.off_sizes, (size_t)g.nb * 8);
        if ((why = s.walk_sizes())) FAIL(SZHIP_ERR_STREAM, "%s", why);
        return SZHIP_OK;
    }
    // ---- device tables: payload offsets / sizes, ranks of the verbatim values, first values and verbatim values at aligned addresses; then the Huffman decode,
    // a workgroup per box
    int decode_boxes() {
        TRY(clear_small(ctx, &sm));
        TRY(ensure(ctx, ctx->reg_flags, (size_t)g.nb * 8)); TRY(ensure(ctx, ctx->reg_rank, (size_t)g.nb * 8)); TRY(ensure(ctx, ctx->col_off, (size_t)g.nb * 8 + 8));
        TRY(ensure(ctx, ctx->samples, (size_t)g.nb * sizeof(T))); TRY(ensure(ctx, ctx->unpred, (size_t)E * sizeof(T) + 16));
        TRY(ensure(ctx, ctx->dec_tab, up64(s.D.dtab.size() * 4) + SZH_LUT_BYTES + 16));
        HIPCHK(hipMemcpyAsync(ctx->reg_flags.p, s.bbytes.data(), (size_t)g.nb * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->reg_rank.p, s.boff.data(), (size_t)g.nb * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->col_off.p, s.uoff.data(), ((size_t)g.nb + 1) * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->dec_tab.p, s.D.dtab.data(), s.D.dtab.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->samples.p, in.d_stream + s.off_first, (size_t)g.nb * sizeof(T), hipMemcpyDeviceToDevice, st));
        if (E > 0) HIPCHK(hipMemcpyAsync(ctx->unpred.p, in.d_stream + s.off_unpred, (size_t)E * sizeof(T), hipMemcpyDeviceToDevice, st));
        d_uoff = (const u64 *)ctx->col_off.p; d_first = (const T *)ctx->samples.p; d_unpred = (const T *)ctx->unpred.p;
        TRY(ensure(ctx, ctx->codes_nat, (size_t)n * 2 + 64));
        d_codes = (uint16_t *)ctx->codes_nat.p;
        return huffman_decode(g.nb, in.d_stream + s.off_pay, (unsigned)s.off_pay, (const u64 *)ctx->reg_rank.p, (const u64 *)ctx->reg_flags.p, s.max_box);
    }
    // the Huffman decode of `nb` boxes into d_codes, box after box: their payloads at payload + box_off[b] (`bytes_before` bytes of the buffer lie in front of
    // `payload`, 64 behind the last one), the largest of `max_box` bytes; the node table is in ctx->dec_tab
    int huffman_decode(int nb, const unsigned char *payload, unsigned bytes_before, const u64 *box_off, const u64 *box_bytes, u64 max_box) {
        const dec_table &D = s.D;
        const hdec_fit fit = hdec_lut_fit(max_box, D.n_nodes, D.single_symbol, g.bel);
        if (fit.takes) {
            hdec_launch hl; hl.add(fit); hl.close();
            const size_t lut_off = up64(D.dtab.size() * 4);
            TRY(ensure(ctx, ctx->dec_tab, lut_off + SZH_LUT_BYTES));          // (grown before the table went up: above)
            hipLaunchKernelGGL(k_hdec_build_lut, dim3(SZH_LUT_SIZE / 256), dim3(256), 0, st, (const unsigned *)ctx->dec_tab.p, (uint4 *)((char *)ctx->dec_tab.p + lut_off));
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_omp_hdec_lut, dim3((unsigned)nb), dim3(256), hl.lds_lut, st, g.bel, payload, bytes_before,
                               box_off, box_bytes, (const unsigned *)ctx->dec_tab.p, D.n_nodes, hl.tab_lds(D.n_nodes),
                               (const uint4 *)((char *)ctx->dec_tab.p + lut_off), fit.stage_bytes, d_codes, (unsigned *)(sm + SM_ERR));
        } else {
            const int tab_lds = D.dtab.size() * 4 <= 16384;            // node table and payload in LDS when they are small (the usual case: 2 - 3 bits per code)
            const unsigned pay_cap = (unsigned)std::min<u64>(max_box, 24576);
            const size_t lds = (tab_lds ? D.dtab.size() * 4 : 0) + (size_t)pay_cap + 16;
            hipLaunchKernelGGL(k_omp_hdec, dim3((unsigned)nb), dim3(256), lds, st, g.bel, payload, box_off,
                               box_bytes, (const unsigned *)ctx->dec_tab.p, D.n_nodes, tab_lds, pay_cap, D.single_symbol, d_codes, (unsigned *)(sm + SM_ERR));
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[1], st));
        return SZHIP_OK;
    }
    // ---- reconstruct: the inverse of the compress call's sweep
    int reconstruct() {
        packed = view() && out_on_device && omp_view_packs(g, out, pitch0, pitch1, sizeof(T));      // (then: decoded contiguous, k_view_scatter in finish)
        TRY(device_out(ctx, out, out_on_device && !packed, (size_t)n, &d_out));
        if (view() && out_on_device && !packed) omp_view_pitches(&g, pitch0, pitch1, sizeof(T));       // (a view on the host: decoded contiguous, its rows copied out in finish)
        return sweep();
    }
    bool view() const { return pitch1 != 0 && (pitch1 != r2 || pitch0 != r1 * r2); }
    // the boxes of `g` from d_codes, d_first, d_unpred / d_uoff into d_out, whose pitches `g` has
    int sweep() {
        if ((uintptr_t)d_out & 15u) g.vec = 0;
        const size_t row_bytes = (size_t)g.d1 * sizeof(T), plane_bytes = (size_t)g.d0 * sizeof(T);
        const int rows = g.c0 * g.c1, box_threads = rows;      // one lane per row
        HIPCHK(hipEventRecord(ctx->ev[2], st));
        if (omp_col_applies(g, d_out, row_bytes, plane_bytes)) {
            // the verbatim values go to their places in the output first (boxes that have any); the sweep picks them up where a code is zero
            const int fw = omp_flag_words<T>(g);
            unsigned *d_vflags = nullptr;
            if (E > 0) {
                if (fw > 0) {
                    TRY(ensure(ctx, ctx->chunk_bits, (size_t)g.nb * fw * 4));
                    d_vflags = (unsigned *)ctx->chunk_bits.p;
                    HIPCHK(hipMemsetAsync(d_vflags, 0, (size_t)g.nb * fw * 4, st));
                }
                hipLaunchKernelGGL((k_omp_scatter<T>), dim3((unsigned)g.nb), dim3(256), 0, st, g, (const uint16_t *)d_codes, d_uoff, d_unpred, d_out,
                                   (unsigned *)(sm + SM_ERR), d_vflags, fw);
                HIPCHK(hipGetLastError());
            }
            szh_oc::sweep_args<T> oa;
            oa.vflags = d_vflags; oa.fw = fw;
            oa.g = g; oa.data = nullptr; oa.out = d_out; oa.eb = s.eb; oa.recip = (T)(1 / s.eb); oa.intervals = (int)s.intervals; oa.codes = d_codes;
            oa.ucount = (unsigned *)(sm + SM_ERR); oa.ucount64 = nullptr; oa.first = const_cast<T *>(d_first); oa.uoff = d_uoff;
            hipLaunchKernelGGL((k_omp_col<T, 32, 32, true>), dim3((unsigned)(g.nb / 2)), dim3(64), 0, st, oa);
        } else hipLaunchKernelGGL((g.vec ? k_omp_box<T, true, true> : k_omp_box<T, true, false>), dim3((unsigned)g.nb), dim3((unsigned)box_threads), (size_t)4 * g.c0 * g.pitch * sizeof(T), st, g, (const T *)nullptr,
                                  d_out, s.eb, (T)(1 / s.eb), (int)s.intervals, d_codes, (unsigned *)(sm + SM_ERR), (u64 *)nullptr, const_cast<T *>(d_first), d_unpred, d_uoff);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[3], st));
        S.quant_kernel = omp_col_applies(g, d_out, row_bytes, plane_bytes) ? 3 : (g.vec ? 4 : 5);
        return SZHIP_OK;
    }
    // ---- the array to the caller, the kernels' error count, the statistics
    int finish() {
        unsigned bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, sm + SM_ERR, 4, hipMemcpyDeviceToHost, st));
        if (view() && (!out_on_device || packed)) {                // only a stream whose boxes all decoded reaches the caller's array
            HIPCHK(hipStreamSynchronize(st));
            if (bad) FAIL(SZHIP_ERR_STREAM, "%u boxes whose payload or verbatim-value count does not fit their codes", bad);
            TRY(scatter_view_impl<T>(ctx, d_out, r0, r1, r2, out, out_on_device, pitch0, pitch1));
        } else TRY(return_out(ctx, out, out_on_device, d_out, (size_t)n));
        HIPCHK(hipStreamSynchronize(st));
        if (bad) FAIL(SZHIP_ERR_STREAM, "%u boxes whose payload or verbatim-value count does not fit their codes", bad);
        decompress_times(ctx, S, host_ms, t_begin, (size_t)n * sizeof(T));
        return SZHIP_OK;
    }
};

template <class T>
int decompress_omp_impl(szhip_ctx *ctx, const unsigned char *stream_in, int stream_on_device, size_t stream_len, size_t body_off, size_t r0, size_t r1, size_t r2,
                        void *out, int out_on_device, size_t pitch0, size_t pitch1, szhip_stats *stats)
{
    omp_dec<T> d{call_base(ctx), stream_len, body_off, r0, r1, r2, out, out_on_device, {ctx, stream_in, stream_on_device, stream_len}};
    d.pitch0 = pitch0; d.pitch1 = pitch1;
    TRY(d.read_header());
    TRY(d.decode_boxes());
    TRY(d.reconstruct());
    TRY(d.finish());
    return d.done(stats);
}

// One call for a sub-box [lo, hi) of the array (szhip_decompress_omp_region).  The boxes that meet the region are a rectangular sub-grid of the box grid; the
// call decodes them alone, with the kernels of the full decode launched over COMPACT tables (sub-grid order: box (i0, i1, i2) of the sub-grid is number
// (i0 n1 + i1) n2 + i2, as szh_omp_box_origin_bytes counts the boxes of a geometry) and a sub-geometry `gs` whose box counts are the sub-grid's and whose pitches
// are those of an array of just these boxes.  That array is `out` itself when the region ends on box boundaries (the direct form), else a staging array in the
// context out of which k_omp_crop cuts the region.  The host's walk over the stream's tables (read_header) is the only step that grows with all boxes.
template <class T>
struct omp_region {
    omp_dec<T> &d; const size_t *const lo, *const hi;
    szhip_ctx *const ctx = d.ctx; const hipStream_t st = d.st;
    omp_subgrid<T> c;                                          // the covered sub-grid, its compact tables and pieces, the sub-geometry
    // the call's device blob: [payload sizes][payload offsets][ranks + 1][spans] | [first values][verbatim values][64 bytes, the payloads, 64 zero bytes]
    size_t o_bytes = 0, o_off = 0, o_uoff = 0, o_spans = 0, o_first = 0, o_unp = 0, o_pay = 0, blob_len = 0, n_spans = 0;
    unsigned char *d_blob = nullptr; T *d_stage = nullptr, *d_crop = nullptr;

    // ---- the covered sub-grid; the compact tables and, of a host stream, the covered boxes' values and payloads: one blob, one upload.  Of a device
    // stream the spans go up instead and k_omp_gather fetches them.
    int tables() {
        const bool dev = d.in.on_device != 0;
        c.cover(d.g, lo, hi, d.s, dev ? d.in.stream_in : nullptr);
        const size_t nbc = (size_t)c.nbc;
        o_bytes = 0; o_off = up16(o_bytes + nbc * 8); o_uoff = up16(o_off + nbc * 8); o_spans = up16(o_uoff + (nbc + 1) * 8);
        n_spans = dev ? c.pieces.size() : 0;
        o_first = up16(o_spans + n_spans * 24); o_unp = up16(o_first + nbc * sizeof(T)); o_pay = up16(o_unp + (size_t)c.Ec * sizeof(T)) + 64;
        blob_len = o_pay + c.pay_len + 64;
        c.place_pieces(o_first, o_unp, o_pay);
        TRY(ensure(ctx, ctx->seg_hist, blob_len));
        d_blob = (unsigned char *)ctx->seg_hist.p;
        const size_t up_len = dev ? o_first : blob_len;
        TRY(ensure_pinned3(ctx, up_len));
        unsigned char *hb = (unsigned char *)ctx->pinned3;
        memcpy(hb + o_bytes, c.cbytes.data(), nbc * 8); memcpy(hb + o_off, c.coff.data(), nbc * 8); memcpy(hb + o_uoff, c.cu.data(), (nbc + 1) * 8);
        if (dev) {
            u64 *sp = (u64 *)(hb + o_spans);
            for (size_t p = 0; p < c.pieces.size(); ++p) { sp[3 * p] = c.pieces[p].src; sp[3 * p + 1] = c.pieces[p].dst; sp[3 * p + 2] = c.pieces[p].len; }
            HIPCHK(hipMemcpyAsync(d_blob, hb, up_len, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemsetAsync(d_blob + blob_len - 64, 0, 64, st));
            hipLaunchKernelGGL(k_omp_gather, dim3((unsigned)n_spans), dim3(256), 0, st, d.in.stream_in, d_blob, (const u64 *)(d_blob + o_spans));
            HIPCHK(hipGetLastError());
        } else {
            for (const auto &pc : c.pieces) memcpy(hb + pc.dst, d.in.stream_in + pc.src, pc.len);
            memset(hb + blob_len - 64, 0, 64);
            HIPCHK(hipMemcpyAsync(d_blob, hb, up_len, hipMemcpyHostToDevice, st));
        }
        d.S.n_blocks = (uint64_t)c.nbc; d.S.n_elements = (uint64_t)c.n_out; d.S.n_unpred = c.Ec;
        return SZHIP_OK;
    }
    // ---- the covered boxes' codes (compact, box after box), then the sweeps over the sub-geometry, then the crop
    int decode() {
        const szh_omp_geom g = d.g;
        const dec_table &D = d.s.D;
        TRY(clear_small(ctx, &d.sm));
        TRY(ensure(ctx, ctx->dec_tab, up64(D.dtab.size() * 4) + SZH_LUT_BYTES + 16));
        HIPCHK(hipMemcpyAsync(ctx->dec_tab.p, D.dtab.data(), D.dtab.size() * 4, hipMemcpyHostToDevice, st));
        TRY(ensure(ctx, ctx->codes_nat, (size_t)c.nbc * g.bel * 2 + 64));
        d.d_codes = (uint16_t *)ctx->codes_nat.p;
        d.d_uoff = (const u64 *)(d_blob + o_uoff); d.d_first = (const T *)(d_blob + o_first); d.d_unpred = (const T *)(d_blob + o_unp);
        TRY(d.huffman_decode(c.nbc, d_blob + o_pay, (unsigned)o_pay, (const u64 *)(d_blob + o_off), (const u64 *)(d_blob + o_bytes), c.max_box));
        const size_t n_stage = (size_t)c.nbc * g.bel;
        if (c.direct) TRY(device_out(ctx, d.out, d.out_on_device, c.n_out, &d_crop));        // (n_stage == n_out)
        else {
            TRY(ensure(ctx, ctx->out, n_stage * sizeof(T)));
            d_stage = (T *)ctx->out.p;
            d_crop = (T *)d.out;
            if (!d.out_on_device) { TRY(ensure(ctx, ctx->codes_blk, c.n_out * sizeof(T))); d_crop = (T *)ctx->codes_blk.p; }
        }
        d.g = c.gs; d.E = c.Ec; d.d_out = c.direct ? d_crop : d_stage;
        TRY(d.sweep());
        if (!c.direct) {
            const int cpr = (int)((c.ext[2] + 16 / sizeof(T) - 1) / (16 / sizeof(T)));
            const int64_t total = (int64_t)(c.ext[0] * c.ext[1]) * cpr;
            hipLaunchKernelGGL((k_omp_crop<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const T *)d_stage + c.lo_off, c.gs.d0, c.gs.d1, d_crop, (int)c.ext[1], (int)c.ext[2], cpr, total);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ctx->ev[3], st));
        }
        return SZHIP_OK;
    }
    // ---- the region to the caller, the kernels' error count (covered boxes only), the statistics
    int finish() {
        unsigned bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, d.sm + SM_ERR, 4, hipMemcpyDeviceToHost, st));
        TRY(return_out(ctx, d.out, d.out_on_device, d_crop, c.n_out));
        HIPCHK(hipStreamSynchronize(st));
        if (bad) FAIL(SZHIP_ERR_STREAM, "%u boxes of the region whose payload or verbatim-value count does not fit their codes", bad);
        decompress_times(ctx, d.S, d.host_ms, d.t_begin, c.n_out * sizeof(T));
        return SZHIP_OK;
    }
};

template <class T>
int decompress_omp_region_impl(szhip_ctx *ctx, const unsigned char *stream_in, int stream_on_device, size_t stream_len, size_t body_off, size_t r0, size_t r1, size_t r2,
                               const size_t *lo, const size_t *hi, void *out, int out_on_device, szhip_stats *stats)
{
    omp_dec<T> d{call_base(ctx), stream_len, body_off, r0, r1, r2, out, out_on_device, {ctx, stream_in, stream_on_device, stream_len}};
    d.in.whole = false;
    const double h0 = now_ms();                                // (szhip_stats.ms_host: the header and tables read, the walk over them, the compact tables built)
    TRY(d.read_header());
    omp_region<T> r{d, lo, hi};
    TRY(r.tables());
    d.host_ms += now_ms() - h0;
    TRY(r.decode());
    TRY(r.finish());
    return d.done(stats);
}

