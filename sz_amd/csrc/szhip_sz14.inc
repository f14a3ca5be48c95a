// szhip_sz14.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace): the SZ 1.4 container (3-D / 2-D / 1-D, MSST19 tables).
// =====================================================================================================================
// SZ 1.4 ("no regression") 3-D path: SZ_compress_float_3D_MDQ (sz/src/sz_float.c:946-1415) + convertTDPStoFlatBytes_float
// (TightDataPointStorageF.c:379-479,590-663), and the inverse decompressDataSeries_float_3D (szd_float.c:600-1138).
// Whole-array Lorenzo on the same wavefront kernel (fmt = 1); the code array is already in stream order; the "exact" values are
// compacted in scan order and packed by k_exact_*.
// =====================================================================================================================

// required length (bits) of an exact value and the median it is taken against (sz_float.c:45-56 / sz_double.c:44-55)
template <class T> int req_length(double eb, T range, T *median);
template <> int req_length<float>(double eb, float range, float *median)
{
    const float half = range / 2; uint32_t u; memcpy(&u, &half, 4);
    uint64_t e; memcpy(&e, &eb, 8);
    const int reqExpo = (int)((e >> 52) & 0x7ff) - 1023, radExpo = (int)((u >> 23) & 0xff) - 127;
    int req = 9 + radExpo - reqExpo + 1;
    if (req < 9) req = 9;
    if (req > 32) { req = 32; *median = 0; }
    return req;
}
template <> int req_length<double>(double eb, double range, double *median)
{
    const double half = range / 2; uint64_t u; memcpy(&u, &half, 8);
    uint64_t e; memcpy(&e, &eb, 8);
    const int reqExpo = (int)((e >> 52) & 0x7ff) - 1023, radExpo = (int)((u >> 52) & 0x7ff) - 1023;
    int req = 12 + radExpo - reqExpo;
    if (req < 12) req = 12;
    if (req > 64) { req = 64; *median = 0; }
    return req;
}

template <class T>
int launch_pencil14(szhip_ctx *ctx, const szh_geom3 &G, u64 *sm, bool dec, const T *d_in, T *d_out, uint16_t *d_codes, T eb, unsigned intervals,
                    T median, int ign_bits, const msst_tab *mt = nullptr, int ndim = 3)
{   // mt != nullptr: the table-driven point-wise-relative quantiser (fmt 2) instead of the SZ 1.4 one
    hipStream_t st = ctx->stream;
    int nI, nJ, ntiles;
    using TS = szh_tile_shape<T>;
    TRY(prepare_pencil(ctx, G, szh_gran<T>::NW, TS::TPI, TS::TPJ, &nI, &nJ, &ntiles));
    szh_qargs<T> a; memset(&a, 0, sizeof(a));
    a.G = G; a.data = d_in; a.out = d_out; a.codes = d_codes; a.blk_lor = nullptr; a.coef = nullptr; a.coef_stride = 0;
    a.eb = eb; a.recip = 1 / eb; a.mean = 0; a.cap = (int)intervals; a.radius = (int)intervals / 2; a.use_mean = 0;
    a.fmt = 1; a.median = median; a.ign_bits = ign_bits;
    if (mt) {
        a.fmt = 2; a.ptab = mt->ptab; a.cells = mt->cells; a.tbase = mt->base; a.trange = mt->range; a.tbits = mt->bits;
        a.f32arith = (sizeof(T) == 4 && ndim == 2) ? 1 : 0; a.ndim3 = ndim == 3 ? 1 : 0;
    }
    a.faceI = (szh_u64 *)ctx->faceI.p; a.faceJ = (szh_u64 *)ctx->faceJ.p; a.epoch = ++ctx->epoch;
    a.nI = nI; a.nJ = nJ; a.order = (const unsigned *)ctx->order.p;
    a.ticket = (unsigned *)(sm + SM_TICKET); a.err = (unsigned *)(sm + SM_ERR); a.ticket_mode = ctx->ticket_atomic ? 0 : tune_int("SZ_HIP_TICKET_MODE", 2);
    a.progress = (szh_u64 *)ctx->progress.p; a.backoff = SZH_FILL_BACKOFF; a.wide = pencil_wide<T>(G, nJ);
    HIPCHK(hipEventRecord(ctx->ev[2], st));
    const unsigned pgrid = pencil_grid(ctx, a, ntiles);
    if (mt && dec) hipLaunchKernelGGL((k_pencil<T, true, true>), dim3(pgrid), dim3((TS::TPI * TS::TPJ + 2) * 64), 0, st, a);
    else if (mt) hipLaunchKernelGGL((k_pencil<T, false, true>), dim3(pgrid), dim3((TS::TPI * TS::TPJ + 2) * 64), 0, st, a);
    else if (dec) hipLaunchKernelGGL((k_pencil<T, true>), dim3(pgrid), dim3((TS::TPI * TS::TPJ + 2) * 64), 0, st, a);
    else hipLaunchKernelGGL((k_pencil<T, false>), dim3(pgrid), dim3((TS::TPI * TS::TPJ + 2) * 64), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[3], st));
    return SZHIP_OK;
}


// =====================================================================================================================
// Point-wise relative bounds, table-driven ("MSST19") form: host tables and the sweep (szh_msst.h)
// =====================================================================================================================
struct MsstHostTab { std::vector<double> ptab; std::vector<uint16_t> cells; u64 base = 0, range = 0; int bits = 0; };
static inline u64 f64_bits(double v) { u64 u; memcpy(&u, &v, 8); return u; }
// precisionTable (sz_float.c:2288-2293) and MultiLevelCacheTableWideIntervalBuild (MultiLevelCacheTableWideInterval.c:53-107); pow is the host's
static int msst_build_tab(MsstHostTab &t, double precision, unsigned count, int plus_bits, bool want_cells)
{
    const int radius = (int)count / 2;
    t.ptab.resize(count);
    const double inv = 2.0 - pow(2, -plus_bits);
    for (unsigned i = 0; i < count; ++i) t.ptab[i] = pow(1 + precision, inv * ((int)i - radius));
    if (!want_cells) return 0;
    const uint16_t bits = (uint16_t)((uint16_t)(-((f64_bits(precision) >> 52) - 1023)) + plus_bits);
    if (bits < 1 || bits > 24) return -1;
    t.bits = bits;
    const double bottom = t.ptab[1] / (1 + precision), top = t.ptab[count - 1] / (1 - precision);
    const uint16_t base = (uint16_t)(f64_bits(bottom) >> 52), topi = (uint16_t)(f64_bits(top) >> 52);
    if (topi < base || (u64)(topi - base + 1) << bits > (1ull << 28)) return -1;
    t.base = base; t.range = (u64)(topi - base);
    t.cells.assign((size_t)(t.range + 1) << bits, 0);
    auto rebuild = [&](uint16_t expo, u64 manti) { u64 u = (u64)expo << 52; u += manti << (52 - bits); double r; memcpy(&r, &u, 8); return r; };
    uint32_t index = 0; bool flag = false;
    for (uint32_t i = 0; i <= (uint32_t)(topi - base); ++i) {
        const uint16_t expo = (uint16_t)(i + base);
        for (uint32_t j = 0; j < (1u << bits); ++j) {
            const double sb = rebuild(expo, j), stp = rebuild(expo, (u64)j + 1);
            const double bb = t.ptab[index] / (1 + precision), tb = t.ptab[index] / (1 - precision);
            uint16_t &cell = t.cells[((size_t)i << bits) + j];
            if (stp < tb && sb > bb) { cell = (uint16_t)index; flag = true; }
            else if (flag && index < count - 1) { ++index; cell = (uint16_t)index; }
            else cell = 0;
        }
    }
    return 0;
}
// the histogram bin of one sample: `radiusIndex = (uint64_t)fabs(log2(pred_err)/divider+0.5)` with gcc's x86-64 double -> uint64 sequence
static inline u64 msst_radius_index(double pe, double divider)
{
    const double v = fabs(log2(pe) / divider + 0.5);
    if (v != v) return 0x8000000000000000ull;
    if (v >= 9223372036854775808.0) { const double w = v - 9223372036854775808.0; return (w < 9223372036854775808.0 ? (u64)(int64_t)w : 0x8000000000000000ull) ^ 0x8000000000000000ull; }
    return (u64)(int64_t)v;
}
// optimize_intervals_float_{1,2,3}D_opt_MSST19 (sz_float.c:4468, :4518, :4578; doubles sz_double.c:4163-).  The quotients come from the device
// (k_msst_sample: IEEE adds and divisions, the same bits as the host's), the logarithm and the bin from the host (glibc's log2, as in the reference).
// The reference's walk skips samples that are zero WITHOUT advancing its column counter; zeros are left only when the array's first element is zero
// (nearZero = 0: nothing replaces them) -- then the walk is done here, on a host copy of the array.
template <class T>
int msst_intervals(szhip_ctx *ctx, const szh_geom3 &G, int ndim, const T *d_in, const szhip_params *prm, double precision, bool zeros_left, unsigned *out)
{
    hipStream_t st = ctx->stream;
    const unsigned max_radius = prm->max_quant_intervals / 2;
    const int sd = prm->sample_distance;
    const double divider = (double)(T)(log2(1 + precision) * 2);
    std::vector<u64> hist(max_radius, 0);
    auto add = [&](double pe) { u64 ri = msst_radius_index(pe, divider); if (ri >= max_radius) ri = max_radius - 1; ++hist[ri]; };
    const int64_t n = G.n, r2 = G.g2.count;
    if (zeros_left) {
        std::vector<T> h((size_t)n);
        HIPCHK(hipMemcpyAsync(h.data(), d_in, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const T *d = h.data();
        const int64_t r3 = r2, r23 = ndim == 3 ? G.d0 : 0, rows = ndim == 3 ? G.g1.count : 0;
        if (ndim == 1) {
            for (int64_t pos = 2; pos < n; pos += sd) { if (d[pos] == 0) continue; add(fabs((double)d[pos] / (double)d[pos - 1])); }
        } else if (ndim == 2) {
            int64_t oc = sd - 1, n1 = 1, pos = r3 + oc;
            while (pos < n) {
                if (d[pos] == 0) { pos += sd; continue; }
                const T pv = d[pos - 1] + d[pos - r3] - d[pos - r3 - 1];
                add(fabs((double)(T)(pv / d[pos])));
                oc += sd;
                if (oc >= r3) { ++n1; const int64_t oc2 = n1 % sd; pos += (r3 + sd - oc) + (sd - oc2); oc = sd - oc2; if (oc == 0) ++oc; }
                else pos += sd;
            }
        } else {
            int64_t oc = sd - 2, n1 = 1, n2 = 1, pos = r23 + r3 + oc;
            while (pos < n) {
                if (d[pos] == 0) { pos += sd; continue; }
                const T pv = d[pos - 1] + d[pos - r3] + d[pos - r23] - d[pos - 1 - r23] - d[pos - r3 - 1] - d[pos - r3 - r23] + d[pos - r3 - r23 - 1];
                add(fabs((double)(T)(d[pos] / pv)));
                oc += sd;
                if (oc >= r3) {
                    ++n2;
                    if (n2 == rows) { ++n1; n2 = 1; pos += r3; }
                    const int64_t oc2 = (n1 + n2) % sd;
                    pos += (r3 + sd - oc) + (sd - oc2); oc = sd - oc2; if (oc == 0) ++oc;
                } else pos += sd;
            }
        }
    } else {
        const int64_t nrows = ndim == 1 ? 0 : szh_sample_row_limit(G, sd);
        const int per_row = (int)(r2 / sd + 2);
        const int64_t slots = ndim == 1 ? (n > 2 ? (n - 2 + sd - 1) / sd : 0) : nrows * per_row;
        if (slots > 0) {
            TRY(ensure(ctx, ctx->msst_pe, (size_t)slots * 8));
            const int64_t work = ndim == 1 ? slots : nrows;
            const int grid = (int)std::min<int64_t>((work + 255) / 256, 4096);
            hipLaunchKernelGGL((k_msst_sample<T>), dim3(grid), dim3(256), 0, st, G, ndim, d_in, nrows, sd, per_row, (double *)ctx->msst_pe.p);
            HIPCHK(hipGetLastError());
            std::vector<double> pe((size_t)slots);
            HIPCHK(hipMemcpyAsync(pe.data(), ctx->msst_pe.p, (size_t)slots * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (int64_t k = 0; k < slots; ++k) { if (f64_bits(pe[(size_t)k]) == 0x7ff8000000000001ull) continue; add(pe[(size_t)k]); }
        }
    }
    *out = pick_intervals(hist.data(), max_radius, prm->pred_threshold, sizeof(T) == 8 ? 64u : 32u);
    return SZHIP_OK;
}
static int msst_upload(szhip_ctx *ctx, const MsstHostTab &ht, unsigned intervals, bool dec, msst_tab *tb)
{
    hipStream_t st = ctx->stream;
    memset(tb, 0, sizeof(*tb));
    TRY(ensure(ctx, ctx->msst_ptab, (size_t)intervals * 8));
    HIPCHK(hipMemcpyAsync(ctx->msst_ptab.p, ht.ptab.data(), (size_t)intervals * 8, hipMemcpyHostToDevice, st));
    tb->ptab = (const double *)ctx->msst_ptab.p; tb->intervals = (int)intervals;
    if (!dec) {
        TRY(ensure(ctx, ctx->msst_cells, ht.cells.size() * 2 + 16));
        HIPCHK(hipMemcpyAsync(ctx->msst_cells.p, ht.cells.data(), ht.cells.size() * 2, hipMemcpyHostToDevice, st));
        tb->cells = (const uint16_t *)ctx->msst_cells.p; tb->base = ht.base; tb->range = ht.range; tb->bits = ht.bits;
    }
    HIPCHK(hipStreamSynchronize(st));                        // the host vectors are pageable: the copies must be over before they go away
    return SZHIP_OK;
}
// the sweep: one launch per hyperplane (1-D: the one-lane chain).  codes: u16 per element; rec: the reconstruction (DEC: in place)
template <class T>
int msst_sweep(szhip_ctx *ctx, const szh_geom3 &G, int ndim, bool dec, const T *d_in, T *d_rec, uint16_t *d_codes, const MsstHostTab &ht, unsigned intervals,
               int ign_bits)
{
    hipStream_t st = ctx->stream;
    msst_tab tb;
    TRY(msst_upload(ctx, ht, intervals, dec, &tb));
    HIPCHK(hipEventRecord(ctx->ev[2], st));
    if (ndim == 1) {
        const size_t lds = (size_t)intervals * 8 + (dec ? 0 : ht.cells.size() * 2);
        const int in_lds = lds <= 60 * 1024;
        if (dec) hipLaunchKernelGGL((k_msst_chain_1d<T, true>), dim3(1), dim3(64), in_lds ? lds : 0, st, (const T *)nullptr, d_rec, d_codes, G.n, tb, (int)intervals, (int64_t)0, ign_bits, in_lds);
        else hipLaunchKernelGGL((k_msst_chain_1d<T, false>), dim3(1), dim3(64), in_lds ? lds : 0, st, d_in, (T *)nullptr, d_codes, G.n, tb, (int)intervals, (int64_t)ht.cells.size(), ign_bits, in_lds);
        HIPCHK(hipGetLastError());
    } else {
        const int r0 = ndim == 3 ? G.g0.count : 1, r1 = G.g1.count, r2 = G.g2.count;
        for (int d = 0; d <= (r0 - 1) + (r1 - 1) + (r2 - 1); ++d) {
            const int a_lo = std::max(0, d - (r1 - 1) - (r2 - 1)), a_hi = std::min(d, r0 - 1);
            const int64_t threads = (int64_t)(a_hi - a_lo + 1) * r1;
            const unsigned grid = (unsigned)((threads + 255) / 256);
            if (dec) hipLaunchKernelGGL((k_msst_plane<T, true>), dim3(grid), dim3(256), 0, st, r0, r1, r2, ndim, d, (const T *)nullptr, d_rec, d_codes, tb, ign_bits);
            else hipLaunchKernelGGL((k_msst_plane<T, false>), dim3(grid), dim3(256), 0, st, r0, r1, r2, ndim, d, d_in, d_rec, d_codes, tb, ign_bits);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ctx->ev[3], st));
    return SZHIP_OK;
}

// the zero codes (exact values) of a code array in scan order: counted per chunk of SZH_LIN_CHUNK codes, the chunks' ranks to ctx->col_off, the total to SM_TOTAL_UNPRED
static int rank_zero_codes(szhip_ctx *ctx, const uint16_t *d_codes, int64_t n, int64_t nlin, u64 *sm)
{
    TRY(ensure(ctx, ctx->col_zeros64, (size_t)nlin * 8));
    TRY(ensure(ctx, ctx->col_off, (size_t)nlin * 8));
    hipLaunchKernelGGL(k_lin_zero_count, dim3((unsigned)nlin), dim3(256), 0, ctx->stream, d_codes, n, (u64 *)ctx->col_zeros64.p);
    return scan_u64(ctx, (const u64 *)ctx->col_zeros64.p, nlin, (u64 *)ctx->col_off.p, sm + SM_TOTAL_UNPRED);
}

// One SZ 1.4 compress call: its state, and one member function per phase (compress14_impl is their sequence).
// pw != NULL: the data are log2|x| of a point-wise-relative call and the container carries the PW_REL fields
// r0 == 0: the 2-D compressor SZ_compress_float_2D_MDQ (sz_float.c:610): its predictors are those of the 3-D one's first layer,
// so it is carried as 1 x r1 x r2 (the block size of the carried geometry plays no role here); its optimiser has the 2-D lattice
// r0 == 0 and r1 == 0: the 1-D compressor SZ_compress_float_1D_MDQ (sz_float.c:353): a chain through the previous reconstructed
// value, walked by k_chain_1d; the container and everything after the code array are the same
// pw->msst19: the table-driven form of PW_REL (szh_msst.h): `data` has its zeros replaced, eb_in is the RATIO; another optimiser, another
// quantiser, exact values taken against 0, two more header bytes -- the entropy stage and the container are the same
template <class T>
struct sz14_call : call_base {
    static constexpr int is_double = sizeof(T) == 8;
    // ---- arguments, geometry
    const size_t r0, r1, r2; const szhip_params *const prm; const unsigned char *const meta; const size_t meta_len; const szhip_pwr *const pw;
    const int out_on_device; unsigned char **const out; size_t *const out_size;
    const double eb_in; const T eb = (T)eb_in;                 // eb: `float realPrecision` parameter of sz_float.c:946 (:353 for 1-D)
    const bool one_d = r0 == 0 && r1 == 0, msst = pw && pw->msst19; const int ndim = one_d ? 1 : r0 == 0 ? 2 : 3;
    const szh_geom3 G = one_d ? szh_make_geom2(1, (int)r2) : r0 == 0 ? szh_make_geom2((int)r1, (int)r2) : szh_make_geom3((int)r0, (int)r1, (int)r2);
    const int64_t n = G.n, nlin = (G.n + SZH_LIN_CHUNK - 1) / SZH_LIN_CHUNK;
    // ---- device arrays
    const T *d_in = nullptr; u64 *sm = nullptr; uint16_t *d_codes = nullptr;
    // ---- decisions: interval count, the format of an exact value
    unsigned intervals = 0; T median = 0; int req_len = 0, req_bytes = 0, resi_bits = 0, ign_bits = 0;
    // ---- the code book, the exact values, the stream's layout
    huff_ptr hf; std::vector<u64> tab_code; std::vector<uint8_t> tab_len; unsigned maxlen = 0;
    size_t tree_bytes = 0, pay_bytes = 0; u64 total_bits = 0, E = 0, nmid = 0;
    size_t lead_size = 0, resi_size = 0, blob = 0, hdr_len = 0, total_len = 0;
    std::vector<unsigned char> hdr;

    // ---- the array staged; interval optimiser (optimize_intervals_float_3D_opt, sz_float.c:4644): the SZ 2.1 sample lattice, radius histogram only; the format
    // of an exact value
    int choose_intervals(const void *data, int data_on_device, double range_in, double median_in) {
        S.n_elements = (uint64_t)n;
        TRY(stage_input(ctx, data, data_on_device, (size_t)n, &d_in));
        TRY(clear_small(ctx, &sm));
        HIPCHK(hipEventRecord(ctx->ev[0], st));
        intervals = prm->quantization_intervals;
        if (intervals == 0 && msst) {
            bool zeros_left = false;                                // only when the array's first element is zero (szhip_msst_prepare)
            { T first; HIPCHK(hipMemcpyAsync(&first, d_in, sizeof(T), hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st)); zeros_left = first == 0; }
            TRY(msst_intervals<T>(ctx, G, ndim, d_in, prm, eb_in, zeros_left, &intervals));
        } else if (intervals == 0)
            TRY(sampled_intervals<T>(ctx, G, one_d, d_in, prm, eb, sm, &intervals, &host_ms));
        if (intervals > 65536 || intervals < 4) FAIL(SZHIP_ERR_UNSUP, "quantization interval count %u outside [4,65536]", intervals);
        S.intervals = intervals;
        median = (T)median_in;
        if (msst) {
            // computeReqLength_float_MSST19 = 9 - exponent of (float)ratio (sz_float.c:58-62), the double rule 12 - exponent (sz_double.c:57-61) --
            // which the FLOAT 2-D quantiser also uses (sz_float.c:2041); exact values are the values themselves (no median)
            const int e64 = (int)((f64_bits(eb_in) & 0x7FF0000000000000ull) >> 52) - 1023;
            const float pf = (float)eb_in; unsigned u32; memcpy(&u32, &pf, 4);
            const int e32 = (int)((u32 & 0x7F800000u) >> 23) - 127;
            req_len = (is_double || ndim == 2) ? 12 - e64 : 9 - e32;
            median = 0;
            if (req_len < 9 || req_len > (int)sizeof(T) * 8) FAIL(SZHIP_ERR_UNSUP, "point-wise ratio %g needs %d leading bits per exact value", eb_in, req_len);
        } else req_len = req_length<T>((double)eb, (T)range_in, &median);
        req_bytes = req_len / 8; resi_bits = req_len % 8; ign_bits = (int)sizeof(T) * 8 - req_len;
        HIPCHK(hipEventRecord(ctx->ev[1], st));
        return SZHIP_OK;
    }
    // ---- predict + quantise: the table-driven quantiser (msst), the 1-D chain, or the wavefront kernel
    int quantise() {
        TRY(ensure(ctx, ctx->codes_nat, (size_t)n * 2 + 64));
        d_codes = (uint16_t *)ctx->codes_nat.p;
        S.quant_kernel_launches = 1;
        if (!msst) return one_d ? quantise_chain() : launch_pencil14<T>(ctx, G, sm, false, d_in, nullptr, d_codes, eb, intervals, median, ign_bits);
        MsstHostTab ht;
        double hb = now_ms();
        if (msst_build_tab(ht, eb_in, intervals, pw->plus_bits, true)) FAIL(SZHIP_ERR_UNSUP, "point-wise ratio %g with %u intervals: look-up table too large", eb_in, intervals);
        host_ms += now_ms() - hb;
        if (ndim >= 2 && !tune_int("SZ_HIP_MSST_SWEEP", 0)) {     // the wavefront kernel with its third quantiser (szh_pencil.h, fmt 2)
            msst_tab tb;
            TRY(msst_upload(ctx, ht, intervals, false, &tb));
            TRY(launch_pencil14<T>(ctx, G, sm, false, d_in, nullptr, d_codes, eb, intervals, (T)0, ign_bits, &tb, ndim));
        } else {                                                  // the plane-by-plane sweep (1-D: the one-lane chain); SZ_HIP_MSST_SWEEP=1 forces it
            TRY(ensure(ctx, ctx->msst_rec, (size_t)n * sizeof(T)));
            TRY(msst_sweep<T>(ctx, G, ndim, false, d_in, (T *)ctx->msst_rec.p, d_codes, ht, intervals, ign_bits));
            S.quant_kernel_launches = ndim == 1 ? 1 : (unsigned)((ndim == 3 ? G.g0.count : 1) + G.g1.count + G.g2.count - 2);
        }
        return SZHIP_OK;
    }
    // the chain cut at its certain restarts, one thread per segment; a segment whose successor turns out not to restart raises
    // the flag, and the array is then walked by the one-wavefront kernel (same result, by construction; SZ_HIP_1D_SERIAL=1 forces it)
    int quantise_chain() {
        HIPCHK(hipEventRecord(ctx->ev[2], st));
        unsigned violation = 1;
        if (!tune_int("SZ_HIP_1D_SERIAL", 0)) {
            const int grid = (int)std::min<int64_t>((n + 255) / 256, 1 << 20);
            hipLaunchKernelGGL((k_chain_seg_1d<T, false>), dim3(grid), dim3(256), 0, st, d_in, (T *)nullptr, d_codes, n, eb, (T)(1 / eb), (int)intervals,
                               median, ign_bits, tune_int("SZ_HIP_1D_REACH_PCT", 100) / 100.0, (unsigned *)(sm + SM_CHANGED));
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&violation, sm + SM_CHANGED, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        if (violation) {
            hipLaunchKernelGGL((k_chain_1d<T, false>), dim3(1), dim3(64), 0, st, d_in, (T *)nullptr, d_codes, n, eb, (T)(1 / eb), (int)intervals, median, ign_bits);
            HIPCHK(hipGetLastError());
            S.quant_kernel_launches = 2;
        }
        HIPCHK(hipEventRecord(ctx->ev[3], st));
        return SZHIP_OK;
    }
    // ---- histogram -> code book (host), exact-value counts
    int hist_and_book() {
        TRY(ensure(ctx, ctx->hist, (size_t)(65536 + 8192) * 4 + 64));
        unsigned *d_hist = (unsigned *)ctx->hist.p;
        TRY(ensure_pinned(ctx, (size_t)intervals * 4 + 64));
        unsigned *h_hist = (unsigned *)ctx->pinned;
        HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)intervals * 4, st));
        TRY(launch_hist_u16(ctx, st, d_codes, 0, n, intervals, d_hist));
        HIPCHK(hipMemcpyAsync(h_hist, d_hist, (size_t)intervals * 4, hipMemcpyDeviceToHost, st));
        TRY(rank_zero_codes(ctx, d_codes, n, nlin, sm));
        u64 h_small[SM_COUNT];
        HIPCHK(hipMemcpyAsync(h_small, sm, SM_COUNT * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if ((unsigned)h_small[SM_ERR] != 0) { ctx->wave_timeout = true; FAIL(SZHIP_ERR_INTERNAL, "wavefront kernel: halo wait timed out"); }
        E = h_small[SM_TOTAL_UNPRED];
        S.n_unpred = E;
        double h0 = now_ms();
        hf = host_book(h_hist, intervals, tab_code, tab_len, &maxlen);
        if (!hf) FAIL(SZHIP_ERR_INTERNAL, "Huffman build failed");
        tree_bytes = szhost_huff_tree_size(hf.get());
        total_bits = hf->total_bits;
        pay_bytes = (size_t)((total_bits + 7) / 8);
        host_ms += now_ms() - h0;
        return SZHIP_OK;
    }
    // ---- exact values: compact in scan order, lead numbers, mid-byte offsets
    int compact_exact() {
        if (E > 0) {
            TRY(ensure(ctx, ctx->unpred, (size_t)E * sizeof(T)));
            TRY(ensure(ctx, ctx->lor_bits, (size_t)E + 8));              // lead numbers, one byte each
            TRY(ensure(ctx, ctx->reg_flags, (size_t)E * 8));             // mid-byte counts
            TRY(ensure(ctx, ctx->reg_rank, (size_t)E * 8));              // mid-byte offsets
            hipLaunchKernelGGL((k_lin_zero_move<T, 0>), dim3((unsigned)nlin), dim3(256), 0, st, (const uint16_t *)d_codes, n, (const u64 *)ctx->col_off.p,
                               d_in, (T *)ctx->unpred.p, (T *)nullptr);
            hipLaunchKernelGGL((k_exact_lead<T>), dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, (const T *)ctx->unpred.p, (int64_t)E, median,
                               req_bytes, (uint8_t *)ctx->lor_bits.p, (u64 *)ctx->reg_flags.p);
            HIPCHK(hipGetLastError());
            TRY(scan_u64(ctx, (const u64 *)ctx->reg_flags.p, (int64_t)E, (u64 *)ctx->reg_rank.p, sm + SM_SCRATCH));
            HIPCHK(hipMemcpyAsync(&nmid, sm + SM_SCRATCH, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        lead_size = (size_t)((E * 2 + 7) / 8); resi_size = resi_bits ? (size_t)((E * (u64)resi_bits + 7) / 8) : 0;
        return SZHIP_OK;
    }
    // ---- container: everything in front of the Huffman payload, on the host
    void write_header() {
        const double h0 = now_ms();
        const size_t type_size = 8 + tree_bytes + pay_bytes;
        blob = pw ? (size_t)pw->signs_blob_size : 0;
        hdr_len = meta_len + 8 + 4 + (pw ? 1 + 8 + 4 : 0) + 4 + sizeof(T) + 1 + (msst ? 2 : 0) + 8 + 8 + 8 + 8 + (pw ? sizeof(T) : 0) + 8 + tree_bytes; // ... up to the Huffman payload
        total_len = hdr_len + pay_bytes + blob + lead_size + (size_t)nmid + resi_size;
        hdr.assign(hdr_len, 0);
        unsigned char *q = hdr.data();
        memcpy(q, meta, meta_len); q += meta_len;
        szhost_put_u64be(q, (uint64_t)n); q += 8;
        szhost_put_u32be(q, prm->max_quant_intervals); q += 4;
        if (pw) {                                                // TightDataPointStorageF.c:408-419
            *q++ = pw->rad_expo;
            szhost_put_u64be(q, pw->segment_size); q += 8;
            szhost_put_u32be(q, pw->signs_blob_size); q += 4;
        }
        szhost_put_u32be(q, intervals); q += 4;
        const T median_field = msst ? (T)pw->median_stored : median;
        if (is_double) szhost_put_f64be(q, (double)median_field); else szhost_put_f32be(q, (float)median_field);
        q += sizeof(T);
        *q++ = (unsigned char)req_len;
        if (msst) { *q++ = pw->plus_bits; *q++ = (unsigned char)maxlen; }       // plus_bits, max_bits (TightDataPointStorageF.c:431-435; Huffman.c:828-833)
        szhost_put_f64be(q, msst ? eb_in : (double)eb); q += 8;
        szhost_put_u64be(q, (uint64_t)type_size); q += 8;
        szhost_put_u64be(q, (uint64_t)E); q += 8;
        szhost_put_u64be(q, (uint64_t)nmid); q += 8;
        if (pw) {                                                // minLogValue in the data's type (:454-459; TightDataPointStorageD.c:456-461)
            if (is_double) szhost_put_f64be(q, pw->min_log_value); else szhost_put_f32be(q, (float)pw->min_log_value);
            q += sizeof(T);
        }
        szhost_put_u32be(q, (uint32_t)hf->n_nodes); q += 4;      // encode_withTree blob (Huffman.c:790-816)
        szhost_put_u32be(q, intervals); q += 4;
        szhost_huff_tree_write(hf.get(), q);
        hf.reset();
        host_ms += now_ms() - h0;
    }
    // ---- packing: header, Huffman payload, the sign bytes of a PW_REL call, the exact values' three tables into the stream buffer
    int pack() {
        TRY(upload_code_tables(ctx, tab_code, tab_len));
        TRY(ensure(ctx, ctx->stream_buf, total_len + 64));
        unsigned char *d_stream = (unsigned char *)ctx->stream_buf.p;
        HIPCHK(hipMemsetAsync(d_stream, 0, total_len + 64, st));
        HIPCHK(hipMemcpyAsync(d_stream, hdr.data(), hdr_len, hipMemcpyHostToDevice, st));
        if (blob) HIPCHK(hipMemcpyAsync(d_stream + hdr_len + pay_bytes, pw->signs_blob, blob, hipMemcpyHostToDevice, st));   // after the type array (:463-467)
        if (total_bits > 0) {
            TRY(chunk_bit_offsets(ctx, d_codes, n, intervals, sm, 0));
            TRY(launch_encode(ctx, d_codes, n, intervals, (u64)hdr_len * 8, d_stream));
        }
        if (E > 0) {
            unsigned char *lead_out = d_stream + hdr_len + pay_bytes + blob, *mid_out = lead_out + lead_size, *resi_out = mid_out + nmid;
            hipLaunchKernelGGL((k_exact_write<T>), dim3((unsigned)(((E + 7) / 8 + 255) / 256)), dim3(256), 0, st, (const T *)ctx->unpred.p, (int64_t)E,
                               median, req_bytes, resi_bits, (const uint8_t *)ctx->lor_bits.p, (const u64 *)ctx->reg_rank.p, lead_out, mid_out, resi_out,
                               (int64_t)resi_size);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ctx->ev[4], st));
        return SZHIP_OK;
    }
    // ---- delivery, the packed bit count against the book's, the statistics
    int deliver_and_check() {
        TRY(deliver_stream(ctx, (unsigned char *)ctx->stream_buf.p, total_len, out_on_device, out, out_size, false, false));
        u64 tb = 0;
        if (total_bits > 0) { HIPCHK(hipMemcpy(&tb, sm + SM_TOTAL_BITS, 8, hipMemcpyDeviceToHost)); }
        if (tb != total_bits) FAIL_PUBLISHED(SZHIP_ERR_INTERNAL, "encoded bit count mismatch (%llu vs %llu)", (unsigned long long)tb, (unsigned long long)total_bits);
        compress_times(ctx, S, host_ms, t_begin, total_len);
        return SZHIP_OK;
    }
};

template <class T>
int compress14_impl(szhip_ctx *ctx, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, double eb_in, double range_in,
                    double median_in, const szhip_params *prm, const unsigned char *meta, size_t meta_len, const szhip_pwr *pw, int out_on_device,
                    unsigned char **out, size_t *out_size, szhip_stats *stats)
{
    sz14_call<T> c{call_base(ctx), r0, r1, r2, prm, meta, meta_len, pw, out_on_device, out, out_size, eb_in};
    TRY(c.choose_intervals(data, data_on_device, range_in, median_in));
    TRY(c.quantise());
    TRY(c.hist_and_book());
    TRY(c.compact_exact());
    c.write_header();
    TRY(c.pack());
    TRY(c.deliver_and_check());
    return c.done(stats);
}

// One SZ 1.4 decompress call.  `body_off`: offset of the max_quant_intervals field (4 + 28|36 + 8);
// pwr: 0 plain, 1 PW_REL log-domain form, 2 PW_REL table-driven form (szh_msst.h)
template <class T>
struct sz14_dec : call_base {
    static constexpr int is_double = sizeof(T) == 8;
    // ---- arguments, geometry
    const size_t stream_len, body_off, r0, r1, r2; const int pwr; void *const out; const int out_on_device; stream_intake in;
    const bool one_d = r0 == 0 && r1 == 0, msst = pwr == 2; const int ndim = one_d ? 1 : r0 == 0 ? 2 : 3;            // one_d: decompressDataSeries_float_1D (szd_float.c:185)
    const szh_geom3 G = one_d ? szh_make_geom2(1, (int)r2) : r0 == 0 ? szh_make_geom2((int)r1, (int)r2) : szh_make_geom3((int)r0, (int)r1, (int)r2);
    const int64_t n = G.n, nlin = (G.n + SZH_LIN_CHUNK - 1) / SZH_LIN_CHUNK;
    // ---- the header
    unsigned intervals = 0; T median = 0, eb = 0; double eb_field = 0; int req_bytes = 0, resi_bits = 0, plus_bits = 0;
    uint64_t type_size = 0, E = 0, nmid = 0; size_t blob = 0, type_off = 0, lead_size = 0, resi_size = 0, pay_off = 0; u64 total_bits = 0;
    dec_table D;
    // ---- device arrays
    u64 *sm = nullptr; uint16_t *d_codes = nullptr; T *d_out = nullptr;

    // ---- the stream taken in; header + tree on the host (TightDataPointStorageF.c:54-265); a device-resident stream hands over a prefix
    int read_header() {
        S.n_elements = (uint64_t)n;
        TRY(in.open());
        double h0 = now_ms();
        const size_t fixed = 4 + (pwr ? 1 + 8 + 4 : 0) + 4 + sizeof(T) + 1 + (msst ? 2 : 0) + 8 + 8 + 8 + 8 + (pwr ? sizeof(T) : 0) + 8;
        if (body_off + fixed > stream_len) FAIL(SZHIP_ERR_STREAM, "truncated stream");
        TRY(in.fetch(body_off + fixed));
        const unsigned char *q = in.hs + body_off;
        q += 4;                                                        // max_quant_intervals
        if (pwr) { q += 1 + 8; blob = szhost_get_u32be(q); q += 4; }   // radExpo, segment_size, size of the sign bytes (TightDataPointStorageF.c:137-148)
        intervals = szhost_get_u32be(q); q += 4;
        median = is_double ? (T)szhost_get_f64be(q) : (T)szhost_get_f32be(q); q += sizeof(T);
        const int req_len = *q++;
        if (msst) { plus_bits = q[0]; q += 2; median = 0; }           // plus_bits, max_bits (TightDataPointStorageF.c:164-168); exact values carry no median
        eb_field = szhost_get_f64be(q);
        eb = (T)eb_field; q += 8;                                      // `float realPrecision = tdps->realPrecision`, szd_float.c:610
        type_size = szhost_get_u64be(q); q += 8;
        E = szhost_get_u64be(q); q += 8;
        nmid = szhost_get_u64be(q); q += 8;
        if (pwr) q += sizeof(T);                                       // minLogValue (the caller read it: szhip_sz14_pwr_locate)
        type_off = body_off + fixed - 8;                               // the blob starts with nodeCount | intervals
        if (intervals < 4 || intervals > 65536) FAIL(SZHIP_ERR_STREAM, "bad interval count %u", intervals);
        if (req_len < 9 || req_len > (int)sizeof(T) * 8) FAIL(SZHIP_ERR_STREAM, "bad exact-value length %d", req_len);
        if (!(eb > 0)) FAIL(SZHIP_ERR_STREAM, "bad error bound");
        req_bytes = req_len / 8; resi_bits = req_len % 8;
        lead_size = (size_t)((E * 2 + 7) / 8); resi_size = resi_bits ? (size_t)((E * (uint64_t)resi_bits + 7) / 8) : 0;
        if (E >= ((uint64_t)1 << 32)) FAIL(SZHIP_ERR_UNSUP, "more than 2^32 exact values");   // the prefix counts of k_exact_* are packed in 32-bit halves
        if (E > (uint64_t)n || type_size < 8 || type_size > stream_len || nmid > stream_len ||
            blob > stream_len || type_off + type_size + blob + lead_size + nmid + resi_size > stream_len) FAIL(SZHIP_ERR_STREAM, "truncated stream");
        const int node_count = (int)szhost_get_u32be(q);
        if (node_count <= 0 || 8 + szhost_huff_serial_size(node_count) > type_size) FAIL(SZHIP_ERR_STREAM, "bad Huffman tree size");
        const size_t tree_bytes = szhost_huff_serial_size(node_count);
        TRY(in.fetch(type_off + 8 + tree_bytes));
        if (!read_tree(in.hs + type_off + 8, node_count, intervals, D)) FAIL(SZHIP_ERR_STREAM, "bad Huffman tree");
        pay_off = type_off + 8 + tree_bytes;
        total_bits = (u64)(type_size - 8 - tree_bytes) * 8;
        S.intervals = intervals; S.n_unpred = E;
        host_ms += now_ms() - h0;
        return SZHIP_OK;
    }
    // ---- Huffman decode of the code array; its zero codes counted and ranked, and checked against the header
    int decode_codes() {
        TRY(clear_small(ctx, &sm));
        TRY(ensure(ctx, ctx->codes_nat, (size_t)n * 2 + 64));
        d_codes = (uint16_t *)ctx->codes_nat.p;
        TRY(huff_decode_device(ctx, sm, in.d_stream + pay_off, (unsigned)std::min<size_t>(pay_off, 4096), total_bits, D.dtab, D.n_nodes, D.single_symbol, n, d_codes));
        TRY(rank_zero_codes(ctx, d_codes, n, nlin, sm));
        u64 zeros_found = 0;
        HIPCHK(hipMemcpyAsync(&zeros_found, sm + SM_TOTAL_UNPRED, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return check_decoded(ctx, n, E, zeros_found, "exact");
    }
    // ---- exact values back into the output array
    int place_exact() {
        TRY(device_out(ctx, out, out_on_device, (size_t)n, &d_out));
        if (E > 0) {
            const unsigned char *lead_in = in.d_stream + type_off + type_size + blob, *mid_in = lead_in + lead_size, *resi_in = mid_in + nmid;
            const unsigned gE = (unsigned)((E + 255) / 256);
            TRY(ensure(ctx, ctx->unpred, (size_t)E * sizeof(T)));
            TRY(ensure(ctx, ctx->reg_flags, (size_t)E * 8 * 3));         // flag words: f01 | f2 | mid counts
            TRY(ensure(ctx, ctx->reg_rank, (size_t)E * 8 * 3));          // their exclusive prefix sums
            TRY(ensure(ctx, ctx->lor_bits, (size_t)E * 3 + 8));          // compacted own bytes of positions 0..2
            u64 *f01 = (u64 *)ctx->reg_flags.p, *f2 = f01 + E, *mc = f2 + E;
            u64 *s01 = (u64 *)ctx->reg_rank.p, *s2 = s01 + E, *mo = s2 + E;
            uint8_t *own0 = (uint8_t *)ctx->lor_bits.p, *own1 = own0 + E, *own2 = own1 + E;
            hipLaunchKernelGGL(k_exact_flags, dim3(gE), dim3(256), 0, st, lead_in, (int64_t)E, req_bytes, resi_bits, f01, f2, mc);
            TRY(scan_u64(ctx, f01, (int64_t)E, s01, sm + SM_SCRATCH));
            TRY(scan_u64(ctx, f2, (int64_t)E, s2, sm + SM_SCRATCH));
            TRY(scan_u64(ctx, mc, (int64_t)E, mo, sm + SM_SCRATCH));
            u64 mid_need = 0;
            HIPCHK(hipMemcpyAsync(&mid_need, sm + SM_SCRATCH, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (mid_need != nmid) FAIL(SZHIP_ERR_STREAM, "stream holds %llu mid bytes, lead numbers need %llu", (unsigned long long)nmid, (unsigned long long)mid_need);
            hipLaunchKernelGGL(k_exact_own, dim3(gE), dim3(256), 0, st, lead_in, (int64_t)E, req_bytes, resi_bits, mid_in, resi_in,
                               (const u64 *)s01, (const u64 *)s2, (const u64 *)mo, own0, own1, own2);
            hipLaunchKernelGGL((k_exact_build<T>), dim3(gE), dim3(256), 0, st, lead_in, (int64_t)E, req_bytes, resi_bits, mid_in, resi_in,
                               (const u64 *)s01, (const u64 *)s2, (const u64 *)mo, (const uint8_t *)own0, (const uint8_t *)own1, (const uint8_t *)own2,
                               median, (T *)ctx->unpred.p);
            hipLaunchKernelGGL((k_lin_zero_move<T, 1>), dim3((unsigned)nlin), dim3(256), 0, st, (const uint16_t *)d_codes, n, (const u64 *)ctx->col_off.p,
                               (const T *)nullptr, (T *)ctx->unpred.p, d_out);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ctx->ev[1], st));
        return SZHIP_OK;
    }
    // ---- reconstruct: the inverse of the compress call's quantiser
    int reconstruct() {
        if (msst) {
            if (!(eb_field > 0 && eb_field < 1) || plus_bits > 16) FAIL(SZHIP_ERR_STREAM, "bad point-wise ratio / table parameters");
            MsstHostTab ht;
            msst_build_tab(ht, eb_field, intervals, plus_bits, false);
            if (ndim >= 2 && !tune_int("SZ_HIP_MSST_SWEEP", 0)) {
                msst_tab tb;
                TRY(msst_upload(ctx, ht, intervals, true, &tb));
                TRY(launch_pencil14<T>(ctx, G, sm, true, nullptr, d_out, d_codes, eb, intervals, (T)0, 0, &tb, ndim));
            } else
                TRY(msst_sweep<T>(ctx, G, ndim, true, nullptr, d_out, d_codes, ht, intervals, 0));
        } else if (one_d) {
            HIPCHK(hipEventRecord(ctx->ev[2], st));
            if (tune_int("SZ_HIP_1D_SERIAL", 0))
                hipLaunchKernelGGL((k_chain_1d<T, true>), dim3(1), dim3(64), 0, st, (const T *)nullptr, d_out, d_codes, n, eb, (T)(1 / eb), (int)intervals, median, 0);
            else {   // decoding sees where the chain restarts (code 0): one thread per segment, nothing to verify
                const int grid = (int)std::min<int64_t>((n + 255) / 256, 1 << 20);
                hipLaunchKernelGGL((k_chain_seg_1d<T, true>), dim3(grid), dim3(256), 0, st, (const T *)nullptr, d_out, d_codes, n, eb, (T)(1 / eb), (int)intervals,
                                   median, 0, 1.0, (unsigned *)nullptr);
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ctx->ev[3], st));
        } else
            TRY(launch_pencil14<T>(ctx, G, sm, true, nullptr, d_out, d_codes, eb, intervals, median, 0));
        S.quant_kernel_launches = 1;
        return SZHIP_OK;
    }
    // ---- the array to the caller, the wavefront kernel's error flag, the statistics
    int finish() {
        unsigned kerr = 0;
        HIPCHK(hipMemcpyAsync(&kerr, sm + SM_ERR, 4, hipMemcpyDeviceToHost, st));
        TRY(return_out(ctx, out, out_on_device, d_out, (size_t)n));
        HIPCHK(hipEventRecord(ctx->ev[4], st));
        HIPCHK(hipStreamSynchronize(st));
        if (kerr) { ctx->wave_timeout = true; FAIL(SZHIP_ERR_INTERNAL, "wavefront kernel: halo wait timed out"); }
        decompress_times(ctx, S, host_ms, t_begin, (size_t)n * sizeof(T));
        return SZHIP_OK;
    }
};

template <class T>
int decompress14_impl(szhip_ctx *ctx, const unsigned char *stream_in, int stream_on_device, size_t stream_len, size_t body_off, int pwr,
                      size_t r0, size_t r1, size_t r2, void *out, int out_on_device, szhip_stats *stats)
{
    sz14_dec<T> d{call_base(ctx), stream_len, body_off, r0, r1, r2, pwr, out, out_on_device, {ctx, stream_in, stream_on_device, stream_len}};
    TRY(d.read_header());
    TRY(d.decode_codes());
    TRY(d.place_exact());
    TRY(d.reconstruct());
    TRY(d.finish());
    return d.done(stats);
}
