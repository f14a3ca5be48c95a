// szhip_sz21.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace): the SZ 2.1 path (sz_float.c:7126-7560 / szd_float.c:3491-5860 and the double twins): sz21_plan + sz21_call (a compress call's plan, its shared state and one member function per phase), compress_impl (the list of phases), the device Huffman decode, parse_header, decompress_impl.
// the device code book's verdict as the host reads it behind the call's final synchronisation (szh_book.h): the kernel's own status, the plan's (the stream
// outgrew the buffers), or the tests' switch -- any of them sends the call round again with the host's book
static bool book_declines(unsigned rec_status, unsigned long long plan_status, int test_switch) { return rec_status != 0 || plan_status != 0 || test_switch != 0; }

// Which sweep a compress call takes and how its codes are packed: a pure function of the geometry, the alphabet, the regression-block count, the switches and the
// context's flags, made once the chains' overlap is settled; `revise` is its one later change.
struct sz21_plan {
    bool use_beam = false;       // the beam sweep (else k_pencil)
    bool segenc = false;         // the packing passes read the sweep's natural-order codes, segment by segment (szh_segenc.h); else block order first, then k_encode / k_encode32
    bool seghist = false;        // small alphabets: a histogram per block column (k_col_hist), from which the columns' bit counts follow without another pass over the codes
    bool dev_book = false;       // the code book on the device (szh_book.h)
    bool sliced = false;         // histogram and block ordering slice by slice beside the running sweep
    int slices_req = 1;
    int se_vw = 1, se_segb = 0, se_nseg = 0, se_nrmax = szh_se::NR; size_t se_tile = 0;      // segments of `se_segb` blocks of a block column
    int sh_rshift = 0;
    // the code book is built and its longest code word known: k_col_encode takes code words of up to 32 bits -- beyond that the block-ordered copy after all
    // (the caller runs permute_all) and the passes that read it
    bool revise(unsigned enc_maxlen) { if (!segenc || enc_maxlen <= 32) return false; segenc = false; seghist = false; return true; }
};
template <class T>
sz21_plan sz21_make_plan(const szhip_ctx *ctx, const szh_geom3 &G, unsigned intervals, size_t reg_count, bool beam_ok, bool overlap, bool feed, size_t meta_len)
{
    sz21_plan P;
    const int64_t n = G.n;
    // Which sweep: the beam takes everything it covers (0.69 ms at 512^3 float; k_pencil's 4.4 / 7.4 ms become 1.2 / 2.3 at 512^3 M-field / the f64 slab), unless the
    // chains run beside k_pencil (`overlap`); SZ_HIP_BEAM=0 switches it off
    P.use_beam = !overlap && beam_ok;
    // (round 6) the packing passes read the sweep's natural-order codes themselves, segment by segment (szh_segenc.h): no block-ordered copy, no k_permute /
    // k_unpred, no cleared stream buffer.  Every 3-D array; whether the code book fits its kernels is known once the tree is built (revise).  SZ_HIP_SEGENC=0: as in round 5.
    // Not for a sweep that is fed while the host's coefficient chains run (the 512^3 M-field): that sweep takes 1.8 ms, the older passes' slices hide beside it, and one
    // call measured 3.04 ms with them against 3.18 with these (SZ_HIP_SEGENC=2 takes them there too).
    const int segenc_sw = tune_int("SZ_HIP_SEGENC", 1);
    P.segenc = G.ndim == 3 && segenc_sw != 0 && (!feed || segenc_sw == 2);
    // the segments' rows, the code table and the bit window (sized here for the longest code words the kernel takes, 32 bits) share the workgroup's LDS.  A tile of
    // 14 KB: k_col_encode needs 75 registers (six wavefronts per SIMD), so the LDS a workgroup takes decides how many columns a CU works on at once -- 512^3,
    // segments of 29 / 22 / 17 / 15 / 11 blocks: 0.251 / 0.220 / 0.206 / 0.224 / 0.253 ms (profiles/r07_packing_rounds.txt)
    P.se_vw = (G.g2.count % 8) == 0 ? 8 : ((G.g2.count % 4) == 0 ? 4 : 1);
    if (P.segenc) {
        bool ok = intervals < 65536 && (double)n < 4.0e9;            // (k_col_encode keeps a row's element offset in 32 bits)
        // every block holds at least 32 codes, so a column's first round (all runs of its first segment, or 256 threads' worth) holds at least 32 code words and
        // never ends inside the column's leading partial word; k_col_encode tells a word shared with the column before by its position all the same.  (3-D arrays of a
        // 2 x 2 cross-section are the only ones this sends to the older passes: a dimension of 1 never comes here.)
        if ((int64_t)G.g0.late * G.g1.late * G.g2.late < 32) ok = false;
        const size_t fixed = ((size_t)intervals + 1) * 8 + 16 + szh_se::seg_window_words(G, 32) * 4 + 64;
        const size_t lds_cap = (size_t)63 * 1024, want = (size_t)std::max(4, tune_int("SZ_HIP_SEG_TILE_KB", 14)) * 1024;
        if (ok && fixed + szh_se::seg_tile_bytes(G, 1, P.se_vw) > lds_cap) ok = false;
        if (ok) {
            const size_t budget = std::min(lds_cap - fixed, std::max(want, szh_se::seg_tile_bytes(G, 1, P.se_vw)));
            int sb = 1;
            while (sb < G.g2.num && szh_se::seg_tile_bytes(G, sb + 1, P.se_vw) <= budget && szh_se::seg_pieces_per_thread(G, sb + 1, P.se_vw) <= (size_t)szh_se::PF) ++sb;
            // segments of equal size, as few as the tile allows: no short segment at the end that pays a whole round's barriers, scan and tile load for a handful of runs
            sb = (G.g2.num + (G.g2.num + sb - 1) / sb - 1) / ((G.g2.num + sb - 1) / sb);
            if (const int f = tune_int("SZ_HIP_SEG_SEGB", 0)) sb = std::max(1, std::min(f, sb));
            P.se_segb = sb;
            P.se_nseg = (G.g2.num + sb - 1) / sb;
            P.se_tile = szh_se::seg_tile_bytes(G, sb, P.se_vw);
            // a round of k_col_encode is 256 threads x up to `se_nrmax` runs (the window is sized for that many): the usual block column's segment in as few rounds as
            // NR allows, its runs spread evenly over them; a column of more rows takes more rounds
            const int rows_typ = (2 * G.g0.split > G.g0.num ? G.g0.early : G.g0.late) * (2 * G.g1.split > G.g1.num ? G.g1.early : G.g1.late);
            const int runs_typ = std::max(1, sb * rows_typ), rounds_typ = (runs_typ + 256 * szh_se::NR - 1) / (256 * szh_se::NR);
            P.se_nrmax = std::max(1, std::min(szh_se::NR, (runs_typ + 256 * rounds_typ - 1) / (256 * rounds_typ)));
            if ((double)G.g0.num * G.g1.num >= 2.0e9) ok = false;
        }
        P.segenc = ok;
    }
    P.seghist = P.segenc && intervals <= SZH_COL_HBINS && tune_int("SZ_HIP_SEGHIST", 1) != 0;
    if (P.seghist) P.sh_rshift = hist_rshift(intervals, 4096);                 // (16 KB of LDS)
    // (SZ_HIP_DEV_BOOK=1, off by default) the code book on the device (szh_book.h): a Lorenzo-only array that takes the packing passes above, their two scans in
    // one launch -- nothing of its entropy stage waits for the host; a book the kernel declines sends the call round again with the host's (with_ticket_fallback)
    P.dev_book = P.segenc && reg_count == 0 && !ctx->no_dev_book && tune_int("SZ_HIP_DEV_BOOK", 0) != 0 && G.g0.num * G.g1.num <= 1024 * SZH_COL_SCAN_PER &&
                 tune_int("SZ_HIP_SEG_SCAN1", 1) != 0 && meta_len + 8 + 4 + sizeof(T) + 1 + sizeof(T) <= 3072;
    // The entropy stage's passes over the code array (histogram, block ordering) start on finished block rows while the beam sweep is still running: every wavefront
    // publishes how many of its lines have their codes in memory (szh_beam.h, `tile_done`: a word per wavefront, written every 32 lines after write-through code stores
    // and a vmcnt(0) -- a system-scope RELEASE per word cost ~35 us each and took the sweep from 1.05 to 1.58 ms); a slice = the block rows whose lines every wavefront
    // has passed.  Measured at 512^3, one call: S-field 2.12 ms unsliced, 1.94 - 1.96 with 3 - 6 slices; M-field 3.94 -> 3.82 (profiles/r05_beam_slices.txt); more slices
    // cost more than they hide (the slices' kernels take 2 - 4 x their lone time beside the sweep).  SZ_HIP_SLICES=1: everything after the sweep.  A lane of a pool
    // (several arrays in flight) takes two slices (SZ_HIP_SLICES_POOL).  Not with the per-column histogram, which runs behind the sweep.
    P.slices_req = tune_int("SZ_HIP_SLICES", ctx->gate ? tune_int("SZ_HIP_SLICES_POOL", 2) : 4);
    P.sliced = P.use_beam && P.slices_req > 1 && !P.seghist;
    return P;
}

// One compress call of the SZ 2.1 path: what its phases share.  compress_impl (below) is the list of the phases; each returns the usual status.
// LIFETIMES.  Host threads work on this object while a call runs: the chain threads and the pool's jobs (run_chains) read and write cf, sec_len, section_failed,
// all_reg_keep, chain_done, chain_avail, chain_t0/1, and call make_section.  The destructor's BODY joins them (as join_sections() does where the header is assembled), so
// every member is still alive then, whichever way the call returns (it also disarms the pool, a no-op on the early returns that never armed it); the members go after
// it, in reverse order of declaration: fed_guard is lowered after the join.
// se_segs, tab_code and tab_len are copied to the device asynchronously and live until the final synchronisation.  The object is neither copied nor moved.
template <class T>
struct sz21_call : call_base {
    static constexpr int is_double = sizeof(T) == 8;
    static constexpr int64_t LINE = 128 / (int64_t)sizeof(T);         // values per 128-byte cache line
    // ---- arguments, geometry
    const szhip_params *const prm; const unsigned char *meta; const size_t meta_len; const int out_on_device; unsigned char **const out; size_t *const out_size;
    const double eb_in; const T eb;
    const bool two_d;                                          // r0 == 0: a 2-D array r1 x r2 (sz_float.c:5516)
    const szh_geom3 G; const int ncoef, ncols; const int64_t n, nb;
    // ---- the SZ_HIP_TIMING trace
    const int tp_on = tune_int("SZ_HIP_TIMING", 0); double tp_t[32]; const char *tp_n[32]; int tp_k = 0;
    // ---- device arrays, the pinned words the fit pass fills
    const T *d_in = nullptr; u64 *sm = nullptr; T *d_coef = nullptr; uint8_t *d_lor = nullptr; uint16_t *d_nat = nullptr, *d_blk = nullptr; unsigned *d_hist = nullptr, *h_hist = nullptr;
    T noise = 0; bool fit_tile = false; int ft_nseg = 0;
    size_t ind_bytes = 0; unsigned char *ind_bits = nullptr; u64 *nreg_h = nullptr, *minmax_h = nullptr;
    // ---- decisions
    unsigned intervals = 0; int use_mean = 0; T mean = 0; size_t reg_count = 0;
    std::vector<unsigned char> meta_own;                       // the parameter bytes as they go into the stream
    sz21_plan P;
    unsigned *tile_done = nullptr; size_t beam_words = 0;      // sliced: the words the beam's wavefronts publish
    int perm_segb = 1, perm_nseg = 1; size_t perm_lds = 0;     // k_permute's tile (prepare_permute)
    // ---- the code book and the stream's layout (host book)
    std::vector<szh_se::seg_t> se_segs; std::vector<u64> tab_code; std::vector<uint8_t> tab_len;
    unsigned enc_maxlen = 0; bool enc32 = false; size_t lds_e32 = 0;
    unsigned char *hdr = nullptr; size_t pre_len = 0, sections_total = 0, hdr_len = 0, unpred_bytes = 0, total_len = 0; u64 total_bits = 0, total_unpred = 0;
    u64 h_small[SM_COUNT];                                     // the device's small words, read after the final synchronisation
    // ---- the coefficient chains: everything the host threads touch (see LIFETIMES)
    szhost_coeffs cf;
    size_t sec_len[4] = {0, 0, 0, 0};           // the coefficient sections (built by the chain threads in the context's PINNED buffers: they go to the device from where they are, beside
                                                // the encoder -- assembling 3.4 MB of them into the header cost 0.2 ms of host copies and 0.1 ms of transfer in front of the encoder at the 512^3 M-field)
    std::vector<std::thread> section_threads;
    std::atomic<int> section_failed{0};
    std::vector<unsigned char> all_reg_keep;   // "every block is a regression block" for the chain over the compacted coefficients
    std::vector<uint32_t> blk_of_rank;
    size_t chain_done[4] = {0, 0, 0, 0};       // regression blocks finished per coefficient (written by the chain threads)
    size_t chain_avail = 0;                    // regression blocks whose coefficients have arrived on the host (read by the chain threads)
    double chain_t0[4] = {0, 0, 0, 0}, chain_t1[4] = {0, 0, 0, 0};   // (SZ_HIP_TIMING: when each chain thread started / finished its chain)
    bool overlap = false, feed = false, two_pieces = false;
    fed_call_guard fed_guard;                   // (lowered when this call returns, whichever way)
    T *hcoef = nullptr;   // pinned: an asynchronous copy to or from pageable memory makes the runtime pin and unpin the pages around it, which was seen to stall later calls for ~20 ms
    bool pool_busy = false;                     // a job of this call is on the context's chain workers
    bool cf_own = false;                        // cf's output arrays belong to the context
    sz21_call(szhip_ctx *c, size_t r0, size_t r1, size_t r2, double eb_, const szhip_params *p, const unsigned char *m, size_t ml, int ood, unsigned char **o, size_t *os)
        : call_base(c), prm(p), meta(m), meta_len(ml), out_on_device(ood), out(o), out_size(os), eb_in(eb_), eb((T)eb_), two_d(r0 == 0),
          G(r0 == 0 ? szh_make_geom2((int)r1, (int)r2) : szh_make_geom3((int)r0, (int)r1, (int)r2)), ncoef(r0 == 0 ? 3 : 4), ncols(G.g0.num * G.g1.num), n(G.n), nb(G.nblocks)
    {
        memset(&cf, 0, sizeof(cf));
        S.n_elements = (uint64_t)n; S.n_blocks = (uint64_t)nb;
    }
    // no return may leave the section threads (or the pool's workers) running on this object, or the pool armed
    ~sz21_call() {
        join_sections();
        if (ctx->chain_pool) ctx->chain_pool->disarm();
        if (cf_own) for (int e = 0; e < 4; ++e) { cf.codes[e] = nullptr; cf.unpred[e] = nullptr; }
        szhost_coeffs_free(&cf);
    }
    void join_sections() {
        for (auto &x : section_threads) if (x.joinable()) x.join();
        if (pool_busy && ctx->chain_pool) { ctx->chain_pool->wait_all(); pool_busy = false; }
    }
    void TP(const char *nm) { if (tp_on && tp_k < 32) { tp_t[tp_k] = now_ms() - t_begin; tp_n[tp_k++] = nm; } }
    void print_trace() const { if (tp_on) { for (int i = 0; i < tp_k; ++i) fprintf(stderr, "%s %.2f | ", tp_n[i], tp_t[i]); fprintf(stderr, "\n"); } }
    // the indicator bits are in scan order (dim 0 outermost), most significant bit first; a set bit = a Lorenzo block
    bool is_lorenzo(int64_t bb) const { return (ind_bits[bb >> 3] >> (7 - (bb & 7))) & 1; }
    size_t count_lorenzo(int64_t bb, int64_t b_end) const {
        size_t ones = 0;
        for (; bb < b_end && (bb & 7); ++bb) ones += is_lorenzo(bb);
        for (; bb + 64 <= b_end; bb += 64) { uint64_t w8; memcpy(&w8, ind_bits + (bb >> 3), 8); ones += (size_t)__builtin_popcountll(w8); }
        for (; bb < b_end; ++bb) ones += is_lorenzo(bb);
        return ones;
    }
    // how far the slowest chain is: regression blocks that every coefficient's chain has finished
    size_t chains_done() const {
        size_t p = reg_count;
        for (int e = 0; e < ncoef; ++e) { const size_t d = __atomic_load_n(&chain_done[e], __ATOMIC_ACQUIRE); if (d < p) p = d; }
        return p;
    }
    int launch_fit(hipStream_t s_, int um, T mn) {
        if (fit_tile) hipLaunchKernelGGL((k_fit_tile<T>), dim3((unsigned)((int64_t)ncols * ft_nseg)), dim3(64), 0, s_, G, d_in, d_coef, d_lor, noise, um, mn, sm + SM_MINMAX, ft_nseg);
        else hipLaunchKernelGGL((k_fit_select<T>), dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s_, G, d_in, d_coef, d_lor, noise, um, mn, sm + SM_MINMAX);
        HIPCHK(hipGetLastError());
        return SZHIP_OK;
    }
    int launch_pack_lor(hipStream_t s_) {
        hipLaunchKernelGGL(k_pack_lor, dim3((unsigned)((ind_bytes + 255) / 256)), dim3(256), 0, s_, (const uint8_t *)d_lor, nb, (uint8_t *)ctx->lor_bits.p, sm + SM_NREG);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ind_bits, ctx->lor_bits.p, ind_bytes, hipMemcpyDeviceToHost, s_));
        HIPCHK(hipMemcpyAsync(nreg_h, sm + SM_NREG, 8, hipMemcpyDeviceToHost, s_));
        return SZHIP_OK;
    }
    // ---- the input staged, the scratch cleared; regression fit + predictor selection on the second stream, overlapped with the interval optimiser.  The pass
    //      needs only the bound -- except for the mean shortcut of the selection, which the optimiser may switch on; it is run WITHOUT it here and repeated in the
    //      (rare) use_mean case (join_fit).
    int stage_and_fit(const void *data, int data_on_device) {
        TRY(stage_input(ctx, data, data_on_device, (size_t)n, &d_in));
        TRY(clear_small(ctx, &sm));
        static const u64 minmax_init[2] = {~0ull, 0ull};          // ordered encodings: the fit pass reduces the array's range into these
        HIPCHK(hipMemcpyAsync(sm + SM_MINMAX, minmax_init, 16, hipMemcpyHostToDevice, st));
        TRY(ensure(ctx, ctx->coef, (size_t)nb * 4 * sizeof(T)));
        TRY(ensure(ctx, ctx->blk_lor, (size_t)nb));
        d_coef = (T *)ctx->coef.p;
        d_lor = (uint8_t *)ctx->blk_lor.p;
        HIPCHK(hipEventRecord(ctx->ev[0], st));
        TP("ev0");
        HIPCHK(hipEventRecord(ctx->ev_in, st));                    // input staged, scratch cleared: the second stream's fit pass may start
        HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_in, 0));
        noise = (T)((double)eb * (two_d ? 0.81 : 1.22));           // sz_float.c:7056 / :5672
        // (round 6) SZ_HIP_FIT_TILE=1: from LDS tiles wherever that form applies (szh_fittile.h: blocks of up to 7, rows on 16-byte boundaries).  Alone it is the faster pass
        // (512^3 float: 0.20 against 0.235 ms), inside a call it is not: the pre-quantisation phase ends with the interval optimiser's sampling pass, which shares the
        // memory system with this one (0.345 against 0.335 ms; the float64 slab 0.81 against 0.76).  Off by default; else one thread per block straight from memory
        fit_tile = !two_d && szh_ft::applies<T>(G, d_in) && tune_int("SZ_HIP_FIT_TILE", 0) != 0;
        ft_nseg = (G.g2.num + szh_ft::shape<T>::SEGB - 1) / szh_ft::shape<T>::SEGB;
        TRY(launch_fit(ctx->stream2, 0, (T)0));
        // the stream's indicator bit array and the regression-block count come from the device (no per-block host loop); they follow the
        // speculative pass on the second stream, so that they are on the host by the time the interval decision is made
        ind_bytes = ((size_t)nb + 7) / 8;
        TRY(ensure(ctx, ctx->lor_bits, ind_bytes + 8));
        TRY(ensure_pinned2(ctx, ind_bytes + 32));                   // pinned: the copies below must not block this thread
        ind_bits = (unsigned char *)ctx->pinned2 + 32;
        nreg_h = (u64 *)ctx->pinned2;
        minmax_h = (u64 *)ctx->pinned2 + 2;
        TRY(launch_pack_lor(ctx->stream2));
        HIPCHK(hipMemcpyAsync(minmax_h, sm + SM_MINMAX, 16, hipMemcpyDeviceToHost, ctx->stream2));
        HIPCHK(hipEventRecord(ctx->ev_fit, ctx->stream2));
        return SZHIP_OK;
    }
    // ---- interval optimiser (round 6 tried two other orders of its passes -- the mean's gather enqueued in front of the fit pass's launches; the sampling pass started before
    //      the mean is known, keeping its sampled values for a small histogram pass --: no faster and slower, profiles/r06_prequant_experiments.txt; removed again)
    int choose_intervals() {
        intervals = prm->quantization_intervals;
        const unsigned max_radius = prm->max_quant_intervals / 2;
        if (intervals == 0) {
            const int64_t md = (int64_t)(int)std::sqrt((double)n);
            // 2-D: a plain stride (sz_float.c:5412-5417): no step-backs
            const szh_meanwalk w = two_d ? szh_make_meanwalk(n, INT64_MAX / 2, INT64_MAX / 2, md) : szh_make_meanwalk(n, G.d0, G.g2.count, md);
            int64_t M = 0, M_hi = n / std::max<int64_t>(md - 2, 1) + 2; // number of strided samples: first m with pos >= n (positions are increasing)
            while (szh_meanwalk_pos(w, M_hi) < n) M_hi *= 2;
            while (M < M_hi) { int64_t mid = (M + M_hi) / 2; if (szh_meanwalk_pos(w, mid) >= n) M_hi = mid; else M = mid + 1; }
            TRY(ensure(ctx, ctx->samples, (size_t)M * sizeof(T)));
            TRY(ensure_pinned(ctx, std::max<size_t>((size_t)M * sizeof(T), (size_t)(max_radius + 8192) * 4 + 64)));
            hipLaunchKernelGGL((k_gather_mean<T>), dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, d_in, w, M, (T *)ctx->samples.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(ctx->pinned, ctx->samples.p, (size_t)M * sizeof(T), hipMemcpyDeviceToHost, st));
            TP("mean enqueued");
            HIPCHK(hipStreamSynchronize(st));
            TP("mean on host");
            double h0 = now_ms();
            const double smean = szhost_seq_mean(is_double, ctx->pinned, (size_t)M);
            host_ms += now_ms() - h0;
            TRY(ensure(ctx, ctx->hist, (size_t)(max_radius + 8192) * 4 + 64));
            unsigned *d_rh = (unsigned *)ctx->hist.p, *d_fh = d_rh + max_radius;
            HIPCHK(hipMemsetAsync(d_rh, 0, (size_t)(max_radius + 8192) * 4, st));
            const int64_t nrows = szh_sample_row_limit(G, prm->sample_distance);
            if (!two_d && (G.g0.count <= 1 || G.g1.count <= 1)) {      // a degenerate 3-D array: the reference's walk, literally (k_sample_walk)
                hipLaunchKernelGGL((k_sample_walk<T, true>), dim3(1), dim3(64), 0, st, G, d_in, prm->sample_distance, (double)eb, (T)smean, max_radius, d_rh, d_fh, sm + SM_WITHIN);
                HIPCHK(hipGetLastError());
            } else if (nrows > 0) {
                int grid = (int)std::min<int64_t>((nrows + 255) / 256, 1024);
                hipLaunchKernelGGL((k_sample<T, true>), dim3(grid), dim3(256), 0, st, G, d_in, nrows, prm->sample_distance, (double)eb, (T)smean, max_radius, d_rh, d_fh, sm + SM_WITHIN);
                HIPCHK(hipGetLastError());
            }
            unsigned *s_hist = (unsigned *)ctx->pinned;
            u64 within = 0;
            HIPCHK(hipMemcpyAsync(s_hist, d_rh, (size_t)(max_radius + 8192) * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(&within, sm + SM_WITHIN, 8, hipMemcpyDeviceToHost, st));
            TP("sample enqueued");
            HIPCHK(hipStreamSynchronize(st));
            TP("sample on host");
            h0 = now_ms();
            u64 sample_count = 0;
            for (unsigned i = 0; i < max_radius; ++i) sample_count += s_hist[i];
            szhost_decision dec;
            szhost_decide(is_double, s_hist, max_radius, s_hist + max_radius, sample_count, within, prm->pred_threshold, (double)eb, smean, &dec);
            host_ms += now_ms() - h0;
            intervals = dec.intervals; use_mean = two_d ? 0 : dec.use_mean;   // 2-D: `use_mean = 0`, sz_float.c:5615
            if (use_mean) {
                T *d_sum = (T *)(sm + SM_MEANSUM);
                hipLaunchKernelGGL((k_mean_seq<T>), dim3(1), dim3(64), 0, st, d_in, n, (T)dec.dense_pos, eb, d_sum, sm + SM_MEANCNT);
                HIPCHK(hipGetLastError());
                T hsum = 0; u64 hcnt = 0;
                HIPCHK(hipMemcpyAsync(&hsum, d_sum, sizeof(T), hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(&hcnt, sm + SM_MEANCNT, 8, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                if (hcnt > 0) mean = hsum / (T)hcnt; // `mean = sum / mean_count`, sz_float.c:6668
            }
        }
        if (intervals > 65536 || intervals < 4) FAIL(SZHIP_ERR_UNSUP, "quantization interval count %u outside [4,65536]", intervals);
        S.intervals = intervals; S.use_mean = use_mean;
        return SZHIP_OK;
    }
    // ---- the fit + selection pass joined (repeated if the selection depends on the mean after all); the range field; SZHIP_CONSTANT
    int join_fit() {
        HIPCHK(hipStreamWaitEvent(st, ctx->ev_fit, 0));
        if (use_mean) {                                            // (the repeated pass: its indicator bits replace the speculative ones)
            TRY(launch_fit(st, use_mean, mean));
            HIPCHK(hipMemsetAsync(sm + SM_NREG, 0, 8, st));
            TRY(launch_pack_lor(st));
            HIPCHK(hipStreamSynchronize(st));
        } else HIPCHK(hipEventSynchronize(ctx->ev_fit));           // usually long done
        TP("fit joined");
        reg_count = (size_t)*nreg_h;
        S.n_reg_blocks = reg_count;
        if (reg_count == 0 && ctx->chain_pool) ctx->chain_pool->disarm();
        // the parameter bytes as they go into the stream: with SZHIP_RANGE_FROM_DATA the range field comes from the fit pass
        // (computeRangeSize_float + `max = min + valueRangeSize`, sz_float.c:2845-2849, in the data's type)
        meta_own.assign(meta, meta + meta_len);
        if (prm->flags & SZHIP_RANGE_FROM_DATA) {
            if (meta_len < 4 + 20 + 2 * sizeof(T)) FAIL(SZHIP_ERR_ARG, "parameter bytes too short for a range field");
            const T lo = (T)ord_dec<T>(minmax_h[0]), hi = (T)ord_dec<T>(minmax_h[1]);
            const T range = hi - lo, top = lo + range;
            unsigned char *q = meta_own.data() + 4 + 20;
            if (is_double) { szhost_put_f64be(q, (double)lo); szhost_put_f64be(q + 8, (double)top); }
            else { szhost_put_f32be(q, (float)lo); szhost_put_f32be(q + 4, (float)top); }
            S.vmin = (double)lo; S.vmax = (double)hi;
            if ((double)range <= eb_in) {          // constant within the bound: the caller's business (a full compression would be thrown away)
                HIPCHK(hipStreamSynchronize(ctx->stream2)); HIPCHK(hipStreamSynchronize(st));
                *out = nullptr; *out_size = 0;
                S.ms_total = now_ms() - t_begin;
                return SZHIP_CONSTANT;
            }
        }
        meta = meta_own.data();
        return SZHIP_OK;
    }
    // a coefficient's section of the stream header (histogram, tree, payload), built by the thread that ran its chain
    void make_section(int e) {
        std::vector<uint32_t> h32(65536, 0);
        for (size_t i = 0; i < reg_count; ++i) h32[(size_t)cf.codes[e][i]]++;
        const huff_ptr ch(szhost_huff_build(131072, h32.data(), nullptr, 65536));
        if (!ch) { section_failed = 1; return; }
        const size_t tb = szhost_huff_tree_size(ch.get());
        const size_t enc_cap = (size_t)((ch->total_bits + 7) / 8) + 16;
        if (sizeof(T) + 12 + tb + 8 + enc_cap + 4 + cf.unpred_count[e] * sizeof(T) > ctx->sec_pin_cap[e]) { section_failed = 1; return; }
        unsigned char *const sec0 = ctx->sec_pin[e];
        unsigned char *q = sec0;
        if (is_double) szhost_put_f64be(q, cf.prec[e]); else szhost_put_f32be(q, (float)cf.prec[e]);
        q += sizeof(T);
        szhost_put_u32be(q, 32768); q += 4;
        szhost_put_u32be(q, (uint32_t)tb); q += 4;
        szhost_put_u32be(q, (uint32_t)ch->n_nodes); q += 4;
        szhost_huff_tree_write(ch.get(), q); q += tb;
        const size_t enc = szhost_huff_encode_i32(ch.get(), cf.codes[e], reg_count, q + 8);
        szhost_put_u64be(q, enc); q += 8 + enc;
        szhost_put_u32be(q, (uint32_t)cf.unpred_count[e]); q += 4;
        memcpy(q, cf.unpred[e], cf.unpred_count[e] * sizeof(T)); q += cf.unpred_count[e] * sizeof(T);
        sec_len[e] = (size_t)(q - sec0);
    }
    // ---- regression coefficient chain (a serial recurrence with reconstruction feedback: host) and its Huffman streams.
    //      The chains of the four (three) coefficients are independent of each other and each is bound by the latency of its own
    //      ~45-cycle dependence per block, so they run on one host thread each; a thread goes on to build its coefficient's section
    //      of the stream header while the sweep is already running on the decoded values.
    //      Here: the sections' buffers, the coefficients ranked and gathered, and how the chains overlap with the sweep (`overlap`, `feed`).
    int prepare_chains() {
        // the sections' buffers, sized for the worst case (a tree of every possible symbol, 64-bit codes, every coefficient verbatim) before any thread writes
        for (int e = 0; e < ncoef; ++e) {
            const size_t bound = sizeof(T) + 12 + (13 * 2 * std::min<size_t>(reg_count, 65536) + 16) + 8 + (8 * reg_count + 16) + 4 + reg_count * sizeof(T) + 64;
            if (ctx->sec_pin_cap[e] < bound) {
                HIPCHK(hipStreamSynchronize(ctx->stream2)); HIPCHK(hipStreamSynchronize(st));
                if (ctx->sec_pin[e]) { HIPCHK(hipHostFree(ctx->sec_pin[e])); ctx->sec_pin[e] = nullptr; ctx->sec_pin_cap[e] = 0; }
                HIPCHK(hipHostMalloc((void **)&ctx->sec_pin[e], bound + bound / 8, hipHostMallocDefault));
                ctx->sec_pin_cap[e] = bound + bound / 8;
            }
        }
        // only the regression blocks' coefficients travel: rank them in scan order, gather [4][reg_count], chain on the host
        // (the compact arrays are "all regression blocks" to the chain), scatter the decoded values back
        TRY(ensure(ctx, ctx->reg_flags, (size_t)nb * 8));
        TRY(ensure(ctx, ctx->reg_rank, (size_t)nb * 8));
        TRY(ensure(ctx, ctx->coef_compact, reg_count * 4 * sizeof(T)));
        hipLaunchKernelGGL(k_reg_flags, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_lor, nb, (u64 *)ctx->reg_flags.p);
        TRY(scan_u64(ctx, (const u64 *)ctx->reg_flags.p, nb, (u64 *)ctx->reg_rank.p, sm + SM_SCRATCH));
        hipLaunchKernelGGL((k_move_coef<T, 0>), dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_lor, (const u64 *)ctx->reg_rank.p, nb, (int64_t)reg_count, d_coef, (T *)ctx->coef_compact.p);
        HIPCHK(hipGetLastError());
#ifndef SZH_SYNC_LAUNCH
        // (not in a pool lane: with several contexts at work the hand-off of coefficients to the running kernel failed 5 - 6 times in 480
        //  rounds of tools/gpu_pool_dbg.py -- errors, not wrong streams; none in 480 rounds with the serial order.  The lanes overlap one
        //  array's chain with the other's kernels anyway.
        //  A lone context takes the overlap only when no other compress call of the process is under way as this one starts.)
        overlap = !beam_applies<T>(G, d_in, reg_count) && !two_d && !ctx->gate && !ctx->no_chain_overlap && g_compress_calls.load() <= 1;
        if (overlap) { TRY(probe_streams(ctx)); overlap = ctx->streams_independent == 1; }
#endif
        // (round 5) the beam sweep FED while it runs: the chains deliver block rows in the order the beam's planes need them, so the sweep is launched
        // as soon as the chains start, k_reg_points follows them slice by slice on the second stream, and the sweep waits per plane (szh_beam.h,
        // wait_fed).  Same conditions as the older overlap (a lone call, streams on different hardware queues), planes of whole cache lines, and the
        // chains on the context's persistent threads.  A sweep that is not fed in time gives up and the call is repeated with the chains first.
        // Only where the chains are long (>= 65536 regression blocks = 0.25 ms): with a short chain there is nothing to hide, and the slices' kernels beside
        // the sweep cost more than they save (BASELINE configs[3]'s float64 slab, a few thousand regression blocks: 4.24 ms unfed, 5.36 fed).
        feed = beam_applies<T>(G, d_in, reg_count) && !ctx->gate && !ctx->no_chain_overlap && g_compress_calls.load() <= 1 && tune_int("SZ_HIP_BEAM_FEED", 1) &&
               G.g0.num >= 2 && reg_count >= (size_t)tune_int("SZ_HIP_FEED_MIN_REG", 65536);
#ifndef SZH_SYNC_LAUNCH
        feed = feed && (G.d0 % 128) == 0;      // (a plane = whole cache lines of values, flags and codes: a line is never loaded while part of it is still to come)
        if (feed) { TRY(probe_streams(ctx)); feed = ctx->streams_independent == 1; }
#endif
        if (feed) feed = fed_guard.try_raise();      // (no other lone context's call may join this one half-way: szhip.hip, fed_call_guard)
        TRY(ensure_pinned3(ctx, reg_count * 4 * sizeof(T) + (overlap ? ((size_t)nb + 64) * 4 * sizeof(T) + 256 : 0)));
        hcoef = (T *)ctx->pinned3;
        return SZHIP_OK;
    }
    // ---- the coefficients to the host and the chains started: on threads of this call beside k_pencil (`overlap`), else on the context's pool -- beside the fed
    //      sweep (`feed`), or finished here and scattered back to the device
    int run_chains() {
        // (round 5, with the fed sweep) the chains start on the FIRST 32768 coefficients of every array while the rest is still on its way (4.8 MB at the
        // 512^3 M-field: 0.1 ms): chain_avail says how many have arrived, a chain that runs into the mark waits (szhost_coeff_chain_one_pa)
        chain_avail = reg_count;
        struct AvailAll {      // (no return path may leave a chain waiting for coefficients that never come: released when this phase ends, before anything waits for the chains)
            size_t *p; size_t v;
            ~AvailAll() { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
        } avail_all{&chain_avail, reg_count};
        const size_t first_piece = (size_t)std::max(1, tune_int("SZ_HIP_CHAIN_EARLY_PIECE", 32768));
        two_pieces = feed && reg_count >= 4 * first_piece;
        if (two_pieces) {
            for (int e = 0; e < 4; ++e)
                HIPCHK(hipMemcpyAsync(hcoef + (size_t)e * reg_count, (const T *)ctx->coef_compact.p + (size_t)e * reg_count, first_piece * sizeof(T), hipMemcpyDeviceToHost, st));
            HIPCHK(hipEventRecord(ctx->ev_sec, st));
            for (int e = 0; e < 4; ++e)
                HIPCHK(hipMemcpyAsync(hcoef + (size_t)e * reg_count + first_piece, (const T *)ctx->coef_compact.p + (size_t)e * reg_count + first_piece, (reg_count - first_piece) * sizeof(T), hipMemcpyDeviceToHost, st));
            chain_avail = 0;
            HIPCHK(hipEventSynchronize(ctx->ev_sec));
            __atomic_store_n(&chain_avail, first_piece, __ATOMIC_RELEASE);
        } else {
            HIPCHK(hipMemcpyAsync(hcoef, ctx->coef_compact.p, reg_count * 4 * sizeof(T), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        TP("coef on host");
        double h0 = now_ms();
        all_reg_keep.assign(reg_count, 0);
        TP("chain begin");
        const unsigned char *const ind = all_reg_keep.data();
        // 2-D planes are carried as {0, a, b, c}: the chain sees components 1..3
        T *const chain_in = hcoef + (two_d ? reg_count : 0);
        szhost_coeff_chain_begin(is_double, ind, reg_count, (double)eb, G.g0.late, G.g1.late, G.g2.late, ncoef, &cf);
        // the chains write into the context's arrays (touched in earlier calls) instead of freshly allocated ones
        if (ctx->chain_codes.size() < reg_count * 4) ctx->chain_codes.resize(reg_count * 4 + reg_count / 4);
        if (ctx->chain_unpred.size() < reg_count * 4 * sizeof(T)) ctx->chain_unpred.resize((reg_count * 4 + reg_count / 4) * sizeof(T));
        for (int e = 0; e < 4; ++e) {
            free(cf.codes[e]); free(cf.unpred[e]);
            cf.codes[e] = ctx->chain_codes.data() + (size_t)e * reg_count;
            cf.unpred[e] = ctx->chain_unpred.data() + (size_t)e * reg_count * sizeof(T);
        }
        cf_own = true;
        // (threads also for a handful of regression blocks: a section's fixed cost -- a 131 072-state code book -- is ~0.5 ms, and
        //  four of them in line delayed the wavefront kernel of BASELINE configs[3] by 2 ms)
        if (overlap) {
            // The chain runs NEXT TO the wavefront kernel: the threads publish how far they are, the kernel is launched right away and
            // makes a pencil that touches a regression block wait until the blocks it reads are final, and this thread ships the decoded
            // coefficients as they appear (ship_coefs).  blk_of_rank: scan-order block index of the r-th regression block.
            blk_of_rank.resize(reg_count);
            size_t r = 0;
            for (int64_t bb = 0; bb < nb && r < reg_count; ++bb) if (!is_lorenzo(bb)) blk_of_rank[r++] = (uint32_t)bb;
            if (r != reg_count) FAIL(SZHIP_ERR_INTERNAL, "indicator bits and regression-block count disagree");
            for (int e = 0; e < 4; ++e) chain_done[e] = 0;
            for (int e = 0; e < ncoef; ++e)
                section_threads.emplace_back([this, e, chain_in, ind] {
                    szhost_coeff_chain_one_p(is_double, chain_in, ind, reg_count, use_mean, e, &cf, &chain_done[e]);
                    make_section(e);
                });
        } else {
            if (!ctx->chain_pool) { ctx->chain_pool = new szhip_chain_pool(); ctx->chain_pool->start(); }
            pool_busy = true;
            for (int e = 0; e < 4; ++e) chain_done[e] = feed && e >= ncoef ? reg_count : 0;
            const size_t *const avail_ptr = two_pieces ? &chain_avail : nullptr;
            ctx->chain_pool->submit(ncoef, [this, chain_in, ind, avail_ptr](int e) {
                    chain_t0[e] = now_ms() - t_begin;
                    szhost_coeff_chain_one_pa(is_double, chain_in, ind, reg_count, use_mean, e, &cf, feed ? &chain_done[e] : nullptr, avail_ptr);
                    chain_t1[e] = now_ms() - t_begin;
                }, [this](int e) { make_section(e); });
            if (two_pieces) {                          // the rest of the coefficients: the chains are at work meanwhile
                HIPCHK(hipStreamSynchronize(st));
                __atomic_store_n(&chain_avail, reg_count, __ATOMIC_RELEASE);
            }
            if (!feed) ctx->chain_pool->wait_chains();           // the decoded coefficients are final: the main thread may ship them (the sections follow on the workers)
        }
        if (!feed) host_ms += now_ms() - h0;
        TP("chain done");
        if (tp_on) fprintf(stderr, "chain threads: %.2f-%.2f %.2f-%.2f %.2f-%.2f %.2f-%.2f | ", chain_t0[0], chain_t1[0], chain_t0[1], chain_t1[1], chain_t0[2], chain_t1[2], chain_t0[3], chain_t1[3]);
        if (!overlap && !feed) {
            HIPCHK(hipMemcpyAsync(ctx->coef_compact.p, hcoef, reg_count * 4 * sizeof(T), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL((k_move_coef<T, 1>), dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_lor, (const u64 *)ctx->reg_rank.p, nb, (int64_t)reg_count, d_coef, (T *)ctx->coef_compact.p);
            HIPCHK(hipGetLastError());
        }
        return SZHIP_OK;
    }
    // the feed of the beam sweep (prepare_chains): slices of block rows; a slice goes out when every chain has passed its last regression block
    int feed_slices(const szh_qargs<T> &a) {
        const double h1 = now_ms();
        const int NF = std::max(2, std::min(G.g0.num, 12));
        const int64_t per_row = (int64_t)G.g1.num * G.g2.num;
        size_t r_lo = 0; int b0_lo = 0;
        for (int sl = 0; sl < NF; ++sl) {
            const int b0_hi = sl == NF - 1 ? G.g0.num : std::max(b0_lo, (int)((int64_t)G.g0.num * (sl + 1) / NF));
            if (b0_hi == b0_lo && sl != NF - 1) continue;
            // regression blocks in block rows below b0_hi
            size_t r_hi = reg_count;
            if (b0_hi < G.g0.num) r_hi = r_lo + ((size_t)(b0_hi - b0_lo) * per_row - count_lorenzo(b0_lo * per_row, b0_hi * per_row));
            unsigned idle = 0;
            while (chains_done() < r_hi) {
                szhip_chain_pool::pause();
                if (++idle > (1u << 28)) FAIL(SZHIP_ERR_INTERNAL, "coefficient chain made no progress");
            }
            const int planes_end = b0_hi >= G.g0.num ? G.g0.count : szh_blk_start(G.g0, b0_hi);
            // (2-D never comes here; the compact arrays are [4][reg_count], the chains decoded them in place)
            TRY((feed_beam_slice<T>(ctx, G, a, ctx->stream2, hcoef, reg_count, r_lo, r_hi, b0_lo, b0_hi, planes_end, (const u64 *)ctx->reg_rank.p, nb)));
            r_lo = r_hi; b0_lo = b0_hi;
        }
        host_ms += now_ms() - h1;
        S.chain_overlapped = 2;
        return SZHIP_OK;
    }
    // `overlap`: ship the decoded coefficients while k_pencil runs: DMA only (no kernel that could queue behind the waiting tiles), on the
    // second stream, in scan order: the values of the newly finished regression blocks go into a block-indexed pinned staging
    // array, the contiguous block range [first, last] of each coefficient into `dec`, then the progress word (same stream: it
    // lands after the data).  Blocks between regression blocks are Lorenzo blocks: whatever they receive is never read.
    int ship_coefs(unsigned epoch, szh_u64 *coh_prog, T *dec, int64_t nbp) {
        const double h1 = now_ms();
        const szh_u64 tag = (szh_u64)(epoch & 0xffffffu) << 40;
        T *const full = (T *)(((uintptr_t)(hcoef + reg_count * 4) + 127) & ~(uintptr_t)127);     // pinned staging, [4][nbp] block-indexed
        const size_t chunk = std::max<size_t>(2048, reg_count / 32);
        size_t shipped = 0; int64_t sent = 0;                 // ranks scattered into the staging array; blocks [0, sent) are on the device
        int idle = 0;
        while (sent < nb) {
            const size_t p = chains_done();
            if (p > shipped && (p - shipped >= chunk || p == reg_count)) {
                for (int e = 0; e < ncoef; ++e)
                    for (size_t r = shipped; r < p; ++r) full[(size_t)e * nbp + blk_of_rank[r]] = hcoef[(size_t)e * reg_count + r];
                shipped = p;
                // every block below `fin` is final; whole lines of them travel
                const int64_t fin = p == reg_count ? nb : (int64_t)blk_of_rank[p];
                const int64_t upto = fin == nb ? nb : fin / LINE * LINE;
                if (upto > sent) {
                    for (int e = 0; e < ncoef; ++e)
                        HIPCHK(hipMemcpyAsync(dec + (size_t)e * nbp + sent, full + (size_t)e * nbp + sent, (size_t)(upto - sent) * sizeof(T), hipMemcpyHostToDevice, ctx->stream2));
                    HIPCHK(hipStreamSynchronize(ctx->stream2));            // the values are in device memory ...
                    __atomic_store_n(coh_prog, tag | (szh_u64)upto, __ATOMIC_RELEASE);   // ... before the kernel may look for them
                    sent = upto;
                }
                idle = 0;
            } else if (++idle > 200000) FAIL(SZHIP_ERR_INTERNAL, "coefficient chain made no progress");
            else std::this_thread::sleep_for(std::chrono::microseconds(10));
        }
        host_ms += now_ms() - h1;
        S.chain_overlapped = 1;
        TP("coefficients shipped");
        return SZHIP_OK;
    }
    // ---- predict + quantise: the sweep (beam or k_pencil), and what feeds it while it runs
    int launch_sweep() {
        TRY(ensure(ctx, ctx->codes_nat, (size_t)n * 2 + 64));
        TRY(ensure(ctx, ctx->codes_blk, (size_t)n * 2 + 64));
        d_nat = (uint16_t *)ctx->codes_nat.p; d_blk = (uint16_t *)ctx->codes_blk.p;
        int nI, nJ, ntiles;
        using TS = szh_tile_shape<T>;
        TRY(prepare_pencil(ctx, G, szh_gran<T>::NW, TS::TPI, TS::TPJ, &nI, &nJ, &ntiles));
        const szh_bm::grid_t bgrid = szh_bm::make_grid(G);
        beam_words = (size_t)bgrid.nKB * bgrid.nJG * szh_bm::WPG;
        if (P.sliced) {
            TRY(ensure_coherent(ctx, 512 + beam_words * 4));
            tile_done = (unsigned *)((char *)ctx->coh + 512);
            if (!ctx->stream3) HIPCHK(hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking));
            if (!ctx->ev_perm) HIPCHK(hipEventCreateWithFlags(&ctx->ev_perm, hipEventDisableTiming));
        }
        szh_qargs<T> a; memset(&a, 0, sizeof(a));
        a.tile_done = tile_done; a.pub_lines = 32;
        a.G = G; a.data = d_in; a.out = nullptr; a.codes = d_nat; a.blk_lor = d_lor; a.coef = d_coef; a.coef_stride = nb;
        a.eb = eb; a.recip = 1 / eb; a.mean = mean; a.cap = (int)intervals; a.radius = (int)intervals / 2; a.use_mean = use_mean;
        a.faceI = (szh_u64 *)ctx->faceI.p; a.faceJ = (szh_u64 *)ctx->faceJ.p; a.epoch = ++ctx->epoch;
        a.nI = nI; a.nJ = nJ; a.order = (const unsigned *)ctx->order.p; a.no_reg = reg_count == 0;
        a.ticket = (unsigned *)(sm + SM_TICKET); a.err = (unsigned *)(sm + SM_ERR); a.ticket_mode = ctx->ticket_atomic ? 0 : tune_int("SZ_HIP_TICKET_MODE", 2);
        a.progress = (szh_u64 *)ctx->progress.p; a.backoff = SZH_FILL_BACKOFF; a.wide = pencil_wide<T>(G, nJ);
        a.coef_progress = nullptr;
        szh_u64 *coh_prog = nullptr;
        T *dec = nullptr;                                          // the decoded coefficients as the kernel reads them
        const int64_t nbp = (nb + LINE - 1) / LINE * LINE;         // a coefficient's array starts on a line boundary
        if (overlap) {
            // Hand-off between the host's chain and the running kernel (per-XCD L2s are not coherent, and DMA writes do not touch them):
            //  * the progress word lives in HOST-COHERENT pinned memory (uncached on the GPU; the kernel polls it over PCIe).  In device
            //    memory a poll leaves the line in that XCD's L2 and every later poll finds the old value -- seen as a pencil that never saw
            //    the word the memory held.  It carries the launch epoch, so it is never cleared;
            //  * the coefficients go by DMA into a device buffer that no kernel ever stores to (reading them over PCIe was 45 ms: every lane
            //    of a block's rows reads them).  A line of it must never be loaded while only part of it is final -- the rest would stay
            //    stale in that L2 -- so progress is published in whole 128-byte lines of blocks, every coefficient array is line-aligned,
            //    and a pencil only loads below the published mark.  Lines of an earlier launch are gone at kernel start.
            TRY(ensure_coherent(ctx, 256));
            TRY(ensure(ctx, ctx->coef_dec, (size_t)nbp * 4 * sizeof(T)));
            coh_prog = (szh_u64 *)ctx->coh;
            dec = (T *)ctx->coef_dec.p;
            a.coef_progress = coh_prog;
            a.coef = dec; a.coef_stride = nbp;
        }
        HIPCHK(hipEventRecord(ctx->ev[2], st));
        if (P.use_beam) {
#ifdef SZH_SYNC_LAUNCH
            // (the CPU shim runs a launch to its end before the next one starts: the slices first, then a sweep that finds every plane there)
            if (feed) {
                TRY(ensure(ctx, ctx->pt_flags, (size_t)G.n + 64)); TRY(ensure(ctx, ctx->rb_vals, (size_t)G.n * sizeof(T) + 64)); TRY(ensure(ctx, ctx->feed_word, 256));
                HIPCHK(hipMemsetAsync(ctx->pt_flags.p, 0, (size_t)G.n, st));
                TRY(feed_slices(a));
                TRY((launch_beam<T, false>(ctx, G, a, st, reg_count, true)));
            } else
#endif
            TRY((launch_beam<T, false>(ctx, G, a, st, reg_count, feed)));
            S.quant_kernel = 2;
#ifndef SZH_SYNC_LAUNCH
            if (feed) TRY(feed_slices(a));
#endif
        } else {
            const unsigned pgrid = pencil_grid(ctx, a, ntiles);
            hipLaunchKernelGGL((k_pencil<T, false>), dim3(pgrid), dim3((TS::TPI * TS::TPJ + 2) * 64), 0, st, a);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ctx->ev[3], st));
        TP("pencil launched");
        S.quant_kernel_launches = 1;
        if (overlap) TRY(ship_coefs(a.epoch, coh_prog, dec, nbp));
        return SZHIP_OK;
    }
    // the histogram of the whole code array (and its copy to the host) on the second stream, next to the block-ordering pass: the host builds the code book while
    // k_permute is still running.  (The histogram inside k_permute instead measured equal in kernel time -- 393 against 322 + 69 us -- and lost the overlap.)
    int launch_hist() {
        HIPCHK(hipEventRecord(ctx->ev_in, st));                    // codes complete
        HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_in, 0));
        HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)intervals * 4, ctx->stream2));
        TRY(launch_hist_u16(ctx, ctx->stream2, d_nat, 0, n, intervals, d_hist));
        HIPCHK(hipMemcpyAsync(h_hist, d_hist, (size_t)intervals * 4, hipMemcpyDeviceToHost, ctx->stream2));
        HIPCHK(hipEventRecord(ctx->ev_fit, ctx->stream2));
        return SZHIP_OK;
    }
    // k_permute's tile: blocks per segment, segments per column, the zero-code lists per segment, the dynamic LDS
    int prepare_permute() {
        perm_segb = choose_segb(G, 2, SZH_PERM_TILE_BYTES);
        perm_nseg = (G.g2.num + perm_segb - 1) / perm_segb;
        TRY(ensure(ctx, ctx->zcnt, (size_t)ncols * perm_nseg * 4));
        TRY(ensure(ctx, ctx->zpos, (size_t)ncols * perm_nseg * SZH_ZCAP * 4));
        const size_t tile_el = (tile_bytes(G, perm_segb, 2) + 1) / 2;
        perm_lds = ((tile_el + 1) & ~(size_t)1) * 2 + 16;
        return SZHIP_OK;
    }
    // the block-ordering pass over block columns [col0, col0 + cols) on stream `s_`
    void launch_permute(hipStream_t s_, int col0, int cols) {
        hipLaunchKernelGGL((k_permute<0>), dim3((unsigned)cols, std::min(perm_nseg, std::max(1, tune_int("SZ_HIP_PERM_Y", 1)))), dim3(256), perm_lds, s_, G, (const uint16_t *)d_nat, d_blk,
                           (unsigned *)ctx->col_zeros.p, perm_segb, (unsigned *)ctx->zcnt.p, (unsigned *)ctx->zpos.p, col0);
    }
    // the columns' zero-code counts -> where each column's unpredictable values start
    int scan_col_zeros(hipStream_t s_) {
        hipLaunchKernelGGL(k_u32_to_u64, dim3((ncols + 255) / 256), dim3(256), 0, s_, (const unsigned *)ctx->col_zeros.p, (int64_t)ncols, (u64 *)ctx->col_zeros64.p);
        return scan_u64(ctx, (const u64 *)ctx->col_zeros64.p, ncols, (u64 *)ctx->col_off.p, sm + SM_TOTAL_UNPRED, s_);
    }
    // the block-ordering pass over the whole array, on the first stream (arrays whose sweep feeds no slices; with segenc: only if the code book turns out not to fit its kernels)
    int permute_all() {
        HIPCHK(hipMemsetAsync(ctx->col_zeros.p, 0, (size_t)ncols * 4, st));
        TRY(prepare_permute());
        launch_permute(st, 0, ncols);
        HIPCHK(hipGetLastError());
        return scan_col_zeros(st);
    }
    // slices of block rows (dim 0) beside the running beam sweep: the codes are in natural order, so a slice's codes are ONE contiguous range for the histogram, and the
    // block-ordering pass takes the slice's block rows.  A slice starts when every wavefront of the sweep has published its lines.
    int hist_and_order_sliced() {
        const int NS = std::min(P.slices_req, G.g0.num);
        TRY(prepare_permute());
        HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)intervals * 4, ctx->stream2));
        HIPCHK(hipMemsetAsync(ctx->col_zeros.p, 0, (size_t)ncols * 4, ctx->stream3));
        const unsigned tag = (ctx->epoch & 0xfffu) << 20;
        bool sweep_over = false;
        int b0_done = 0;
        int64_t hist_first = 0;
        for (int sl = 0; sl < NS; ++sl) {
            const int b0_hi = sl == NS - 1 ? G.g0.num : std::max(b0_done, (int)((int64_t)G.g0.num * (sl + 1) / NS));
            const int rows_need = b0_hi >= G.g0.num ? G.g0.count : szh_blk_start(G.g0, b0_hi);
            size_t first_late = 0;                                     // wavefronts below this index have been seen past the current slice's rows
            unsigned spins = 0;
            while (!sweep_over && first_late < beam_words) {
                const unsigned wv = __atomic_load_n(&tile_done[first_late], __ATOMIC_ACQUIRE);
                if ((wv & 0xfff00000u) == tag && (int)(wv & 0xfffffu) >= rows_need) { ++first_late; continue; }
                szhip_chain_pool::pause();
                if ((++spins & 127u) == 0) {
                    const hipError_t q = hipEventQuery(ctx->ev[3]);
                    if (q == hipSuccess) { sweep_over = true; break; }
                    if (q != hipErrorNotReady) HIPCHK(q);
                }
            }
            if (b0_hi > b0_done) {
                // (k_hist_u16 counts groups of eight codes: a slice of it ends on a multiple of eight below the slice's last code, the last slice takes the rest)
                const int64_t h_lo = hist_first, h_hi = b0_hi >= G.g0.num ? (int64_t)n : ((int64_t)rows_need * G.d0) / 8 * 8;
                hist_first = h_hi;
                if (h_hi > h_lo) TRY(launch_hist_u16(ctx, ctx->stream2, d_nat, h_lo, h_hi, intervals, d_hist));
                if (!P.segenc) launch_permute(ctx->stream3, b0_done * G.g1.num, (b0_hi - b0_done) * G.g1.num);
                HIPCHK(hipGetLastError());
                b0_done = b0_hi;
            }
        }
        HIPCHK(hipMemcpyAsync(h_hist, d_hist, (size_t)intervals * 4, hipMemcpyDeviceToHost, ctx->stream2));
        HIPCHK(hipEventRecord(ctx->ev_fit, ctx->stream2));
        if (!P.segenc) TRY(scan_col_zeros(ctx->stream3));
        HIPCHK(hipEventRecord(ctx->ev_perm, ctx->stream3));
        return SZHIP_OK;
    }
    // ---- histogram, block ordering, unpredictable counts
    int hist_and_order() {
        TRY(ensure(ctx, ctx->hist, (size_t)(65536 + 8192) * 4 + 64));
        d_hist = (unsigned *)ctx->hist.p;
        TRY(ensure_pinned(ctx, (size_t)intervals * 4 + 64));
        h_hist = (unsigned *)ctx->pinned;
        if (P.seghist) {
            // (behind the sweep, on its stream: beside it the pass took from the sweep what it saved behind it -- 512^3: sweep 0.70 -> 0.76 ms with four slices of the older histogram)
            TRY(ensure(ctx, ctx->seg_hist, (size_t)ncols * intervals * 4));
            HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)intervals * 4, st));
            hipLaunchKernelGGL(k_col_hist, dim3((unsigned)ncols), dim3(256), ((size_t)intervals * 4) << P.sh_rshift, st, G, (const uint16_t *)d_nat, intervals, P.sh_rshift, P.se_vw, (unsigned *)ctx->seg_hist.p);
            hipLaunchKernelGGL(k_hist_reduce, dim3((unsigned)std::min<int64_t>(64, ncols)), dim3(256), 0, st, (const unsigned *)ctx->seg_hist.p, intervals, (int64_t)ncols, d_hist);
            HIPCHK(hipGetLastError());
            if (!P.dev_book) {
                HIPCHK(hipMemcpyAsync(h_hist, d_hist, (size_t)intervals * 4, hipMemcpyDeviceToHost, st));
                HIPCHK(hipEventRecord(ctx->ev_fit, st));
            }
        } else if (!P.sliced) TRY(launch_hist());                  // next to the block-ordering pass
        TRY(ensure(ctx, ctx->col_zeros, (size_t)ncols * 4));
        TRY(ensure(ctx, ctx->col_zeros64, (size_t)ncols * 8));
        TRY(ensure(ctx, ctx->col_off, (size_t)ncols * 8));
        if (P.sliced) TRY(hist_and_order_sliced());
        else if (!P.segenc) TRY(permute_all());
        return SZHIP_OK;
    }
    // the stream header's fixed front: the parameter bytes, n, the block size, the bound
    unsigned char *put_front(unsigned char *q) const {
        memcpy(q, meta, meta_len); q += meta_len;
        szhost_put_u64be(q, (uint64_t)n); q += 8;
        szhost_put_u32be(q, (uint32_t)G.block_size); q += 4;
        if (is_double) szhost_put_f64be(q, (double)eb); else szhost_put_f32be(q, (float)eb);
        return q + sizeof(T);
    }
    // the segments' geometry, the same for every column (k_col_encode reads it instead of working it out)
    int upload_segments() {
        se_segs.resize((size_t)P.se_nseg);
        for (int q = 0; q < P.se_nseg; ++q) se_segs[(size_t)q] = szh_se::make_seg(G, 1, q, P.se_segb, P.se_vw);
        TRY(ensure(ctx, ctx->seg_tab, se_segs.size() * sizeof(szh_se::seg_t)));
        HIPCHK(hipMemcpyAsync(ctx->seg_tab.p, se_segs.data(), se_segs.size() * sizeof(szh_se::seg_t), hipMemcpyHostToDevice, st));
        return SZHIP_OK;
    }
    // The packing passes on natural-order codes (szh_segenc.h): bits and zero codes per block column, their offsets (the scan also clears the words at the column
    // boundaries), then k_col_encode.  `base_bits`: where the payload starts in `d_stream`; `d_plan`: the device code book's plan, which says so instead (szh_book.h);
    // `maxlen`: the longest code word, for the bit window.  `between` enqueues what writes the stream in front of the payload: behind the scan, because the first word
    // it clears may begin with the header's (or the unpredictable values') last bytes.
    template <class F>
    int pack_columns(unsigned char *d_stream, u64 base_bits, const u64 *d_plan, unsigned maxlen, F &&between) {
        const int64_t nent = (int64_t)ncols;
        TRY(ensure(ctx, ctx->seg_bits, (size_t)nent * 8)); TRY(ensure(ctx, ctx->seg_zeros, (size_t)nent * 8));
        TRY(ensure(ctx, ctx->seg_bitoff, (size_t)nent * 8)); TRY(ensure(ctx, ctx->seg_zoff, (size_t)nent * 8));
        u64 *const bits = (u64 *)ctx->seg_bits.p, *const zeros = (u64 *)ctx->seg_zeros.p, *const bitoff = (u64 *)ctx->seg_bitoff.p, *const zoff = (u64 *)ctx->seg_zoff.p;
        const size_t lb = intervals <= 16384 ? (size_t)intervals : 16;
        if (P.seghist) hipLaunchKernelGGL(k_col_bits_h, dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, st, (const unsigned *)ctx->seg_hist.p, (const uint8_t *)ctx->len_tab.p, intervals, nent, bits, zeros);
        else hipLaunchKernelGGL(k_col_bits, dim3((unsigned)nent), dim3(256), lb, st, G, (const uint16_t *)d_nat, (const uint8_t *)ctx->len_tab.p, intervals, P.se_vw, bits, zeros);
        if (nent <= 1024 * SZH_COL_SCAN_PER && tune_int("SZ_HIP_SEG_SCAN1", 1))
            hipLaunchKernelGGL(k_col_scan, dim3(1), dim3(1024), 0, st, (const u64 *)bits, (const u64 *)zeros, (int)nent, bitoff, zoff, sm + SM_TOTAL_BITS, sm + SM_TOTAL_UNPRED, base_bits, (unsigned *)d_stream, d_plan);
        else {
            TRY(scan_u64(ctx, (const u64 *)bits, nent, bitoff, sm + SM_TOTAL_BITS));
            TRY(scan_u64(ctx, (const u64 *)zeros, nent, zoff, sm + SM_TOTAL_UNPRED));
            hipLaunchKernelGGL(k_col_bounds, dim3((unsigned)((nent + 1 + 255) / 256)), dim3(256), 0, st, (const u64 *)bitoff, nent, (const u64 *)(sm + SM_TOTAL_BITS), base_bits, (unsigned *)d_stream);
        }
        HIPCHK(hipGetLastError());
        TRY(between());
        const unsigned win = (unsigned)szh_se::seg_window_words(G, std::max(1u, maxlen), P.se_nrmax);
        const size_t lds = ((size_t)intervals + 1) * 8 + P.se_tile + 16 + (size_t)win * 4;
        auto encode = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)nent), dim3(256), lds, st, G, (const uint16_t *)d_nat, (const u64 *)ctx->code_tab.p, intervals, (const szh_se::seg_t *)ctx->seg_tab.p, P.se_nseg, P.se_vw,
                               P.se_nrmax, P.se_tile, win, (const u64 *)bitoff, (const u64 *)zoff, base_bits, (unsigned *)d_stream, d_in, (T *)ctx->unpred.p, d_plan);
        };
        if (G.g2.num >= 2 && G.g2.early <= szh_se::INNER && G.g2.late >= szh_se::INNER - 1) encode(k_col_encode<T, true>);
        else encode(k_col_encode<T, false>);
        HIPCHK(hipGetLastError());
        return SZHIP_OK;
    }
    // ---- the end of every call: the sweep's and the packing passes' words read back, checked behind the final synchronisation, the stream delivered, the statistics
    int enqueue_readback() {
        HIPCHK(hipEventRecord(ctx->ev[4], st));
        TP("encode launched");
        HIPCHK(hipMemcpyAsync(h_small, sm, SM_COUNT * 8, hipMemcpyDeviceToHost, st));
        return SZHIP_OK;
    }
    // after the final synchronisation: the wavefront kernel's error flag; the device book's verdict (`declined`, with its status; the caller's wrapper repeats the
    // call with the host's book, so no message on stderr); the packed bit count and the device's count of zero codes must match what the code book predicted
    int check_final(bool declined, unsigned book_status, u64 bits, u64 unpred) {
        if ((unsigned)h_small[SM_ERR] == 2) { ctx->coef_late = true; FAIL(SZHIP_ERR_INTERNAL, "wavefront kernel: the regression coefficients did not arrive"); }
        if ((unsigned)h_small[SM_ERR] != 0) { ctx->wave_timeout = true; FAIL(SZHIP_ERR_INTERNAL, "wavefront kernel: halo wait timed out"); }
        if (declined) {
            ctx->book_declined = true;
            snprintf(ctx->err, sizeof(ctx->err), "device code book declined (status %u)", book_status);
            return SZHIP_ERR_INTERNAL;
        }
        if ((bits > 0 && h_small[SM_TOTAL_BITS] != bits) || h_small[SM_TOTAL_UNPRED] != unpred)
            FAIL(SZHIP_ERR_INTERNAL, "entropy stage mismatch (bits %llu vs %llu, unpredictable %llu vs %llu)", (unsigned long long)h_small[SM_TOTAL_BITS],
                 (unsigned long long)bits, (unsigned long long)h_small[SM_TOTAL_UNPRED], (unsigned long long)unpred);
        return SZHIP_OK;
    }
    void finish_stats(size_t len, u64 unpred, int packing, int book_on_device) {
        compress_times(ctx, S, host_ms, t_begin, len);
        S.n_unpred = unpred; S.packing = packing; S.book_on_device = book_on_device;
    }
    // ---- the code book on the device (k_huff_book), the header written by kernels, the packing passes: nothing waits for the host before the call's one
    //      synchronisation; the checks come before an output is published
    int encode_with_device_book() {
        const size_t bk_front = meta_len + 8 + 4 + sizeof(T), bk_mid = 1 + sizeof(T);
        if (!P.seghist) HIPCHK(hipStreamWaitEvent(st, ctx->ev_fit, 0));           // (the histogram of the larger alphabets is the second stream's)
        if (!ctx->book_pin) HIPCHK(hipHostMalloc((void **)&ctx->book_pin, 4096, hipHostMallocDefault));
        unsigned char *const blob = (unsigned char *)ctx->book_pin + 256;       // the header's fixed front, then the mean byte and the mean
        unsigned char *const mid = put_front(blob);
        mid[0] = (unsigned char)use_mean; memcpy(mid + 1, &mean, sizeof(T));
        const size_t plan_fixed = bk_front + 12 + bk_mid + ind_bytes + 8;       // the header without the tree
        const size_t tree_cap = 1 + (size_t)9 * (2 * SZH_BOOK_CAP - 1);
        // the buffers are sized before the stream's length is known: room for a stream as large as the array and for a quarter of its values unpredictable (a
        // stream beyond that is declined on the device)
        const size_t unpred_cap = std::min((size_t)n * sizeof(T), (size_t)n * sizeof(T) / 4 + 65536);
        const bool in_place = out_on_device == 2 && *out && *out_size >= plan_fixed + tree_cap + 64 && ((uintptr_t)*out & 15) == 0 && tune_int("SZ_HIP_OUT_IN_PLACE", 1);
        const size_t stream_cap = in_place ? *out_size : plan_fixed + tree_cap + (size_t)n * sizeof(T) + 65536;
        if (!in_place) TRY(ensure(ctx, ctx->stream_buf, stream_cap));
        unsigned char *d_stream = in_place ? (unsigned char *)*out : (unsigned char *)ctx->stream_buf.p;
        TRY(ensure(ctx, ctx->book_stage, bk_front + bk_mid)); TRY(ensure(ctx, ctx->book_tree, tree_cap)); TRY(ensure(ctx, ctx->book_rec, 32 + SZH_PLAN_COUNT * 8));
        TRY(ensure(ctx, ctx->code_tab, (size_t)intervals * 8)); TRY(ensure(ctx, ctx->len_tab, (size_t)intervals));
        TRY(ensure(ctx, ctx->unpred, unpred_cap + 64));
        szh_book_rec *const d_rec = (szh_book_rec *)ctx->book_rec.p;
        u64 *const d_plan = (u64 *)((char *)ctx->book_rec.p + 32);
        HIPCHK(hipMemcpyAsync(ctx->book_stage.p, blob, bk_front + bk_mid, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_huff_book, dim3(1), dim3(256), 0, st, (const unsigned *)d_hist, intervals, SZH_BOOK_TAB_SEG, (unsigned char *)ctx->book_tree.p, (unsigned)tree_cap,
                           (u64 *)ctx->code_tab.p, (uint8_t *)ctx->len_tab.p, d_rec, d_plan, (u64)plan_fixed, (unsigned)sizeof(T), (u64)stream_cap, (u64)unpred_cap);
        HIPCHK(hipGetLastError());
        TRY(upload_segments());
        // the window sized for the longest code words the packing passes take (32 bits)
        TRY(pack_columns(d_stream, 0, (const u64 *)d_plan, 32u, [&]() -> int {
            hipLaunchKernelGGL(k_book_tail, dim3((unsigned)std::min<size_t>(64, (plan_fixed + tree_cap + 255) / 256)), dim3(256), 0, st, d_stream, (const unsigned char *)ctx->book_stage.p, (unsigned)bk_front,
                               (unsigned)bk_mid, intervals, (const unsigned char *)ctx->lor_bits.p, ind_bytes, (const unsigned char *)ctx->book_tree.p, (const szh_book_rec *)d_rec, (const u64 *)d_plan);
            return SZHIP_OK;
        }));
        hipLaunchKernelGGL((k_book_unpred<T>), dim3((unsigned)std::min<size_t>(256, (unpred_cap / sizeof(T) + 255) / 256)), dim3(256), 0, st, d_stream, (const T *)ctx->unpred.p, (const szh_book_rec *)d_rec, (const u64 *)d_plan);
        HIPCHK(hipGetLastError());
        TRY(enqueue_readback());
        HIPCHK(hipMemcpyAsync(ctx->book_pin, ctx->book_rec.p, 32 + SZH_PLAN_COUNT * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));                                      // the call's one wait behind the sweep
        TP("final sync");
        szh_book_rec rec; memcpy(&rec, ctx->book_pin, sizeof(rec));
        const u64 *const plan = (const u64 *)ctx->book_pin + 4;
        print_trace();
        TRY(check_final(book_declines(rec.status, plan[SZH_PLAN_STATUS], tune_int("SZ_HIP_TEST_BOOK_FALLBACK", 0)), rec.status ? rec.status : (unsigned)plan[SZH_PLAN_STATUS],
                        rec.total_bits, rec.total_unpred));
        const size_t len = (size_t)plan[SZH_PLAN_TOTAL_LEN];
        TRY(deliver_stream(ctx, d_stream, len, out_on_device, out, out_size, in_place, true));     // (the final synchronisation is behind us)
        finish_stats(len, rec.total_unpred, 1, 1);
        return SZHIP_OK;
    }
    // ---- Huffman code book (host: heap order decides the codes), built as soon as the histogram has arrived.  This is the only host
    //      round trip of the entropy stage: the number of unpredictable values is the histogram's bin 0, so the header can be written
    //      and the remaining kernels enqueued while the block-ordering pass is still running; the kernel error flag and the device's
    //      own count of zero codes are checked after the final synchronisation.
    //      Here: the book, the coefficient sections joined, the header assembled in pinned memory, the plan revised, the code tables on their way to the device.
    int build_host_book() {
        TP("permute launched");
        HIPCHK(hipEventSynchronize(ctx->ev_fit));
        TP("hist on host");
        double h0 = now_ms();
        const huff_ptr hf = host_book(h_hist, intervals, tab_code, tab_len, &enc_maxlen);
        host_ms += now_ms() - h0;
        total_unpred = h_hist[0];
        if (!hf) FAIL(SZHIP_ERR_INTERNAL, "Huffman build failed");
        TP("tree built");
        join_sections();
        TP("sections joined");
        if (section_failed) FAIL(SZHIP_ERR_INTERNAL, "coefficient Huffman build failed");
        for (int e = 0; e < ncoef; ++e) sections_total += sec_len[e];
        h0 = now_ms();
        const size_t tree_bytes = szhost_huff_tree_size(hf.get());
        pre_len = meta_len + 8 + 4 + sizeof(T) + 4 + 4 + 4 + tree_bytes + 1 + sizeof(T) + ind_bytes;     // the header in front of the coefficient sections
        hdr_len = pre_len + sections_total + 8;
        unpred_bytes = (size_t)total_unpred * sizeof(T);
        total_len = hdr_len + unpred_bytes + (size_t)((hf->total_bits + 7) / 8);
        // assembled in pinned memory (the histogram that lived there has been consumed): with coefficient sections the header is megabytes,
        // and an asynchronous copy from pageable memory of that size makes the runtime pin and unpin the pages
        TRY(ensure_pinned(ctx, pre_len + 8 + 64));
        hdr = (unsigned char *)ctx->pinned;                              // [the header in front of the sections][the eight bytes behind them]
        memset(hdr, 0, pre_len + 8);
        unsigned char *q = put_front(hdr);
        szhost_put_u32be(q, intervals); q += 4;
        szhost_put_u32be(q, (uint32_t)tree_bytes); q += 4;
        szhost_put_u32be(q, (uint32_t)hf->n_nodes); q += 4;
        szhost_huff_tree_write(hf.get(), q); q += tree_bytes;
        *q++ = (unsigned char)use_mean;
        memcpy(q, &mean, sizeof(T)); q += sizeof(T);
        memcpy(q, ind_bits, ind_bytes); q += ind_bytes;
        const uint64_t tu = total_unpred; memcpy(q, &tu, 8);
        total_bits = hf->total_bits;
        // code words of up to 32 bits and a table that fits beside the window in LDS: k_encode32 (32 consecutive codes per thread) packs the
        // payload, from the table `code << 8 | length`; anything else stays with k_encode
        lds_e32 = (size_t)intervals * 8 + ((size_t)SZH_E32_ROUND * enc_maxlen / 32 + 4) * 4 + 16;
        enc32 = enc_maxlen >= 1 && enc_maxlen <= 32 && lds_e32 <= 60 * 1024 && tune_int("SZ_HIP_ENC32", 1);
        if (P.revise(enc_maxlen)) {                                      // (the code book does not fit the packing passes on natural-order codes)
            if (P.sliced) HIPCHK(hipStreamWaitEvent(st, ctx->ev_perm, 0));
            TRY(permute_all());
        }
        if (P.segenc) TRY(upload_segments());
        if (P.segenc) for (unsigned s = 0; s < intervals; ++s) tab_code[s] = (tab_code[s] << 32) | tab_len[s] | (s == 0 ? 0x10000u : 0u);      // (k_col_encode's table: szh_segenc.h)
        else if (enc32) for (unsigned s = 0; s < intervals; ++s) tab_code[s] = (tab_code[s] << 8) | tab_len[s];
        host_ms += now_ms() - h0;
        return upload_code_tables(ctx, tab_code, tab_len);
    }
    // the header in front of the coefficient sections and the eight bytes behind them; the sections themselves from the chain threads' pinned buffers, beside the encoder
    int copy_header(unsigned char *d_stream) {
        HIPCHK(hipMemcpyAsync(d_stream, hdr, pre_len, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_stream + pre_len + sections_total, hdr + pre_len, 8, hipMemcpyHostToDevice, st));
        if (sections_total) {
            const hipStream_t ssec = ctx->stream3 ? ctx->stream3 : ctx->stream2;      // (the third stream has nothing else to do from here on)
            HIPCHK(hipEventRecord(ctx->ev_feed, st));
            HIPCHK(hipStreamWaitEvent(ssec, ctx->ev_feed, 0));
            size_t off = pre_len;
            for (int e = 0; e < ncoef; ++e) { HIPCHK(hipMemcpyAsync(d_stream + off, ctx->sec_pin[e], sec_len[e], hipMemcpyHostToDevice, ssec)); off += sec_len[e]; }
            HIPCHK(hipEventRecord(ctx->ev_sec, ssec));
        }
        return SZHIP_OK;
    }
    // the older packing passes, on block-ordered codes: k_unpred on the second stream beside k_chunk_bits + k_encode32 / k_encode
    int pack_block_ordered(unsigned char *d_stream) {
        const u64 base_bits = (u64)(hdr_len + unpred_bytes) * 8;
        if (P.sliced) HIPCHK(hipStreamWaitEvent(st, ctx->ev_perm, 0));      // block order and per-column offsets (third stream) from here on
        if (total_unpred > 0) {
            // the unpredictable values are gathered on the second stream while the payload is being encoded on the first (both only read
            // the block-ordered codes); their copy into the stream follows the join below
            TRY(ensure(ctx, ctx->unpred, unpred_bytes));
            HIPCHK(hipEventRecord(ctx->ev_in, st));                // block order, per-column offsets ready
            HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_in, 0));
            hipLaunchKernelGGL((k_unpred<T, 0>), dim3(ncols), dim3(256), 0, ctx->stream2, G, (const uint16_t *)d_blk, (const unsigned *)ctx->col_zeros.p,
                               (const u64 *)ctx->col_off.p, d_in, (T *)ctx->unpred.p, (T *)nullptr, (const unsigned *)ctx->zcnt.p, (const unsigned *)ctx->zpos.p, perm_segb, perm_nseg);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ctx->ev_fit, ctx->stream2));
        }
        if (total_bits > 0) {
            TRY(chunk_bit_offsets(ctx, d_blk, n, intervals, sm, 64));
            if (enc32) {
                const int64_t nrounds = (n + SZH_E32_ROUND - 1) / SZH_E32_ROUND;
                hipLaunchKernelGGL(k_encode32, dim3((unsigned)((nrounds + SZH_E32_PER - 1) / SZH_E32_PER)), dim3(256), lds_e32, st, (const uint16_t *)d_blk, n, (const u64 *)ctx->code_tab.p,
                                   intervals, (const u64 *)ctx->chunk_off.p, base_bits, (unsigned *)d_stream);
                HIPCHK(hipGetLastError());
            } else
                TRY(launch_encode(ctx, d_blk, n, intervals, base_bits, d_stream));
        }
        if (total_unpred > 0) HIPCHK(hipStreamWaitEvent(st, ctx->ev_fit, 0));
        return SZHIP_OK;
    }
    // ---- the host's book: header, payload and unpredictable values into the stream buffer; the stream is delivered with the final synchronisation and checked
    //      behind it -- a host copy published by then is released again if a check fails
    int encode_with_host_book() {
        TRY(build_host_book());
        // (a caller's device buffer with room for the stream and the 64 bytes of slack behind it is written in place: no 37 MB copy at the end of the call)
        const bool in_place = out_on_device == 2 && *out && *out_size >= total_len + 64 && ((uintptr_t)*out & 15) == 0 && tune_int("SZ_HIP_OUT_IN_PLACE", 1);
        if (!in_place) TRY(ensure(ctx, ctx->stream_buf, total_len + 64));
        unsigned char *d_stream = in_place ? (unsigned char *)*out : (unsigned char *)ctx->stream_buf.p;
        if (P.segenc) {
            TRY(pack_columns(d_stream, (u64)(hdr_len + unpred_bytes) * 8, (const u64 *)nullptr, enc_maxlen, [&]() -> int {
                TRY(copy_header(d_stream));
                return ensure(ctx, ctx->unpred, unpred_bytes + 64);
            }));
        } else {
            HIPCHK(hipMemsetAsync(d_stream, 0, total_len + 64, st));
            TRY(copy_header(d_stream));
            TRY(pack_block_ordered(d_stream));
        }
        if (total_unpred > 0) HIPCHK(hipMemcpyAsync(d_stream + hdr_len, ctx->unpred.p, unpred_bytes, hipMemcpyDeviceToDevice, st));
        if (sections_total) HIPCHK(hipStreamWaitEvent(st, ctx->ev_sec, 0));
        TRY(enqueue_readback());
        TRY(deliver_stream(ctx, d_stream, total_len, out_on_device, out, out_size, in_place, false));
        TP("final sync");
        print_trace();
        const int rc = check_final(false, 0, total_bits, total_unpred);
        if (rc != SZHIP_OK) {                                    // found AFTER the stream was handed to the caller's pointer: a host copy that this call malloc'd is released again
            if (!out_on_device && *out) { free(*out); *out = nullptr; }
            *out_size = 0;
            return rc;
        }
        finish_stats(total_len, total_unpred, P.segenc ? 1 : 0, 0);
        return SZHIP_OK;
    }
};

template <class T>
int compress_impl(szhip_ctx *ctx, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, double eb_in, const szhip_params *prm, const unsigned char *meta, size_t meta_len, int out_on_device,
                  unsigned char **out, size_t *out_size, szhip_stats *stats)
{
    sz21_call<T> c(ctx, r0, r1, r2, eb_in, prm, meta, meta_len, out_on_device, out, out_size);
    int rc = c.stage_and_fit(data, data_on_device);
    if (rc == SZHIP_OK) rc = c.choose_intervals();
    if (rc == SZHIP_OK) rc = c.join_fit();
    if (rc == SZHIP_CONSTANT && stats) *stats = c.S;
    if (rc != SZHIP_OK) return rc;
    if (ctx->chain_pool) ctx->chain_pool->arm();       // (the workers wake up now and spin until the coefficients are there -- or are sent back to sleep when the call ends)
    if (c.reg_count > 0) { TRY(c.prepare_chains()); TRY(c.run_chains()); }
    HIPCHK(hipEventRecord(ctx->ev[1], c.st));
    c.TP("ev1");
    c.P = sz21_make_plan<T>(ctx, c.G, c.intervals, c.reg_count, beam_applies<T>(c.G, c.d_in, c.reg_count), c.overlap, c.feed, meta_len);
    TRY(c.launch_sweep());
    TRY(c.hist_and_order());
    TRY(c.P.dev_book ? c.encode_with_device_book() : c.encode_with_host_book());
    return c.done(stats);
}

// Huffman decode of `n` symbols on the device (self-synchronising sub-sequence decode, k_hdec_*): `d_bits` points at the payload,
// `dtab` is the host-built decode table of the tree, `single_symbol` >= 0 for the one-leaf tree (zero payload bits).
// after the synchronisation that follows huff_decode_device: did its two unsynchronised rounds settle every start?
#define HDEC_CHECK(ctx) do { if ((ctx)->hdec_res[1] != 0 || (tune_int("SZ_HIP_TEST_HDEC_FALLBACK", 0) && !(ctx)->hdec_sync_rounds)) { (ctx)->hdec_unconverged = true; \
        /* (no message on stderr: the caller's wrapper repeats the call with a synchronisation per round) */ \
        snprintf((ctx)->err, sizeof((ctx)->err), "Huffman decode: %llu start guesses still moving after two rounds", (ctx)->hdec_res[1]); return SZHIP_ERR_INTERNAL; } } while (0)
int huff_decode_device(szhip_ctx *ctx, u64 *sm, const unsigned char *d_bits, unsigned bytes_before, u64 total_bits, const std::vector<uint32_t> &dtab, int n_nodes,
                       int single_symbol, int64_t n, uint16_t *d_out_codes)
{
    // ctx->hdec_res[0] receives the number of symbols the payload holds ASYNCHRONOUSLY: the caller compares it with n after its next
    // synchronisation of the stream (check_decoded; the write pass below never stores beyond n, so a short payload is harmless until then)
    if (!ctx->hdec_res) HIPCHK(hipHostMalloc((void **)&ctx->hdec_res, 64, hipHostMallocDefault));
    ctx->hdec_res[0] = (u64)n; ctx->hdec_res[1] = 0;
    hipStream_t st = ctx->stream;
    if (single_symbol >= 0) {
        hipLaunchKernelGGL(k_fill_u16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_out_codes, n, (uint16_t)single_symbol);
        HIPCHK(hipGetLastError());
    } else {
        const int64_t nsub = (int64_t)((total_bits + SZH_SUBSEQ_BITS - 1) / SZH_SUBSEQ_BITS);
        if (nsub == 0) FAIL(SZHIP_ERR_STREAM, "empty Huffman payload");
        const size_t lut_off = (dtab.size() * 4 + 63) / 64 * 64;
        TRY(ensure(ctx, ctx->dec_tab, lut_off + SZH_LUT_BYTES));
        HIPCHK(hipMemcpyAsync(ctx->dec_tab.p, dtab.data(), dtab.size() * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_hdec_build_lut, dim3(SZH_LUT_SIZE / 256), dim3(256), 0, st, (const unsigned *)ctx->dec_tab.p, (uint4 *)((char *)ctx->dec_tab.p + lut_off));
        TRY(ensure(ctx, ctx->starts, (size_t)nsub * 8)); TRY(ensure(ctx, ctx->ends, (size_t)nsub * 8));
        TRY(ensure(ctx, ctx->counts, (size_t)nsub * 8)); TRY(ensure(ctx, ctx->offs, (size_t)nsub * 8));
        TRY(ensure(ctx, ctx->dirty, (size_t)nsub));
        szh_hdec_args a;
        a.bits = d_bits; a.total_bits = total_bits; a.bytes_before = bytes_before; a.table = (const unsigned *)ctx->dec_tab.p; a.n_nodes = n_nodes;
        a.table_in_lds = (size_t)n_nodes * 8 <= 13 * 1024; a.nsub = nsub;      // (the write pass: 33 KB of bits + 16 KB of table + this <= 64 KB)
        a.lut = (const uint4 *)((char *)ctx->dec_tab.p + lut_off);
        a.starts = (u64 *)ctx->starts.p; a.ends = (u64 *)ctx->ends.p; a.counts = (u64 *)ctx->counts.p;
        a.dirty = (unsigned char *)ctx->dirty.p; a.changed = (unsigned *)(sm + SM_CHANGED);
        const size_t lds_tab = a.table_in_lds ? (size_t)n_nodes * 8 : 16;
        const size_t lds_pass = SZH_HDEC_LDS + SZH_LUT_SIZE * 4 + lds_tab, lds_write = SZH_HDEC_LDS + SZH_LUT_SIZE * 16 + lds_tab;
        const unsigned gsub = (unsigned)((nsub + 255) / 256);
        hipLaunchKernelGGL(k_hdec_init, dim3(gsub), dim3(256), 0, st, a);
        const bool optimistic = !ctx->hdec_sync_rounds;
        // rounds without a host round trip: round 0 (warm-up guesses), then repair rounds that only touch the sub-sequences whose start
        // moved (a workgroup without one returns at once: ~10 us per idle round).  Smooth fields settle in round 1; wide code books
        // (codes longer than the look-up window resynchronise slowly) sometimes need a third
        constexpr int64_t opt_rounds = 3;
        int64_t iter = 0;
        for (;;) {
            a.warmup = iter == 0;                                  // the first round finds its own starts (k_hdec_pass)
            hipLaunchKernelGGL(k_hdec_pass, dim3(gsub), dim3(256), lds_pass, st, a);
            HIPCHK(hipMemsetAsync(sm + SM_CHANGED, 0, 8, st));
            hipLaunchKernelGGL(k_hdec_update, dim3(gsub), dim3(256), 0, st, a);
            HIPCHK(hipGetLastError());
            if (optimistic) {
                // round 0 repairs nearly every guess (84 of 287 393 wrong at 512^3), round 1 the rest; whether anything still moved after
                // the last round is read with the caller's next synchronisation (two host round trips of ~35 us less per call)
                if (iter + 1 < opt_rounds && nsub > 1) { ++iter; continue; }
                HIPCHK(hipMemcpyAsync(&ctx->hdec_res[1], sm + SM_CHANGED, 8, hipMemcpyDeviceToHost, st));
                break;
            }
            unsigned changed = 0;
            HIPCHK(hipMemcpyAsync(&changed, sm + SM_CHANGED, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (!changed) break;
            if (++iter > nsub + 2) FAIL(SZHIP_ERR_INTERNAL, "Huffman decode did not converge");
        }
        TRY(scan_u64(ctx, (const u64 *)ctx->counts.p, nsub, (u64 *)ctx->offs.p, sm + SM_TOTAL_SYM));
        HIPCHK(hipMemcpyAsync(&ctx->hdec_res[0], sm + SM_TOTAL_SYM, 8, hipMemcpyDeviceToHost, st));   // (pinned: a copy into pageable memory blocks the host)
        hipLaunchKernelGGL(k_hdec_write, dim3(gsub), dim3(256), lds_write, st, a, (const u64 *)ctx->offs.p, d_out_codes, n);
        HIPCHK(hipGetLastError());
    }

    return SZHIP_OK;
}

// behind that synchronisation: every start guess settled, the payload holds n symbols, the codes' zeros are as many as the `listed` values of the stream (`what` they are)
int check_decoded(szhip_ctx *ctx, int64_t n, u64 listed, u64 zeros_found, const char *what)
{
    HDEC_CHECK(ctx);
    if ((int64_t)ctx->hdec_res[0] < n) FAIL(SZHIP_ERR_STREAM, "Huffman payload holds %llu symbols, need %lld", ctx->hdec_res[0], (long long)n);
    if (zeros_found != listed) FAIL(SZHIP_ERR_STREAM, "stream lists %llu %s values, codes need %llu", (unsigned long long)listed, what, (unsigned long long)zeros_found);
    return SZHIP_OK;
}

// everything the host reads from an SZ 2.1 regression-type stream before the unpredictable values
template <class T> struct dec_header {
    T eb = 0, mean = 0;
    unsigned intervals = 0; int use_mean = 0;
    dec_table D;                                       // of the type array's tree
    size_t reg_count = 0, ind_off = 0, unpred_off = 0, pay_off = 0; uint64_t total_unpred = 0;
    std::vector<T> coef;                               // decoded regression coefficients, compact [4][reg_count]
    bool defer = false;                                // in: the caller runs the coefficient sections' decode itself (finish), beside other work
    std::function<int()> finish; char finish_err[200] = {0};
};

// returns 0 = parsed, 1 = needs at least *need bytes of the stream on the host, < 0 = malformed (message in err)
template <class T>
int parse_header(const unsigned char *hs, size_t avail, size_t stream_len, size_t body_off, size_t nb, int want_block_size,
                 dec_header<T> &H, size_t *need, char *err, size_t errlen)
{
    const int ncoef = want_block_size == SZH_BLOCK_SIZE_2D ? 3 : 4;
    const int is_double = sizeof(T) == 8;
#define PFAIL(code, ...) do { snprintf(err, errlen, __VA_ARGS__); return (code); } while (0)
#define NEED(k) do { const size_t end_ = (size_t)(q - hs) + (size_t)(k); if (end_ > stream_len) PFAIL(SZHIP_ERR_STREAM, "truncated stream"); \
                     if (end_ > avail) { *need = std::min(stream_len, end_ + need_more); return 1; } } while (0)
    size_t need_more = 0;                      // what a longer prefix should hold beyond the bytes asked for (the coefficient sections still to come)
    const unsigned char *q = hs + body_off;
    const int tp_on = tune_int("SZ_HIP_TIMING", 0); const double tp0 = now_ms();
    auto mark = [&](const char *nm) { if (tp_on) fprintf(stderr, "[header %s %.3f] ", nm, now_ms() - tp0); };
    NEED(4 + sizeof(T) + 12);
    const unsigned block_size = szhost_get_u32be(q); q += 4;
    if ((int)block_size != want_block_size) PFAIL(SZHIP_ERR_UNSUP, "block size %u", block_size);
    H.eb = is_double ? (T)szhost_get_f64be(q) : (T)szhost_get_f32be(q); q += sizeof(T);
    H.intervals = szhost_get_u32be(q); q += 4;
    const unsigned tree_size = szhost_get_u32be(q); q += 4;
    const int node_count = (int)szhost_get_u32be(q); q += 4;
    if (H.intervals < 4 || H.intervals > 65536) PFAIL(SZHIP_ERR_STREAM, "bad interval count %u", H.intervals);
    NEED(tree_size);
    if (node_count <= 0 || szhost_huff_serial_size(node_count) > tree_size) PFAIL(SZHIP_ERR_STREAM, "bad Huffman tree size");
    if (!read_tree(q, node_count, H.intervals, H.D)) PFAIL(SZHIP_ERR_STREAM, "bad Huffman tree");
    q += tree_size;
    NEED(1 + sizeof(T));
    H.use_mean = *q++;
    memcpy(&H.mean, q, sizeof(T)); q += sizeof(T);
    const size_t ind_bytes = (nb - 1) / 8 + 1;
    NEED(ind_bytes);
    {   // regression blocks = zero bits among the first nb
        size_t ones = 0, full = nb / 8;
        for (size_t i = 0; i < full; ++i) ones += (size_t)__builtin_popcount(q[i]);
        for (size_t b = full * 8; b < nb; ++b) ones += (q[b >> 3] >> (7 - (b & 7))) & 1;
        H.reg_count = nb - ones;
    }
    H.ind_off = (size_t)(q - hs);
    q += ind_bytes;
    H.coef.clear();
    if (H.reg_count > 0) {
        // The four sections are LOCATED first (their lengths stand in front of them) and decoded afterwards, each on its own thread for a large
        // array: located first, a prefix of the stream that turns out too short costs no decoding (round 4 decoded the sections again for every
        // longer prefix it fetched: 3 x at the M-field's 3.4 MB header), and the bit-serial Huffman decode of ~300 000 codes is the long part.
        int crad[4]; double cprec[4]; const unsigned char *cun[4];
        const unsigned char *tree_at[4], *pay_at[4]; int cnc_of[4]; size_t enc_of[4]; unsigned cu_of[4];
        for (int e = 0; e < ncoef; ++e) {
            NEED(sizeof(T) + 12);
            cprec[e] = is_double ? szhost_get_f64be(q) : (double)szhost_get_f32be(q); q += sizeof(T);
            crad[e] = (int)szhost_get_u32be(q); q += 4;
            const unsigned ts = szhost_get_u32be(q); q += 4;
            const int cnc = (int)szhost_get_u32be(q); q += 4;
            NEED(ts);
            if (cnc <= 0 || crad[e] <= 0 || crad[e] > 32768 || szhost_huff_serial_size(cnc) > ts) PFAIL(SZHIP_ERR_STREAM, "bad coefficient tree size");
            tree_at[e] = q; cnc_of[e] = cnc;
            q += ts;
            NEED(8);
            const uint64_t enc64 = szhost_get_u64be(q); q += 8;
            if (enc64 > (uint64_t)(stream_len - (size_t)(q - hs))) PFAIL(SZHIP_ERR_STREAM, "truncated stream");   // before any size arithmetic on it
            enc_of[e] = (size_t)enc64;
            need_more = (size_t)(ncoef - 1 - e) * (enc_of[e] + enc_of[e] / 2 + ts + 65536) + 65536;   // (the sections are of similar size: one more fetch, not three)
            NEED(enc_of[e]);
            need_more = 0;
            pay_at[e] = q;
            q += enc_of[e];
            NEED(4);
            cu_of[e] = szhost_get_u32be(q); q += 4;
            NEED((size_t)cu_of[e] * sizeof(T));
            cun[e] = q; q += (size_t)cu_of[e] * sizeof(T);
        }
        NEED(8);                                   // (the word after the sections: nothing below asks for more of the stream)
        mark("located");
        // The sections' decode (Huffman payload -> codes -> chain) is the long part of the host's work (~1 ms for the 512^3 M-field's 303 450 blocks on four
        // threads).  A caller that sets H.defer gets it back as H.finish and runs it BESIDE the device's decode of the type array (decompress_impl): it reads
        // only the stream bytes located above (which stay where they are until it has run) and writes H.coef.
        H.coef.assign(H.reg_count * 4, (T)0);
        struct sec_desc { const unsigned char *tree_at, *pay_at, *cun; int cnc, crad; size_t enc; unsigned cu; double prec; };
        std::array<sec_desc, 4> sd{};
        for (int e = 0; e < ncoef; ++e) sd[e] = sec_desc{tree_at[e], pay_at[e], cun[e], cnc_of[e], crad[e], enc_of[e], cu_of[e], cprec[e]};
        T *const coef_out = H.coef.data(); const size_t reg_count = H.reg_count; char *const ferr = H.finish_err;
        auto run_sections = [sd, ncoef, is_double, coef_out, reg_count, ferr]() -> int {
            int sec_rc[4] = {0, 0, 0, 0};              // 1 bad tree, 2 payload too short, 3 too few verbatim values
            size_t sec_zeros[4] = {0, 0, 0, 0};
            const std::vector<unsigned char> all_reg(reg_count, 0);
            auto decode_section = [&](int e) {
                const huff_ptr ch(szhost_huff_from_bytes(4 * sd[e].crad, sd[e].tree_at, sd[e].cnc));
                if (!ch) { sec_rc[e] = 1; return; }
                std::vector<int> codes(reg_count);
                if (!szhost_huff_decode_i32(ch.get(), sd[e].pay_at, sd[e].enc, reg_count, codes.data())) { sec_rc[e] = 2; return; }   // (bounded by the section's own length)
                // every zero code takes one verbatim coefficient (szd_float.c:5809-5820): the list must hold them all
                size_t zeros = 0;
                for (size_t i = 0; i < reg_count; ++i) zeros += codes[i] == 0;
                sec_zeros[e] = zeros;
                if (zeros > sd[e].cu) { sec_rc[e] = 3; return; }
                // the chain of this coefficient (szd_float.c:5809-5820), on the same thread: compact [4][reg_count] in scan order, which the device scatters
                // to the blocks (k_move_coef); 2-D planes {a, b, c} are carried as {0, a, b, c}
                int *const c1[4] = {codes.data(), nullptr, nullptr, nullptr};
                const int r1[4] = {sd[e].crad, 0, 0, 0}; const double p1[4] = {sd[e].prec, 0, 0, 0}; const unsigned char *const u1[4] = {sd[e].cun, nullptr, nullptr, nullptr};
                szhost_coeff_unchain(is_double, coef_out + (size_t)(e + (ncoef == 3 ? 1 : 0)) * reg_count, all_reg.data(), reg_count, c1, r1, p1, u1, 1);
            };
            if (reg_count >= 16384) {
                std::vector<std::thread> th;
                for (int e = 1; e < ncoef; ++e) th.emplace_back(decode_section, e);
                decode_section(0);
                for (auto &t : th) t.join();
            } else {
                for (int e = 0; e < ncoef; ++e) decode_section(e);
            }
            for (int e = 0; e < ncoef; ++e) {
                if (sec_rc[e] == 1) { snprintf(ferr, 200, "bad coefficient tree"); return SZHIP_ERR_STREAM; }
                if (sec_rc[e] == 2) { snprintf(ferr, 200, "coefficient payload too short"); return SZHIP_ERR_STREAM; }
                if (sec_rc[e] == 3) { snprintf(ferr, 200, "coefficient section lists %u verbatim values, codes need %zu", sd[e].cu, sec_zeros[e]); return SZHIP_ERR_STREAM; }
            }
            return 0;
        };
        if (H.defer && H.reg_count >= (size_t)tune_int("SZ_HIP_DEC_DEFER_MIN", 16384)) H.finish = run_sections;
        else { const int src = run_sections(); if (src) PFAIL(src, "%s", H.finish_err); }
        mark("unchained");
    }
    NEED(8);
    memcpy(&H.total_unpred, q, 8); q += 8;
    H.unpred_off = (size_t)(q - hs);
    if (H.total_unpred > (stream_len - H.unpred_off) / sizeof(T)) PFAIL(SZHIP_ERR_STREAM, "truncated stream");
    H.pay_off = H.unpred_off + (size_t)H.total_unpred * sizeof(T);
    mark("done");
    return 0;
#undef NEED
#undef PFAIL
}

template <class T>
int decompress_impl(szhip_ctx *ctx, const unsigned char *stream_in, int stream_on_device, size_t stream_len, size_t body_off,
                    size_t r0, size_t r1, size_t r2, void *out, int out_on_device, szhip_stats *stats)
{
    const szh_geom3 G = r0 == 0 ? szh_make_geom2((int)r1, (int)r2) : szh_make_geom3((int)r0, (int)r1, (int)r2);
    const int64_t n = G.n, nb = G.nblocks;
    const double t_begin = now_ms();
    double host_ms = 0;
    hipStream_t st = ctx->stream;
    szhip_stats S; memset(&S, 0, sizeof(S));
    S.n_elements = (uint64_t)n; S.n_blocks = (uint64_t)nb;

    // ---- stream on both sides: the device gets the whole stream; the host only needs the header (everything up to the
    //      unpredictable values), fetched from a device-resident stream in growing prefixes
    std::vector<unsigned char> hcopy;
    const unsigned char *hs = stream_in;
    size_t avail = stream_len;
    TRY(ensure(ctx, ctx->stream_buf, stream_len + 64));
    unsigned char *d_stream = (unsigned char *)ctx->stream_buf.p;
    // (a device-resident stream: the header's bytes go to the host FIRST, straight from the caller's array, and the copy of the whole stream into the context's buffer -- the bit
    //  reader may look a few bytes past the end: 64 zero bytes behind it -- runs behind them while the host reads the header: ~30 us of a 512^3 call off its serial head)
    HIPCHK(hipEventRecord(ctx->ev[0], st));
    bool on_device_copied = false;
    auto copy_on_device = [&]() -> int {
        if (on_device_copied) return SZHIP_OK;
        on_device_copied = true;
        if (stream_in != d_stream) HIPCHK(hipMemcpyAsync(d_stream, stream_in, stream_len, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemsetAsync(d_stream + stream_len, 0, 64, st));
        return SZHIP_OK;
    };
    if (stream_on_device) avail = 0;
    else {
        TRY(staged_copy(ctx, d_stream, stream_in, stream_len, true));
        HIPCHK(hipMemsetAsync(d_stream + stream_len, 0, 64, st));
    }

    // ---- header (szd_float.c:3491-3587)
    double h0 = now_ms();
    dec_header<T> H;
    H.defer = true;
    struct Finisher {     // the deferred part of the header (the coefficient sections) on its own thread; no return path may leave it running on H
        std::thread th; int rc = 0;
        void join() { if (th.joinable()) th.join(); }
        ~Finisher() { join(); }
    } finisher;
    for (size_t want = std::min<size_t>(stream_len, (size_t)256 << 10);;) {
        if (stream_on_device && want > avail) {
            TRY(ensure_pinned(ctx, want));
            HIPCHK(hipMemcpyAsync(ctx->pinned, stream_in, want, hipMemcpyDeviceToHost, st));
            HIPCHK(hipEventRecord(ctx->ev_in, st));
            TRY(copy_on_device());
            HIPCHK(hipEventSynchronize(ctx->ev_in));
            hs = (const unsigned char *)ctx->pinned; avail = want;
        }
        size_t need = 0;
        const int rc = parse_header<T>(hs, avail, stream_len, body_off, (size_t)nb, G.block_size, H, &need, ctx->err, sizeof(ctx->err));
        if (rc == 0) break;
        if (rc < 0) {
            if (on_device_copied) hipStreamSynchronize(st);      // (the copy reads the caller's array: not beyond this call's return)
            fprintf(stderr, "szhip: %s\n", ctx->err); return rc;
        }
        want = std::min<size_t>(stream_len, std::max<size_t>(need, avail * 2)); // rc == 1: more bytes needed
    }
    if (stream_on_device) TRY(copy_on_device());
    if (H.finish) finisher.th = std::thread([&] { finisher.rc = H.finish(); });      // (beside the device's decode of the type array, joined where the coefficients are shipped)
    if (tune_int("SZ_HIP_TIMING", 0)) fprintf(stderr, "[header on host %.3f ms after the call began]\n", now_ms() - t_begin);
    const T eb = H.eb, mean = H.mean;
    const unsigned intervals = H.intervals;
    const int use_mean = H.use_mean, n_nodes = H.D.n_nodes, single_symbol = H.D.single_symbol;
    const size_t reg_count = H.reg_count, unpred_off = H.unpred_off, pay_off = H.pay_off;
    const uint64_t total_unpred = H.total_unpred;
    std::vector<T> &hcoef = H.coef;
    std::vector<uint32_t> &dtab = H.D.dtab;
    const u64 total_bits = (u64)(stream_len - pay_off) * 8;
    S.intervals = intervals; S.use_mean = use_mean; S.n_reg_blocks = reg_count; S.n_unpred = total_unpred;
    host_ms += now_ms() - h0;

    u64 *sm = nullptr;
    TRY(clear_small(ctx, &sm));
    // The inverse sweep: k_beam wherever it applies (szh_beam.h), k_pencil on natural-order codes for the rest (2-D, SZ 1.4, rows that are no multiple of four values).
    // (Rounds 3 - 5 ran Lorenzo-only 3-D arrays through the hyperplane "ribbon" mapping in its own code / value order, k_unribbon behind it: removed in round 6.)
    const size_t nat_elems = (size_t)n;
    const bool dec_beam = beam_applies<T>(G, out_on_device ? (const void *)out : (const void *)nullptr, reg_count);   // (the context's own buffer is aligned)
    TRY(ensure(ctx, ctx->codes_nat, nat_elems * 2 + 64));
    TRY(ensure(ctx, ctx->codes_blk, (size_t)n * 2 + 64));
    uint16_t *d_nat = (uint16_t *)ctx->codes_nat.p, *d_blk = (uint16_t *)ctx->codes_blk.p;

    // ---- Huffman decode of the type array
    TRY(huff_decode_device(ctx, sm, d_stream + pay_off, (unsigned)std::min<size_t>(pay_off, 4096), total_bits, dtab, n_nodes, single_symbol, n, d_blk));

    // ---- natural order, unpredictable values into the output array
    const int ncols = G.g0.num * G.g1.num;
    TRY(ensure(ctx, ctx->col_zeros, (size_t)ncols * 4));
    TRY(ensure(ctx, ctx->col_zeros64, (size_t)ncols * 8));
    TRY(ensure(ctx, ctx->col_off, (size_t)ncols * 8));
    int perm_segb = 1, perm_nseg = 1;
    T *d_out = nullptr;
    TRY(device_out(ctx, out, out_on_device, (size_t)n, &d_out));
    T *d_sweep = d_out;                        // what the inverse sweep works on: the output array, or (mode 2) a ribbon-order value array
    // (the inverse sweep fed slice by slice while it runs, tried in round 5, measured slower -- 2.34 against 2.12 - 2.21 ms, profiles/r05_tried_fed_inverse_sweep.txt -- and
    //  removed in round 6)
    // (round 6) where the inverse beam runs (codes and values in natural order): the zero codes per block column are counted first (k_col_zeros), and behind the checks below
    // ONE pass turns the block-ordered codes into natural order and drops the unpredictable values into the array (k_col_unpack, szh_segenc.h) -- k_permute<1> + k_unpred<1> before
    const int up_vw = (G.g2.count % 8) == 0 ? 8 : ((G.g2.count % 4) == 0 ? 4 : 1);
    int up_segb = 0, up_nseg = 0; size_t up_lds = 0;
    bool col_unpack = dec_beam && tune_int("SZ_HIP_COL_UNPACK", 1) != 0 && ((uintptr_t)d_blk & 15) == 0 && (double)n < 4.0e9;
    if (col_unpack) {
        const size_t rows_max = (size_t)G.g0.early * G.g1.early, want = (size_t)std::max(4, tune_int("SZ_HIP_UNPACK_TILE_KB", 24)) * 1024;
        int sb = 1;
        while (sb < G.g2.num && (rows_max * (size_t)(sb + 1) * G.g2.early + 16) * 2 <= want) ++sb;
        up_segb = sb; up_nseg = (G.g2.num + sb - 1) / sb;
        up_lds = ((rows_max * (size_t)sb * G.g2.early + 16) * 2 + 15) & ~(size_t)15;
        if (up_lds > 63 * 1024 || rows_max > 128) col_unpack = false;
    }
    std::vector<szh_se::seg_t> up_segs;                              // (on its way to the device until the synchronisation below)
    if (col_unpack) {
        hipLaunchKernelGGL(k_col_zeros, dim3((unsigned)ncols), dim3(256), 0, st, G, (const uint16_t *)d_blk, (unsigned *)ctx->col_zeros.p);
        HIPCHK(hipGetLastError());
        up_segs.resize((size_t)up_nseg);
        for (int q = 0; q < up_nseg; ++q) up_segs[(size_t)q] = szh_se::make_seg(G, 1, q, up_segb, up_vw);
        TRY(ensure(ctx, ctx->seg_tab, up_segs.size() * sizeof(szh_se::seg_t)));
        HIPCHK(hipMemcpyAsync(ctx->seg_tab.p, up_segs.data(), up_segs.size() * sizeof(szh_se::seg_t), hipMemcpyHostToDevice, st));
    } else
    {
        HIPCHK(hipMemsetAsync(ctx->col_zeros.p, 0, (size_t)ncols * 4, st));     // (k_permute<1> adds its segments' counts; k_col_zeros stores a column's)
        const int segb = choose_segb(G, 2, SZH_PERM_TILE_BYTES);
        const int nseg = (G.g2.num + segb - 1) / segb;
        TRY(ensure(ctx, ctx->zcnt, (size_t)ncols * nseg * 4));
        TRY(ensure(ctx, ctx->zpos, (size_t)ncols * nseg * SZH_ZCAP * 4));
        hipLaunchKernelGGL((k_permute<1>), dim3(ncols, std::min(nseg, std::max(1, tune_int("SZ_HIP_PERM_Y", nseg)))), dim3(256), tile_bytes(G, segb, 2), st, G, (const uint16_t *)d_blk, d_nat,
                           (unsigned *)ctx->col_zeros.p, segb, (unsigned *)ctx->zcnt.p, (unsigned *)ctx->zpos.p, 0);
        perm_segb = segb; perm_nseg = nseg;
        HIPCHK(hipGetLastError());
    }
    if (col_unpack && ncols <= 1024 * SZH_COL_SCAN_PER && tune_int("SZ_HIP_SEG_SCAN1", 1)) {
        hipLaunchKernelGGL(k_col_zscan, dim3(1), dim3(1024), 0, st, (const unsigned *)ctx->col_zeros.p, (int)ncols, (u64 *)ctx->col_off.p, sm + SM_TOTAL_UNPRED);
        HIPCHK(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_u32_to_u64, dim3((ncols + 255) / 256), dim3(256), 0, st, (const unsigned *)ctx->col_zeros.p, (int64_t)ncols,
                           (u64 *)ctx->col_zeros64.p);
        TRY(scan_u64(ctx, (const u64 *)ctx->col_zeros64.p, ncols, (u64 *)ctx->col_off.p, sm + SM_TOTAL_UNPRED));
    }
    // The checks of what the decoder found -- every start guess settled, the payload holds n symbols, the codes' zeros are as many as the stream's list of unpredictable
    // values -- need the host: a synchronisation.  Where k_col_unpack follows (it never reads beyond the list: `ucap`; any 16-bit code is a code to the sweep) nothing on the
    // device waits for them: they are made behind the call's LAST synchronisation, and the host's round trip (copy, wake-up, the next launches: 30 - 40 us) is off the
    // device's time line.  The older passes (k_unpred<1> trusts the counts) keep the synchronisation here.
    ctx->hdec_res[2] = 0;
    HIPCHK(hipMemcpyAsync(&ctx->hdec_res[2], sm + SM_TOTAL_UNPRED, 8, hipMemcpyDeviceToHost, st));      // (pinned, as the decoder's own two words)
    auto decoder_checks = [&]() { return check_decoded(ctx, n, total_unpred, ctx->hdec_res[2], "unpredictable"); };
    const bool checks_last = col_unpack && tune_int("SZ_HIP_DEC_CHECKS_LAST", 1) != 0;
    if (!checks_last) {
        HIPCHK(hipStreamSynchronize(st));
        TRY(decoder_checks());
    }
    if (col_unpack) {
        TRY(ensure(ctx, ctx->unpred, (size_t)total_unpred * sizeof(T) + 64));
        if (total_unpred > 0) HIPCHK(hipMemcpyAsync(ctx->unpred.p, d_stream + unpred_off, (size_t)total_unpred * sizeof(T), hipMemcpyDeviceToDevice, st));      // (the list lies at any byte offset in the stream)
        hipLaunchKernelGGL((k_col_unpack<T>), dim3((unsigned)ncols), dim3(256), up_lds, st, G, (const uint16_t *)d_blk, d_nat, (const szh_se::seg_t *)ctx->seg_tab.p, up_nseg, up_vw,
                           (const u64 *)ctx->col_off.p, (const T *)ctx->unpred.p, (u64)total_unpred, d_sweep);
        HIPCHK(hipGetLastError());
    } else
    if (total_unpred > 0) {
        TRY(ensure(ctx, ctx->unpred, (size_t)total_unpred * sizeof(T)));
        HIPCHK(hipMemcpyAsync(ctx->unpred.p, d_stream + unpred_off, (size_t)total_unpred * sizeof(T), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL((k_unpred<T, 1>), dim3(ncols), dim3(256), 0, st, G, (const uint16_t *)d_blk, (const unsigned *)ctx->col_zeros.p,
                           (const u64 *)ctx->col_off.p, (const T *)nullptr, (T *)ctx->unpred.p, d_sweep, (const unsigned *)ctx->zcnt.p,
                           (const unsigned *)ctx->zpos.p, perm_segb, perm_nseg);
        HIPCHK(hipGetLastError());
    }
    TRY(ensure(ctx, ctx->coef, (size_t)nb * 4 * sizeof(T)));
    TRY(ensure(ctx, ctx->blk_lor, (size_t)nb));

    hipLaunchKernelGGL(k_unpack_lor, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (const uint8_t *)(d_stream + H.ind_off), nb,
                       (uint8_t *)ctx->blk_lor.p);
    HIPCHK(hipGetLastError());
    if (reg_count > 0) {
        TRY(ensure(ctx, ctx->reg_flags, (size_t)nb * 8));
        TRY(ensure(ctx, ctx->reg_rank, (size_t)nb * 8));
        TRY(ensure(ctx, ctx->coef_compact, reg_count * 4 * sizeof(T)));
        {   // the coefficient sections, if their decode was deferred
            const double hj = now_ms();
            finisher.join();
            host_ms += now_ms() - hj;
            if (tune_int("SZ_HIP_TIMING", 0)) fprintf(stderr, "[sections joined %.3f ms after the call began, waited %.3f]\n", now_ms() - t_begin, now_ms() - hj);
            if (finisher.rc) { snprintf(ctx->err, sizeof(ctx->err), "%s", H.finish_err); fprintf(stderr, "szhip: %s\n", ctx->err); return finisher.rc; }
        }
        TRY(ensure_pinned3(ctx, hcoef.size() * sizeof(T)));    // (asynchronous copies from pageable memory stall later calls, see compress_impl)
        memcpy(ctx->pinned3, hcoef.data(), hcoef.size() * sizeof(T));
        HIPCHK(hipMemcpyAsync(ctx->coef_compact.p, ctx->pinned3, hcoef.size() * sizeof(T), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_reg_flags, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (const uint8_t *)ctx->blk_lor.p, nb, (u64 *)ctx->reg_flags.p);
        TRY(scan_u64(ctx, (const u64 *)ctx->reg_flags.p, nb, (u64 *)ctx->reg_rank.p, sm + SM_SCRATCH));
        hipLaunchKernelGGL((k_move_coef<T, 1>), dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (const uint8_t *)ctx->blk_lor.p,
                           (const u64 *)ctx->reg_rank.p, nb, (int64_t)reg_count, (T *)ctx->coef.p, (T *)ctx->coef_compact.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ctx->ev[1], st));

    // ---- reconstruct: the wavefront kernel
    int nI, nJ, ntiles;
    using TS = szh_tile_shape<T>;
    TRY(prepare_pencil(ctx, G, szh_gran<T>::NW, TS::TPI, TS::TPJ, &nI, &nJ, &ntiles));
    {
        szh_qargs<T> a; memset(&a, 0, sizeof(a));
        a.G = G; a.data = nullptr; a.out = d_out; a.codes = d_nat; a.blk_lor = (const uint8_t *)ctx->blk_lor.p; a.coef = (const T *)ctx->coef.p; a.coef_stride = nb;
        a.eb = eb; a.recip = 1 / eb; a.mean = mean; a.cap = (int)intervals; a.radius = (int)intervals / 2; a.use_mean = use_mean;
        a.faceI = (szh_u64 *)ctx->faceI.p; a.faceJ = (szh_u64 *)ctx->faceJ.p; a.epoch = ++ctx->epoch;
        a.nI = nI; a.nJ = nJ; a.order = (const unsigned *)ctx->order.p; a.no_reg = reg_count == 0;
        a.ticket = (unsigned *)(sm + SM_TICKET); a.err = (unsigned *)(sm + SM_ERR); a.ticket_mode = ctx->ticket_atomic ? 0 : tune_int("SZ_HIP_TICKET_MODE", 2);
        a.progress = (szh_u64 *)ctx->progress.p; a.backoff = SZH_FILL_BACKOFF; a.wide = pencil_wide<T>(G, nJ);
        HIPCHK(hipEventRecord(ctx->ev[2], st));
        if (dec_beam) {
            TRY((launch_beam<T, true>(ctx, G, a, st, reg_count))); S.quant_kernel = 2;
        }
        else {
        const unsigned pgrid = pencil_grid(ctx, a, ntiles);
        hipLaunchKernelGGL((k_pencil<T, true>), dim3(pgrid), dim3((TS::TPI * TS::TPJ + 2) * 64), 0, st, a);
        HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ctx->ev[3], st));
        S.quant_kernel_launches = 1;
    }
    unsigned kerr = 0;
    HIPCHK(hipMemcpyAsync(&kerr, sm + SM_ERR, 4, hipMemcpyDeviceToHost, st));
    TRY(return_out(ctx, out, out_on_device, d_out, (size_t)n));
    HIPCHK(hipEventRecord(ctx->ev[4], st));
    HIPCHK(hipStreamSynchronize(st));
    if (checks_last) TRY(decoder_checks());
    if (kerr) { ctx->wave_timeout = true; FAIL(SZHIP_ERR_INTERNAL, "wavefront kernel: halo wait timed out"); }
    decompress_times(ctx, S, host_ms, t_begin, (size_t)n * sizeof(T));
    if (stats) *stats = S;
    return SZHIP_OK;
}
