// szhip_steps.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace, behind szhip_rt.inc): the steps of a call that the
// SZ 2.1, SZ 1.4 and OpenMP-container paths have in common, one definition each.  A step that would have to ask which path calls it is not here.
// ---- what every call carries: its context and first stream, when it began, the host's share of its time, its statistics
struct call_base {
    szhip_ctx *const ctx; const hipStream_t st; const double t_begin = now_ms(); double host_ms = 0; szhip_stats S;
    explicit call_base(szhip_ctx *c) : ctx(c), st(c->stream) { memset(&S, 0, sizeof(S)); }
    int done(szhip_stats *stats) const { if (stats) *stats = S; return SZHIP_OK; }
};
// ---- the call's arrays
// the caller's array where the kernels read it: as it is when it lies on the device, else staged into the context's input buffer
template <class T> int stage_input(szhip_ctx *ctx, const void *data, int on_device, size_t n, const T **d_in) {
    *d_in = (const T *)data;
    if (on_device) return SZHIP_OK;
    TRY(ensure(ctx, ctx->in, n * sizeof(T)));
    TRY(staged_copy(ctx, ctx->in.p, data, n * sizeof(T), true));
    *d_in = (const T *)ctx->in.p;
    return SZHIP_OK;
}
// where the kernels write the decoded array: the caller's device array, else the context's output buffer ...
template <class T> int device_out(szhip_ctx *ctx, void *out, int on_device, size_t n, T **d_out) {
    *d_out = (T *)out;
    if (on_device) return SZHIP_OK;
    TRY(ensure(ctx, ctx->out, n * sizeof(T)));
    *d_out = (T *)ctx->out.p;
    return SZHIP_OK;
}
// ... from which it goes back to the caller's host array
template <class T> int return_out(szhip_ctx *ctx, void *out, int on_device, const T *d_out, size_t n) {
    return on_device ? SZHIP_OK : staged_copy(ctx, out, d_out, n * sizeof(T), false);
}
// the "small" device scratch (SM_*), cleared on the first stream
int clear_small(szhip_ctx *ctx, u64 **sm) {
    TRY(ensure(ctx, ctx->small, SM_COUNT * 8));
    *sm = (u64 *)ctx->small.p;
    HIPCHK(hipMemsetAsync(*sm, 0, SM_COUNT * 8, ctx->stream));
    return SZHIP_OK;
}
// ---- interval count from a radius histogram (sz_float.c:4644-4700): the radius that covers pred_threshold of the samples, doubled, rounded up to a power of two
template <class H> unsigned pick_intervals(const H *hist, unsigned max_radius, float pred_threshold, unsigned floor_) {
    u64 total = 0;
    for (unsigned i = 0; i < max_radius; ++i) total += hist[i];
    const size_t target = (size_t)((float)total * pred_threshold);       // `size_t targetCount = totalSampleSize*predThreshold`
    size_t sum = 0; unsigned i = 0;
    for (; i < max_radius; ++i) { sum += hist[i]; if (sum > target) break; }
    if (i >= max_radius) i = max_radius - 1;
    unsigned p2 = 2 * (i + 1); p2 -= 1; p2 |= p2 >> 1; p2 |= p2 >> 2; p2 |= p2 >> 4; p2 |= p2 >> 8; p2 |= p2 >> 16; p2 += 1;
    return p2 < floor_ ? floor_ : p2;
}
// the SZ 1.4 interval optimiser (optimize_intervals_float_{1,2,3}D_opt) on the SZ 2.1 sample lattice, radius histogram only: sampled on the device into
// ctx->hist, the count chosen on the host.  `one_d`: the 1-D lattice (sz_float.c:4413).  `p0` / `p1` (3-D only; 0: the array is contiguous): the element pitches of
// a view whose sub-box `G` describes -- the same samples through k_sample_view / k_sample_walk_view
template <class T>
int sampled_intervals(szhip_ctx *ctx, const szh_geom3 &G, bool one_d, const T *d_in, const szhip_params *prm, T eb, u64 *sm, unsigned *intervals, double *host_ms,
                      int64_t p0 = 0, int64_t p1 = 0) {
    const bool view = p1 != 0 && (p0 != G.d0 || p1 != G.d1);
    hipStream_t st = ctx->stream;
    const unsigned max_radius = prm->max_quant_intervals / 2;
    TRY(ensure(ctx, ctx->hist, (size_t)(max_radius + 8192) * 4 + 64));
    TRY(ensure_pinned(ctx, (size_t)(max_radius + 8192) * 4 + 64));
    unsigned *d_rh = (unsigned *)ctx->hist.p, *d_fh = d_rh + max_radius;
    HIPCHK(hipMemsetAsync(d_rh, 0, (size_t)(max_radius + 8192) * 4, st));
    const int64_t n = G.n, nrows = one_d ? 0 : szh_sample_row_limit(G, prm->sample_distance);
    if (one_d) {
        const int64_t count = (n - 2 + prm->sample_distance - 1) / prm->sample_distance;
        int grid = (int)std::min<int64_t>((count + 255) / 256 + 1, 1024);
        hipLaunchKernelGGL((k_sample_1d<T>), dim3(grid), dim3(256), 0, st, d_in, n, prm->sample_distance, (double)eb, max_radius, d_rh);
        HIPCHK(hipGetLastError());
    } else if (G.ndim == 3 && (G.g0.count <= 1 || G.g1.count <= 1)) {      // a degenerate 3-D array: the reference's walk, literally
        if (view) hipLaunchKernelGGL((k_sample_walk_view<T>), dim3(1), dim3(64), 0, st, G, d_in, p0, p1, prm->sample_distance, (double)eb, max_radius, d_rh, sm + SM_WITHIN);
        else hipLaunchKernelGGL((k_sample_walk<T, false>), dim3(1), dim3(64), 0, st, G, d_in, prm->sample_distance, (double)eb, (T)0, max_radius, d_rh, d_fh, sm + SM_WITHIN);
        HIPCHK(hipGetLastError());
    } else if (nrows > 0) {
        int grid = (int)std::min<int64_t>((nrows + 255) / 256, 1024);
        if (view) hipLaunchKernelGGL((k_sample_view<T>), dim3(grid), dim3(256), 0, st, G, d_in, p0, p1, nrows, prm->sample_distance, (double)eb, max_radius, d_rh, sm + SM_WITHIN);
        else hipLaunchKernelGGL((k_sample<T, false>), dim3(grid), dim3(256), 0, st, G, d_in, nrows, prm->sample_distance, (double)eb, (T)0,
                                max_radius, d_rh, d_fh, sm + SM_WITHIN);
        HIPCHK(hipGetLastError());
    }
    unsigned *h_rh = (unsigned *)ctx->pinned;
    HIPCHK(hipMemcpyAsync(h_rh, d_rh, (size_t)max_radius * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const double h0 = now_ms();
    *intervals = pick_intervals(h_rh, max_radius, prm->pred_threshold, 32u);
    *host_ms += now_ms() - h0;
    return SZHIP_OK;
}
// ---- histogram of the codes [first, end) of an array (k_hist_u16) into d_hist, cleared by the caller: lane-private copies of the bins in LDS, as many as fit `cap_bins`
static int hist_rshift(unsigned intervals, size_t cap_bins) { int r = 0; while (r < 6 && ((size_t)intervals << (r + 1)) <= cap_bins) ++r; return r; }
int launch_hist_u16(szhip_ctx *ctx, hipStream_t s_, const uint16_t *d_codes, int64_t first, int64_t end, unsigned intervals, unsigned *d_hist) {
    const int use_lds = intervals <= 16384, rshift = use_lds ? hist_rshift(intervals, 16384) : 0;
    const size_t lds = use_lds ? ((size_t)intervals << rshift) * 4 : 16;
    int grid = (int)std::min<int64_t>(((end - first) / 8 + 255) / 256 + 1, 2048);
    hipLaunchKernelGGL(k_hist_u16, dim3(grid), dim3(256), lds, s_, d_codes, end, intervals, rshift, use_lds, d_hist, first);
    HIPCHK(hipGetLastError());
    return SZHIP_OK;
}
// ---- Huffman code books on the host (szhost.c); the handle frees the book on every return
struct huff_free { void operator()(szhost_huff *h) const { szhost_huff_free(h); } };
using huff_ptr = std::unique_ptr<szhost_huff, huff_free>;
// the book of a histogram (empty: the build failed) and the device's tables of it: right-aligned code bits + lengths, one entry per symbol < intervals
huff_ptr host_book(const unsigned *h_hist, unsigned intervals, std::vector<u64> &tab_code, std::vector<uint8_t> &tab_len, unsigned *maxlen) {
    huff_ptr hf(szhost_huff_build(2 * (int)intervals, h_hist, nullptr, intervals));
    if (!hf) return hf;
    tab_code.resize(intervals); tab_len.resize(intervals);
    *maxlen = 0;
    for (unsigned s = 0; s < intervals; ++s) { tab_code[s] = hf->code[s]; tab_len[s] = hf->len[s]; *maxlen = std::max<unsigned>(*maxlen, hf->len[s]); }
    return hf;
}
int upload_code_tables(szhip_ctx *ctx, const std::vector<u64> &tab_code, const std::vector<uint8_t> &tab_len) {
    TRY(ensure(ctx, ctx->code_tab, tab_code.size() * 8));
    TRY(ensure(ctx, ctx->len_tab, tab_len.size()));
    HIPCHK(hipMemcpyAsync(ctx->code_tab.p, tab_code.data(), tab_code.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->len_tab.p, tab_len.data(), tab_len.size(), hipMemcpyHostToDevice, ctx->stream));
    return SZHIP_OK;
}
// what the device's decoders need of a stream's serialised tree (`node_count` nodes at `tree`): the node table, and the symbol of a one-leaf tree (zero payload bits)
struct dec_table { std::vector<uint32_t> dtab; int n_nodes = 0, single_symbol = -1; };
bool read_tree(const unsigned char *tree, int node_count, unsigned intervals, dec_table &D) {
    const huff_ptr hf(szhost_huff_from_bytes(2 * (int)intervals, tree, node_count));
    if (!hf) return false;
    D.dtab.resize((size_t)hf->n_nodes * 2);
    szhost_huff_decode_table(hf.get(), D.dtab.data());
    D.single_symbol = hf->t[0] ? (int)hf->C[0] : -1;
    D.n_nodes = hf->n_nodes;
    return true;
}
// ---- linear packing of a code array: the bits of every chunk (k_chunk_bits), their exclusive scan (the total to SM_TOTAL_BITS) ...
// (`slack`: what the caller has always asked for behind the chunks' bit counts -- 64 bytes for SZ 2.1, none for SZ 1.4 --, so that the buffer grows as it did)
int chunk_bit_offsets(szhip_ctx *ctx, const uint16_t *d_codes, int64_t n, unsigned intervals, u64 *sm, size_t slack) {
    const int64_t nchunks = (n + SZH_ENC_CHUNK - 1) / SZH_ENC_CHUNK;
    TRY(ensure(ctx, ctx->chunk_bits, (size_t)nchunks * 8 + slack));
    TRY(ensure(ctx, ctx->chunk_off, (size_t)nchunks * 8));
    hipLaunchKernelGGL(k_chunk_bits, dim3((unsigned)((nchunks + SZH_CB_PER - 1) / SZH_CB_PER)), dim3(256), 0, ctx->stream, d_codes, n, (const uint8_t *)ctx->len_tab.p, intervals, (u64 *)ctx->chunk_bits.p);
    return scan_u64(ctx, (const u64 *)ctx->chunk_bits.p, nchunks, (u64 *)ctx->chunk_off.p, sm + SM_TOTAL_BITS);
}
// ... and k_encode, which packs the chunks behind `base_bits` of the stream
int launch_encode(szhip_ctx *ctx, const uint16_t *d_codes, int64_t n, unsigned intervals, u64 base_bits, unsigned char *d_stream) {
    const int64_t nchunks = (n + SZH_ENC_CHUNK - 1) / SZH_ENC_CHUNK;
    hipLaunchKernelGGL(k_encode, dim3((unsigned)((nchunks + SZH_ENC_PER - 1) / SZH_ENC_PER)), dim3(256), 0, ctx->stream, d_codes, n, (const u64 *)ctx->code_tab.p,
                       (const uint8_t *)ctx->len_tab.p, intervals, (const u64 *)ctx->chunk_off.p, base_bits, (unsigned *)d_stream);
    HIPCHK(hipGetLastError());
    return SZHIP_OK;
}
// ---- the stream to the caller: into its device buffer (of capacity *out_size; `in_place`: it was written there), as a pointer into the context's buffer, or as a
// malloc'd host copy; synchronises the first stream unless that is behind the caller (`synced`) and nothing was enqueued since
int deliver_stream(szhip_ctx *ctx, unsigned char *d_stream, size_t len, int out_on_device, unsigned char **out, size_t *out_size, bool in_place, bool synced) {
    hipStream_t st = ctx->stream;
    if (out_on_device == 2) {
        if (!*out || *out_size < len) FAIL(SZHIP_ERR_ARG, "caller's device buffer too small (%zu < %zu)", *out_size, len);
        if (!in_place) { HIPCHK(hipMemcpyAsync(*out, d_stream, len, hipMemcpyDeviceToDevice, st)); synced = false; }
        if (!synced) HIPCHK(hipStreamSynchronize(st));
    } else if (out_on_device) {
        if (!synced) HIPCHK(hipStreamSynchronize(st));
        *out = d_stream;
    } else {
        unsigned char *h = (unsigned char *)malloc(len ? len : 1);
        if (!h) FAIL(SZHIP_ERR_INTERNAL, "out of host memory");
        const int rc_copy = staged_copy(ctx, h, d_stream, len, false);
        if (rc_copy != SZHIP_OK) { free(h); return rc_copy; }
        *out = h;
    }
    *out_size = len;
    return SZHIP_OK;
}
// ---- a decompress call's intake: the whole stream into the context's buffer, 64 zero bytes behind it (the bit readers may look a few bytes past the end), ev[0]
// recorded; the host reads the header where the caller has it, or -- a device-resident stream -- from prefixes fetched as the header turns out to need them
struct stream_intake {
    szhip_ctx *const ctx; const unsigned char *const stream_in; const int on_device; const size_t stream_len;
    unsigned char *d_stream = nullptr;
    const unsigned char *hs;                                   // the stream on the host (valid up to the last fetch)
    std::vector<unsigned char> hbuf;
    stream_intake(szhip_ctx *c, const unsigned char *s, int od, size_t len) : ctx(c), stream_in(s), on_device(od), stream_len(len), hs(s) {}
    bool whole = true;                                         // false (a region call): the stream stays where it is, d_stream is the caller's device pointer or null
    int open() {
        hipStream_t st = ctx->stream;
        if (!whole) { d_stream = on_device ? const_cast<unsigned char *>(stream_in) : nullptr; HIPCHK(hipEventRecord(ctx->ev[0], st)); return SZHIP_OK; }
        TRY(ensure(ctx, ctx->stream_buf, stream_len + 64));
        d_stream = (unsigned char *)ctx->stream_buf.p;
        if (on_device) { if (stream_in != d_stream) HIPCHK(hipMemcpyAsync(d_stream, stream_in, stream_len, hipMemcpyDeviceToDevice, st)); }
        else TRY(staged_copy(ctx, d_stream, stream_in, stream_len, true));
        HIPCHK(hipMemsetAsync(d_stream + stream_len, 0, 64, st));
        HIPCHK(hipEventRecord(ctx->ev[0], st));
        return SZHIP_OK;
    }
    int fetch(size_t want)                                     // the first `want` bytes of the stream on the host
    {
        if (want > stream_len) FAIL(SZHIP_ERR_STREAM, "truncated stream");
        if (!on_device) return SZHIP_OK;
        hbuf.resize(want);
        HIPCHK(hipMemcpyAsync(hbuf.data(), d_stream, want, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        hs = hbuf.data();
        return SZHIP_OK;
    }
};
// ---- the device times of a call into its statistics: ev[0..1] before the quantiser, ev[2..3] the quantiser, ev[3..4] the entropy stage of a compress call ...
void compress_times(szhip_ctx *ctx, szhip_stats &S, double host_ms, double t_begin, size_t out_bytes) {
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); S.ms_prequant = ms;
    hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]); S.ms_quant = ms;
    hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]); S.ms_entropy = ms;
    S.ms_host = host_ms; S.ms_total = now_ms() - t_begin; S.out_bytes = out_bytes;
}
// ... of a decompress call ev[0..1] the entropy stage and what follows it, ev[2..3] the inverse sweep
void decompress_times(szhip_ctx *ctx, szhip_stats &S, double host_ms, double t_begin, size_t out_bytes) {
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); S.ms_entropy = ms;
    hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]); S.ms_quant = ms;
    S.ms_host = host_ms; S.ms_total = now_ms() - t_begin; S.out_bytes = out_bytes;
}
