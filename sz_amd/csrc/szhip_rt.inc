// szhip_rt.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace): the context's buffers, streams, staging copies and the sweep launchers every path uses.

#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            snprintf(ctx->err, sizeof(ctx->err), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            fprintf(stderr, "szhip: %s\n", ctx->err);                                                  \
            return SZHIP_ERR_NODEVICE;                                                                 \
        }                                                                                              \
    } while (0)

#define FAIL(code, ...)                                                                                \
    do {                                                                                               \
        snprintf(ctx->err, sizeof(ctx->err), __VA_ARGS__);                                             \
        fprintf(stderr, "szhip: %s\n", ctx->err);                                                      \
        return (code);                                                                                 \
    } while (0)
// a failure found AFTER the stream has been handed to the caller's pointer: a host copy that this call malloc'd is released again
#define FAIL_PUBLISHED(code, ...)                                                                      \
    do {                                                                                               \
        if (!out_on_device && out && *out) { free(*out); *out = nullptr; }                              \
        if (out_size) *out_size = 0;                                                                   \
        FAIL(code, __VA_ARGS__);                                                                       \
    } while (0)

int ensure(szhip_ctx *ctx, DevBuf &b, size_t bytes, bool zero_new = false)
{
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return SZHIP_OK;
    if (b.p) { HIPCHK(hipStreamSynchronize(ctx->stream)); HIPCHK(hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    size_t cap = bytes + bytes / 8 + 256;
    HIPCHK(hipMalloc(&b.p, cap));
    b.cap = cap;
    if (zero_new) HIPCHK(hipMemsetAsync(b.p, 0, cap, ctx->stream));
    return SZHIP_OK;
}

#define TRY(x) do { int rc_ = (x); if (rc_ != SZHIP_OK) return rc_; } while (0)

// the context's grow-only pinned host buffers: a buffer that must grow is released once the stream whose copies use it has drained
int ensure_host(szhip_ctx *ctx, void *&p, size_t &have, size_t bytes, hipStream_t user, unsigned flags = hipHostMallocDefault)
{
    if (have >= bytes) return SZHIP_OK;
    if (p) { HIPCHK(hipStreamSynchronize(user)); HIPCHK(hipHostFree(p)); p = nullptr; have = 0; }
    size_t cap = bytes + bytes / 4 + 4096;
    HIPCHK(hipHostMalloc(&p, cap, flags));
    have = cap;
    return SZHIP_OK;
}
int ensure_pinned(szhip_ctx *ctx, size_t bytes) { return ensure_host(ctx, ctx->pinned, ctx->pinned_cap, bytes, ctx->stream); }
int ensure_pinned2(szhip_ctx *ctx, size_t bytes) { return ensure_host(ctx, ctx->pinned2, ctx->pinned2_cap, bytes, ctx->stream2); }
int ensure_pinned3(szhip_ctx *ctx, size_t bytes) { return ensure_host(ctx, ctx->pinned3, ctx->pinned3_cap, bytes, ctx->stream); }
int ensure_coherent(szhip_ctx *ctx, size_t bytes)
{
    const size_t had = ctx->coh_cap;
    TRY(ensure_host(ctx, ctx->coh, ctx->coh_cap, bytes, ctx->stream, hipHostMallocCoherent | hipHostMallocMapped));
    if (ctx->coh_cap != had) memset(ctx->coh, 0, ctx->coh_cap);      // (epoch-tagged words live here: none may look current by accident)
    return SZHIP_OK;
}

// layout of the "small" device scratch (u64 slots)
enum { SM_MINMAX = 0, SM_WITHIN = 2, SM_MEANCNT = 3, SM_TOTAL_UNPRED = 4, SM_TOTAL_BITS = 5, SM_TICKET = 6, SM_ERR = 7,
       SM_CHANGED = 8, SM_MEANSUM = 9, SM_TOTAL_SYM = 10, SM_NREG = 11, SM_SCRATCH = 12, SM_COUNT = 16 };

// Does a copy on the second stream complete while a kernel on the first one is still running?  HIP maps streams onto a few hardware
// queues; two streams of one context can land on the same queue (seen with several contexts + torch in one process), and then anything
// queued behind a kernel that WAITS for it is a deadlock.  Probed once per context: a kernel on `stream` spins (bounded, ~4 ms) on a
// host-coherent word; a small copy goes onto `stream2`; if it completes while the kernel is still spinning the queues are independent.
int probe_streams(szhip_ctx *ctx)
{
    if (ctx->streams_independent >= 0) return SZHIP_OK;
    TRY(ensure_coherent(ctx, 256));
    TRY(ensure(ctx, ctx->small, SM_COUNT * 8));
    volatile unsigned long long *flag = (volatile unsigned long long *)((char *)ctx->coh + 128);
    unsigned long long *src = (unsigned long long *)((char *)ctx->coh + 192);
    *flag = 0; *src = 1;
    HIPCHK(hipStreamSynchronize(ctx->stream)); HIPCHK(hipStreamSynchronize(ctx->stream2));
    u64 *sm = (u64 *)ctx->small.p;
    hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(1), 0, ctx->stream, (const unsigned long long *)flag, (unsigned long long *)(sm + SM_SCRATCH));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sm + SM_SCRATCH + 1, src, 8, hipMemcpyHostToDevice, ctx->stream2));
    const double t0 = now_ms();
    HIPCHK(hipStreamSynchronize(ctx->stream2));
    const double waited = now_ms() - t0;
    *flag = 1;                                                      // release the kernel
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->streams_independent = waited < 2.0 ? 1 : 0;
    return SZHIP_OK;
}

// Do kernels on `b` run while a kernel on `a` is still running?  (As above, with a kernel instead of the copy.)  *shared = 1: no, the two
// streams sit on one hardware queue.
static int probe_pair(szhip_ctx *ctx, hipStream_t a, hipStream_t b, int *shared)
{
    TRY(ensure_coherent(ctx, 256));
    TRY(ensure(ctx, ctx->small, SM_COUNT * 8));
    volatile unsigned long long *flag = (volatile unsigned long long *)((char *)ctx->coh + 128);
    *flag = 0;
    HIPCHK(hipStreamSynchronize(a)); HIPCHK(hipStreamSynchronize(b));
    u64 *sm = (u64 *)ctx->small.p;
    hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(1), 0, a, (const unsigned long long *)flag, (unsigned long long *)(sm + SM_SCRATCH));
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_probe_touch, dim3(1), dim3(1), 0, b, (unsigned long long *)(sm + SM_SCRATCH + 1));
    HIPCHK(hipGetLastError());
    const double t0 = now_ms();
    HIPCHK(hipStreamSynchronize(b));
    const double waited = now_ms() - t0;
    *flag = 1;                                                      // release the kernel
    HIPCHK(hipStreamSynchronize(a));
    *shared = waited < 2.0 ? 0 : 1;
    return SZHIP_OK;
}

// HIP maps the streams of a process onto a few hardware queues, and two streams on one queue run their kernels one after the other.  Which
// streams share a queue is the luck of what else the process has created.  Measured (round 4, 512^3 float32, one call after the other):
// 236 - 241 GB/s when a context's second stream (the fit pass beside the sampling chain, the histogram beside the block ordering) or third stream
// (the slices' passes beside the sweep) sat on the main stream's queue, 274 - 279 otherwise; two lanes of a pool whose main streams shared a queue:
// 248 GB/s against 340.  So a new context PROBES: a kernel that waits (bounded, ~4 ms) on the one stream, a trivial kernel on the other; a side
// stream that does not get through is replaced by a freshly created one (the rejected streams stay alive until the search is over, so that the
// runtime's next choice is another queue), a few times over.  `mains`: the main streams of the pool's earlier lanes (a lane's streams must
// not share a queue with those either).
static void settle_one(szhip_ctx *ctx, hipStream_t *victim, const std::vector<hipStream_t> &against, std::vector<hipStream_t> &rejected, int *probes)
{
    for (int attempt = 0; attempt < 6; ++attempt) {
        bool clash = false;
        for (hipStream_t a : against) {
            if (a == *victim) continue;
            int shared = 0;
            ++*probes;
            if (probe_pair(ctx, a, *victim, &shared) != SZHIP_OK) return;
            if (shared) { clash = true; break; }
        }
        if (!clash) return;
        hipStream_t fresh = nullptr;
        if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) != hipSuccess) return;
        rejected.push_back(*victim);
        *victim = fresh;
    }
}
static void settle_streams(szhip_ctx *ctx, const hipStream_t *mains, int n_mains, bool third = true)
{
#ifdef SZH_SYNC_LAUNCH
    (void)ctx; (void)mains; (void)n_mains; (void)third;             // (the CPU shim runs every kernel at its launch)
#else
    std::vector<hipStream_t> rejected, against(mains, mains + n_mains);
    int probes = 0;
    if (n_mains) settle_one(ctx, &ctx->stream, against, rejected, &probes);      // this lane's main stream against the earlier lanes'
    against.push_back(ctx->stream);
    settle_one(ctx, &ctx->stream2, against, rejected, &probes);
    if (third && !ctx->stream3 && hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking) != hipSuccess) ctx->stream3 = nullptr;
    if (third && ctx->stream3) { against.push_back(ctx->stream2); settle_one(ctx, &ctx->stream3, against, rejected, &probes); }
    ctx->settle_probes = probes; ctx->settle_rejected = (int)rejected.size();
    for (hipStream_t r : rejected) hipStreamDestroy(r);
#endif
}

// ---- bulk copies between pageable host memory and the device.
// hipMemcpyAsync on pageable memory makes the runtime pin and unpin the caller's pages around the transfer: measured on this pool,
// 512 MiB host-to-device ran at 11-25 GB/s depending on the box, device-to-host into a fresh malloc at 3.4 GB/s, and the deferred
// unpinning stalled LATER calls (see the coefficient transfers in compress_impl).  Here the array is cut into 8 MiB chunks; SZH_STAGE_T
// host threads each own two pinned buffers and take every SZH_STAGE_T-th chunk: memcpy into (out of) a pinned buffer, asynchronous DMA on
// the context's stream, the other buffer meanwhile.  The call returns when the last byte has arrived.
// The host side may be a VIEW (`hv`; the calls that take pitches): rows of hv->row bytes, hv->pitch1 bytes apart, hv->r1 of them a plane, planes hv->pitch0
// bytes apart.  The device side stays contiguous, so only the rows' bytes cross the bus: the memcpy into (out of) the pinned buffer walks the rows.
int tune_int(const char *name, int def);
constexpr size_t SZH_STAGE_CHUNK = 8u << 20;
struct host_view { size_t r1, row, pitch0, pitch1; };
// bytes [off, off + len) of the view's packed order: out of the view at `base` into `buf` (gather) or out of `buf` into the view
static void host_view_move(const host_view &v, char *base, char *buf, size_t off, size_t len, bool gather)
{
    size_t rw = off / v.row, col = off - rw * v.row;
    while (len) {
        const size_t k = rw / v.r1, i = rw - k * v.r1, take = std::min(len, v.row - col);
        char *p = base + k * v.pitch0 + i * v.pitch1 + col;
        if (gather) memcpy(buf, p, take); else memcpy(p, buf, take);
        buf += take; len -= take; col = 0; ++rw;
    }
}
int staged_copy(szhip_ctx *ctx, void *dst, const void *src, size_t bytes, bool to_device, const host_view *hv = nullptr)
{
    hipStream_t st = ctx->stream;
    // (SZ_HIP_STAGE_CHUNK_KB: smaller chunks, so that tests reach this path with small arrays)
    const size_t chunk = std::min(SZH_STAGE_CHUNK, (size_t)std::max(1, tune_int("SZ_HIP_STAGE_CHUNK_KB", (int)(SZH_STAGE_CHUNK >> 10))) << 10);
    if (bytes < 4 * chunk && hv) {                                 // a small view: through one pinned buffer
        TRY(ensure_pinned3(ctx, bytes));
        HIPCHK(hipStreamSynchronize(st));
        if (to_device) host_view_move(*hv, (char *)const_cast<void *>(src), (char *)ctx->pinned3, 0, bytes, true);
        HIPCHK(hipMemcpyAsync(to_device ? dst : ctx->pinned3, to_device ? ctx->pinned3 : src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!to_device) host_view_move(*hv, (char *)dst, (char *)ctx->pinned3, 0, bytes, false);
        return SZHIP_OK;
    }
    if (bytes < 4 * chunk) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return SZHIP_OK;
    }
    constexpr int nthr = SZH_STAGE_T;
    for (int w = 0; w < nthr; ++w)
        for (int k = 0; k < 2; ++k)
            if (!ctx->stage_buf[w][k]) {
                HIPCHK(hipHostMalloc(&ctx->stage_buf[w][k], SZH_STAGE_CHUNK, hipHostMallocDefault));
                HIPCHK(hipEventCreateWithFlags(&ctx->stage_ev[w][k], hipEventDisableTiming));
            }
    HIPCHK(hipStreamSynchronize(st));                              // the source (destination) is ready (free) from here on
    const size_t nchunks = (bytes + chunk - 1) / chunk;
    std::atomic<int> failed(0);
    const int device = ctx->device;
    // the host's end of a chunk: the caller's contiguous array, or the rows of its view
    auto host_in = [&](void *buf, size_t off, size_t len) {
        if (hv) host_view_move(*hv, (char *)const_cast<void *>(src), (char *)buf, off, len, true); else memcpy(buf, (const char *)src + off, len);
    };
    auto host_out = [&](const void *buf, size_t off, size_t len) {
        if (hv) host_view_move(*hv, (char *)dst, (char *)const_cast<void *>(buf), off, len, false); else memcpy((char *)dst + off, buf, len);
    };
    auto worker = [&](int w) {
        if (hipSetDevice(device) != hipSuccess) { failed = 1; return; }
        size_t pend_off[2] = {0, 0}, pend_len[2] = {0, 0};        // device-to-host: the chunk in flight into buffer k
        bool pend[2] = {false, false};
        int k = 0;
        for (size_t c = (size_t)w; c < nchunks && !failed; c += (size_t)nthr, k ^= 1) {
            const size_t off = c * chunk, len = std::min(chunk, bytes - off);
            if (to_device) {
                if (pend[k] && hipEventSynchronize(ctx->stage_ev[w][k]) != hipSuccess) { failed = 1; return; }   // buffer k is free again
                host_in(ctx->stage_buf[w][k], off, len);
                if (hipMemcpyAsync((char *)dst + off, ctx->stage_buf[w][k], len, hipMemcpyHostToDevice, st) != hipSuccess ||
                    hipEventRecord(ctx->stage_ev[w][k], st) != hipSuccess) { failed = 1; return; }
                pend[k] = true;
            } else {
                if (pend[k]) {                                     // the chunk that went into buffer k two rounds ago: hand it to the caller
                    if (hipEventSynchronize(ctx->stage_ev[w][k]) != hipSuccess) { failed = 1; return; }
                    host_out(ctx->stage_buf[w][k], pend_off[k], pend_len[k]);
                }
                if (hipMemcpyAsync(ctx->stage_buf[w][k], (const char *)src + off, len, hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipEventRecord(ctx->stage_ev[w][k], st) != hipSuccess) { failed = 1; return; }
                pend[k] = true; pend_off[k] = off; pend_len[k] = len;
            }
        }
        for (int q = 0; q < 2; ++q, k ^= 1) {                      // drain, oldest first
            if (!pend[k]) continue;
            if (hipEventSynchronize(ctx->stage_ev[w][k]) != hipSuccess) { failed = 1; return; }
            if (!to_device) host_out(ctx->stage_buf[w][k], pend_off[k], pend_len[k]);
        }
    };
    std::vector<std::thread> th;
    for (int w = 1; w < nthr; ++w) th.emplace_back(worker, w);
    worker(0);
    for (auto &t : th) t.join();
    if (failed) FAIL(SZHIP_ERR_NODEVICE, "staged %s copy failed", to_device ? "host-to-device" : "device-to-host");
    return SZHIP_OK;
}

// an environment switch (INTEGRATION.md lists them), read on every call so that tests can set it between calls
int tune_int(const char *name, int def)
{
    const char *e = getenv(name);
    return e ? atoi(e) : def;
}

// device-wide exclusive scan of u64 in[0..n) -> out; total to *total_dev (device u64)
int scan_u64(szhip_ctx *ctx, const u64 *in, int64_t n, u64 *out, u64 *total_dev, hipStream_t on = nullptr)
{
    const hipStream_t sst = on ? on : ctx->stream;
    const int64_t nblk = (n + SZH_SCAN_TILE - 1) / SZH_SCAN_TILE;
    TRY(ensure(ctx, ctx->partial, (size_t)(nblk + 1) * 8));
    u64 *partial = (u64 *)ctx->partial.p;
    hipLaunchKernelGGL(k_scan_partials, dim3((unsigned)nblk), dim3(256), 0, sst, in, n, partial);
    hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(256), 0, sst, partial, nblk, total_dev);
    hipLaunchKernelGGL(k_scan_final, dim3((unsigned)nblk), dim3(256), 0, sst, in, n, (const u64 *)partial, out);
    HIPCHK(hipGetLastError());
    return SZHIP_OK;
}

constexpr size_t SZH_PERM_TILE_BYTES = 32 * 1024;   // the tile budget of k_permute (choose_segb)
int choose_segb(const szh_geom3 &G, size_t elem, size_t budget)
{
    const size_t rows = (size_t)G.g0.early * G.g1.early;
    size_t per_block = rows * (size_t)G.g2.early * elem;
    int segb = (int)(budget / (per_block ? per_block : 1));
    if (segb < 1) segb = 1;
    if (segb > 32) segb = 32;
    if (segb > G.g2.num) segb = G.g2.num;
    return segb;
}
// tile of k_permute: rows widened to 16-byte vector boundaries, pitch a multiple of 8 elements
size_t tile_bytes(const szh_geom3 &G, int segb, size_t elem)
{
    const size_t rows = (size_t)G.g0.early * G.g1.early;
    const size_t kp = ((size_t)segb * G.g2.early + 31) & ~(size_t)7;
    return rows * kp * elem + 16;
}

// buffers of the wavefront kernel: granule faces, progress words, start order of the tiles (tpi x tpj pencils each)
int prepare_pencil(szhip_ctx *ctx, const szh_geom3 &G, int nw, int tpi, int tpj, int *nI_out, int *nJ_out, int *ntiles_out)
{
    const int nI = (G.g0.count + 7) / 8, nJ = (G.g1.count + 7) / 8;
    if (nI > 65535 || nJ > 65535) FAIL(SZHIP_ERR_UNSUP, "dimension too large for the pencil grid");
    const size_t rowg = (size_t)G.g2.count * nw * sizeof(u64);
    TRY(ensure(ctx, ctx->faceI, (size_t)nI * nJ * 9 * rowg + 64, true));   // + 64: a 16-byte granule pair may reach one granule past a row's end
    TRY(ensure(ctx, ctx->faceJ, (size_t)nI * nJ * 8 * rowg + 64, true));
    TRY(ensure(ctx, ctx->progress, (size_t)nI * nJ * 2 * sizeof(u64), true));
    const int nTI = (nI + tpi - 1) / tpi, nTJ = (nJ + tpj - 1) / tpj;
    if (ctx->order_nI != nTI || ctx->order_nJ != nTJ) {
        std::vector<unsigned> ord((size_t)nTI * nTJ);
        szh_fill_pencil_order(nTI, nTJ, ord.data());
        TRY(ensure(ctx, ctx->order, ord.size() * 4));
        HIPCHK(hipMemcpyAsync(ctx->order.p, ord.data(), ord.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        ctx->order_nI = nTI; ctx->order_nJ = nTJ;
    }
    *nI_out = nI; *nJ_out = nJ; *ntiles_out = nTI * nTJ;
    return SZHIP_OK;
}

// k_pencil's FILL wavefront: sleep units between two rounds that delivered nothing
constexpr int SZH_FILL_BACKOFF = 4;
// k_pencil: the granule rows of a tile lie within 4 GB of the tile's first row (16-byte buffer accesses with 32-bit offsets)
template <class T> static int pencil_wide(const szh_geom3 &G, int nJ)
{
    using TS = szh_tile_shape<T>;
    return (double)TS::TPI * nJ * 9.0 * (double)G.g2.count * szh_gran<T>::NW * 8.0 < 4.0e9 && (double)TS::TPJ * 9.0 * (double)G.g2.count * szh_gran<T>::NW * 8.0 < 4.0e9;
}
// k_pencil's grid: one workgroup per tile (a lone context: the inverse sweep at 512^3 takes 1.47 ms either way), or that many persistent
// workgroups drawing tiles from the ticket counter (a pool lane: fewer workgroups that only poll for their predecessors -- two M-field
// arrays in flight 111 -> 136 GB/s with 512, 127 with 256).
template <class QA> static unsigned pencil_grid(szhip_ctx *ctx, QA &a, int ntiles)
{
    const int cap = ctx->gate ? 512 : 0;
    a.persist = cap > 0 && cap < ntiles;
    return (unsigned)(a.persist ? cap : ntiles);
}
// ---- the beam mapping of the sweep (szh_beam.h, round 5): 3-D arrays whose contiguous extent is a multiple of 4 values
// does it cover this call?  (SZ_HIP_BEAM=0 sends everything to k_pencil)
template <class T> bool beam_applies(const szh_geom3 &G, const void *base, size_t reg_count)
{
    if (!tune_int("SZ_HIP_BEAM", 1)) return false;
    (void)reg_count;                                                                               // (regression blocks: k_reg_points beside the sweep)
    if (G.ndim != 3) return false;
    if (G.g2.count < 4 || (G.g2.count & 3) != 0 || ((uintptr_t)base & 15) != 0) return false;      // 16-byte row pieces
    if ((double)G.n * sizeof(T) >= 4.0e9) return false;                                            // 32-bit buffer offsets
    const szh_bm::grid_t g = szh_bm::make_grid(G);
    if (g.nKB > 65535 || g.nJG > 65535) return false;
    return (double)szh_bm::kface_words<T>(G) * 8.0 < 4.0e9 && (double)szh_bm::jface_words<T>(G) * 8.0 < 4.0e9;
}
// granule buffers of the beams' faces + the launch; `a` carries everything that does not depend on the mapping
template <class T, bool DEC>
int launch_beam(szhip_ctx *ctx, const szh_geom3 &G, szh_qargs<T> a, hipStream_t st, size_t reg_count, bool feed = false)
{
    const szh_bm::grid_t g = szh_bm::make_grid(G);
    const size_t tiles = (size_t)g.nKB * g.nJG;
    TRY(ensure(ctx, ctx->rb_down, szh_bm::kface_words<T>(G) * sizeof(u64) + 64, true));
    TRY(ensure(ctx, ctx->rb_right, szh_bm::jface_words<T>(G) * sizeof(u64) + 64, true));
    a.faceI = (szh_u64 *)ctx->rb_down.p; a.faceJ = (szh_u64 *)ctx->rb_right.p;
    a.nI = g.nKB; a.nJ = g.nJG;
    if (a.ticket_mode == 2) a.ticket_mode = 1;
    if (ctx->gate) a.ticket_mode = 0;
#ifdef SZH_SYNC_LAUNCH
    const unsigned wgs = (unsigned)tiles;      // (the CPU shim runs workgroups one after the other: a workgroup per tile, in ticket order)
#else
    // persistent workgroups in ticket order: as many as are resident at once (a tile's predecessors hold smaller tickets)
    const int per_cu = sizeof(T) == 4 ? 2 : 1;
    const unsigned wgs = (unsigned)std::min<size_t>(tiles, (size_t)ctx->cus * per_cu);
#endif
    // arrays with regression blocks: their points are quantised / reconstructed by k_reg_points (no neighbour involved); the sweep takes
    // their reconstructions as its neighbours (compress: from a.xr; the inverse: they are in the output array already) and passes them through
    const bool hasreg = reg_count != 0;
    if (hasreg) {
        TRY(ensure(ctx, ctx->pt_flags, (size_t)G.n + 64));
#ifdef SZH_SYNC_LAUNCH
        const bool prepared = feed;            // (the CPU shim: the caller has cleared the flags and run the slices already -- a launch there runs to its end at once)
#else
        const bool prepared = false;
#endif
        if (!prepared) HIPCHK(hipMemsetAsync(ctx->pt_flags.p, 0, (size_t)G.n, st));
        a.ptflags = (const uint8_t *)ctx->pt_flags.p;
        const unsigned rgrid = (unsigned)(G.g0.num * G.g1.num);       // a workgroup per block column (b0, b1)
        if (!DEC) {
            TRY(ensure(ctx, ctx->rb_vals, (size_t)G.n * sizeof(T) + 64));
            a.xr = (const T *)ctx->rb_vals.p;
            if (feed) {
                // the regression points come in slices of block rows while the sweep runs (feed_beam_slice, called by compress_impl as the host's
                // coefficient chains advance): the sweep starts now and waits, plane by plane, on the word the slices' stream stores
                TRY(ensure(ctx, ctx->feed_word, 256));
                if (!prepared) HIPCHK(hipMemsetAsync(ctx->feed_word.p, 0, 256, st));
                a.reg_ready = (const unsigned *)ctx->feed_word.p;
                HIPCHK(hipEventRecord(ctx->ev_feed, st));             // (the slices may write flags and the word from here on)
                HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_feed, 0));
            } else
            hipLaunchKernelGGL((k_reg_points<T, 0>), dim3(rgrid), dim3(256), 0, st, G, a.blk_lor, a.coef, a.coef_stride, a.data, (T *)ctx->rb_vals.p, a.codes, (uint8_t *)ctx->pt_flags.p,
                               a.eb, a.recip, a.cap, a.radius, 0);
        } else
            hipLaunchKernelGGL((k_reg_points<T, 2>), dim3(rgrid), dim3(256), 0, st, G, a.blk_lor, a.coef, a.coef_stride, (const T *)nullptr, a.out, a.codes, (uint8_t *)ctx->pt_flags.p,
                               a.eb, a.recip, a.cap, a.radius, 0);
        HIPCHK(hipGetLastError());
    }
    const dim3 grid(wgs), block(szh_bm::WPG * 64);
    if (hasreg) {
        if (a.use_mean) hipLaunchKernelGGL((k_beam<T, DEC, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_beam<T, DEC, false, true>), grid, block, 0, st, a);
    } else {
        if (a.use_mean) hipLaunchKernelGGL((k_beam<T, DEC, true, false>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_beam<T, DEC, false, false>), grid, block, 0, st, a);
    }
    HIPCHK(hipGetLastError());
    return SZHIP_OK;
}

// One slice of the feed (see launch_beam): the decoded coefficients of the regression blocks with ranks [r_lo, r_hi) go to the device, are scattered to
// their blocks, the points of block rows [b0_lo, b0_hi) are quantised, and the sweep is told that planes < planes_end are complete.  All on `s2`.
template <class T>
int feed_beam_slice(szhip_ctx *ctx, const szh_geom3 &G, const szh_qargs<T> &a, hipStream_t s2, const T *hcoef, size_t reg_count, size_t r_lo, size_t r_hi,
                    int b0_lo, int b0_hi, int planes_end, const u64 *reg_rank, int64_t nb)
{
    if (r_hi > r_lo)
        for (int e = 0; e < 4; ++e)
            HIPCHK(hipMemcpyAsync((T *)ctx->coef_compact.p + (size_t)e * reg_count + r_lo, hcoef + (size_t)e * reg_count + r_lo, (r_hi - r_lo) * sizeof(T), hipMemcpyHostToDevice, s2));
    const int64_t blk_lo = (int64_t)b0_lo * G.g1.num * G.g2.num, blk_hi = std::min<int64_t>(nb, (int64_t)b0_hi * G.g1.num * G.g2.num);
    if (r_hi > r_lo && blk_hi > blk_lo) {
        // (over all blocks, 7 us: the ranks beyond r_hi scatter stale values that their own slice overwrites before anybody reads them)
        hipLaunchKernelGGL((k_move_coef<T, 1>), dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s2, a.blk_lor, reg_rank, nb, (int64_t)reg_count, (T *)a.coef, (T *)ctx->coef_compact.p);
        hipLaunchKernelGGL((k_reg_points<T, 0>), dim3((unsigned)((b0_hi - b0_lo) * G.g1.num)), dim3(256), 0, s2, G, a.blk_lor, a.coef, a.coef_stride, a.data, (T *)ctx->rb_vals.p,
                           a.codes, (uint8_t *)ctx->pt_flags.p, a.eb, a.recip, a.cap, a.radius, b0_lo);
    }
    hipLaunchKernelGGL(k_store_u32, dim3(1), dim3(1), 0, s2, (unsigned *)ctx->feed_word.p, (unsigned)planes_end);
    HIPCHK(hipGetLastError());
    return SZHIP_OK;
}

template <class T> double ord_dec(u64 e);
template <> double ord_dec<float>(u64 e)
{
    unsigned u = (unsigned)e;
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f; memcpy(&f, &u, 4); return (double)f;
}
template <> double ord_dec<double>(u64 e)
{
    u64 u = (e & 0x8000000000000000ull) ? (e & 0x7fffffffffffffffull) : ~e;
    double d; memcpy(&d, &u, 8); return d;
}

template <class T>
int minmax_impl(szhip_ctx *ctx, const void *data, int on_dev, size_t n, double *vmin, double *vmax)
{
    const T *d_in = (const T *)data;
    if (!on_dev) {
        TRY(ensure(ctx, ctx->in, n * sizeof(T)));
        HIPCHK(hipMemcpyAsync(ctx->in.p, data, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        d_in = (const T *)ctx->in.p;
    }
    TRY(ensure(ctx, ctx->small, SM_COUNT * 8));
    u64 *sm = (u64 *)ctx->small.p;
    u64 init[2] = {~0ull, 0ull};
    HIPCHK(hipMemcpyAsync(sm + SM_MINMAX, init, 16, hipMemcpyHostToDevice, ctx->stream));
    int grid = (int)std::min<int64_t>(((int64_t)n + 255) / 256, 2048);
    hipLaunchKernelGGL((k_minmax<T>), dim3(grid), dim3(256), 0, ctx->stream, d_in, (int64_t)n, sm + SM_MINMAX);
    HIPCHK(hipGetLastError());
    u64 res[2];
    HIPCHK(hipMemcpyAsync(res, sm + SM_MINMAX, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *vmin = ord_dec<T>(res[0]); *vmax = ord_dec<T>(res[1]);
    return SZHIP_OK;
}

