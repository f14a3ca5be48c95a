// szhip.hip -- C-ABI HIP layer (include/szhip.h): owns device buffers, launches the kernels of
// szhip_kernels.h in stream order and calls the short serial host pieces of szhost.c between them.
// gfx950 only; no CPU fallback: every entry point returns an error if the HIP runtime/device is missing.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <ctime>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include "../../include/szhip.h"
#include "szhost.h"
#include "szhip_kernels.h"
#include "szh_quality.h"
#include "szh_rangebatch.h"

namespace {

struct DevBuf { void *p = nullptr; size_t cap = 0; };

double now_ms()
{
    timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

} // namespace

// compress calls of this process that are inside the library right now, whatever their context: the chain / kernel overlap of an array with
// regression blocks is only taken by a call that starts alone (see compress_impl)
static std::atomic<int> g_compress_calls{0};
// (round 6) A sweep that is FED while the host's chains run (arrays with regression blocks, a call that starts alone) must not be joined half-way by another lone context's
// call: its slices' kernels then wait behind the other call's sweep, the fed sweep runs into its bounded waits, and the call is repeated -- streams stayed right in 20 000
// calls of two and four contexts on threads, but single calls took up to 5.7 s (profiles/r06_multi_context_stress_before_the_fed_call_guard.txt).  So: the fed call raises
// g_fed_active for its duration, and a compress call that starts meanwhile waits at its door (a few milliseconds at most); a call that meets another one inside the library
// notes the time, and for a while after such a meeting nobody feeds (several contexts at work overlap their calls anyway).  Sequentially consistent: either the fed call sees
// the newcomer's count (and does not feed), or the newcomer sees the flag (and waits).
static std::atomic<int> g_fed_active{0};
static std::atomic<long long> g_last_meeting_us{-(1ll << 60)};
static long long mono_us() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (long long)ts.tv_sec * 1000000ll + ts.tv_nsec / 1000; }
struct compress_call_guard {
    compress_call_guard()
    {
        if (g_compress_calls.fetch_add(1) > 0) g_last_meeting_us.store(mono_us());
        const long long t0 = mono_us();
        while (g_fed_active.load() != 0 && mono_us() - t0 < 200000) std::this_thread::yield();       // (bounded: 0.2 s, far beyond a fed call)
    }
    ~compress_call_guard() { g_compress_calls.fetch_sub(1); }
};
// the fed call's side: raise the flag, then look again whether the call is still alone
struct fed_call_guard {
    bool on = false;
    bool try_raise()
    {
        if (mono_us() - g_last_meeting_us.load() < 100000) return false;       // (another context was at work within the last 0.1 s)
        int expected = 0;
        if (!g_fed_active.compare_exchange_strong(expected, 1)) return false;
        if (g_compress_calls.load() > 1) { g_fed_active.store(0); return false; }
        on = true;
        return true;
    }
    ~fed_call_guard() { if (on) g_fed_active.store(0); }
};
// The host's coefficient chains (szhost_coeff_chain_one_p: one serial chain per coefficient) on PERSISTENT threads (round 5).  Threads created per
// call started 0.1 ms late on cores that had been idle (measured on the GPU box: four chains of 1.0 - 1.2 ms each took 2.1 - 2.7 ms end to
// end, and 4.9 on some runs).  A context that has met regression blocks once keeps four workers; they are woken when a compression STARTS and
// spin -- on cores that are awake by then -- until the fit pass has delivered the coefficients (~0.4 ms), or are sent back to sleep if the array
// has no regression block.  A job has two stages: the chain (the caller waits for it: the sweep needs the decoded coefficients), then the
// coefficient's section of the stream header (collected where the header is assembled).
struct szhip_chain_pool {
    std::thread th[4];
    std::mutex m; std::condition_variable cv;
    std::atomic<int> phase{0};                    // 0 asleep, 1 awake (spinning for a job), 2 quit
    std::atomic<uint64_t> seq{0};
    std::atomic<int> stage1{0}, stage2{0};
    int n = 0;
    std::function<void(int)> chain, section;
    static void pause() {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    void run(int e)
    {
        uint64_t seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return phase.load() != 0; }); }
            if (phase.load() == 2) return;
            while (phase.load(std::memory_order_acquire) == 1 && seq.load(std::memory_order_acquire) == seen) pause();
            const uint64_t s = seq.load(std::memory_order_acquire);
            if (s != seen) {
                seen = s;
                if (e < n) { chain(e); stage1.fetch_add(1, std::memory_order_release); section(e); }
                stage2.fetch_add(1, std::memory_order_release);
            }
        }
    }
    void start() { for (int e = 0; e < 4; ++e) th[e] = std::thread([this, e] { run(e); }); }
    void arm() { { std::lock_guard<std::mutex> lk(m); if (phase.load() == 0) phase.store(1); } cv.notify_all(); }
    void disarm() { std::lock_guard<std::mutex> lk(m); if (phase.load() == 1) phase.store(0); }
    void submit(int ncoef, std::function<void(int)> c, std::function<void(int)> sec)
    {
        n = ncoef; chain = std::move(c); section = std::move(sec);
        stage1.store(0); stage2.store(0);
        arm();
        seq.fetch_add(1, std::memory_order_release);
    }
    void wait_chains() { while (stage1.load(std::memory_order_acquire) < n) pause(); }
    void wait_all() { while (stage2.load(std::memory_order_acquire) < 4) std::this_thread::yield(); }
    ~szhip_chain_pool()
    {
        { std::lock_guard<std::mutex> lk(m); phase.store(2); }
        cv.notify_all();
        for (auto &t : th) if (t.joinable()) t.join();
    }
};

constexpr int SZH_STAGE_T = 4;                   // host threads of a staged copy (staged_copy)
struct szhip_ctx {
    int device = 0;
    int cus = 256;                               // compute units of `device` (hipDeviceAttributeMultiprocessorCount): persistent kernels launch one workgroup per CU at most
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // the fit + selection pass runs here, concurrently with the interval optimiser's sampling and host decisions
    hipEvent_t ev_in = nullptr, ev_fit = nullptr, ev_feed = nullptr, ev_sec = nullptr;
    int settle_probes = 0, settle_rejected = 0;   // settle_streams: queue probes made, streams replaced
    hipStream_t stream3 = nullptr;   // the block-ordering pass of finished tile rows, while the sweep is still running on `stream` (created on first use)
    hipEvent_t ev_perm = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    char err[512] = {0};
    unsigned epoch = 0;
    // Huffman decode: two rounds without asking the device in between (checked with the caller's next synchronisation); a call whose
    // start guesses were still moving after them is repeated once with a synchronisation per round (with_ticket_fallback)
    bool hdec_sync_rounds = false, hdec_unconverged = false;
    // a lane of a pool (several arrays in flight, szhip_pool); false for a lone context.  (The lanes' sweeps share the CUs: taking turns
    // measured slower at 512^3 with two lanes over 60 steps, 294 - 303 GB/s against 305 - 319.)
    bool gate = false;
    unsigned long long *hdec_res = nullptr;      // pinned: {symbols the payload holds, starts still moving after round 1}, copied asynchronously
    // workspaces (grow-only)
    DevBuf lor_bits, reg_flags, reg_rank, coef_compact, in, out, codes_nat, codes_blk, coef, blk_lor, faceI, faceJ, rb_down, rb_right, rb_vals, pt_flags, feed_word, progress, order, small, hist, col_zeros, col_zeros64,
        seg_bits, seg_zeros, seg_bitoff, seg_zoff, seg_hist, seg_tab, col_off, partial, samples, unpred, stream_buf, chunk_bits, chunk_off, code_tab, len_tab, dec_tab,
        starts, ends, counts, offs, dirty, zcnt, zpos, pwr_log, pwr_signs, pwr_small, coef_dec, msst_ptab, msst_cells, msst_rec, msst_pe, book_tree, book_rec, book_stage,
        batch_rec, batch_blob,               // szhip_*_omp_batch: the per-array table; the blob of streams (the single calls inside a batch use stream_buf)
        in2, quality;                        // szhip_compare: the second host array of the pair; the workgroups' partial results
    void *pinned = nullptr; size_t pinned_cap = 0;
    void *pinned2 = nullptr; size_t pinned2_cap = 0;   // target of the second stream's copies (indicator bits, regression-block count)
    // bulk copies between the caller's pageable arrays and the device: SZH_STAGE_T host threads, two pinned buffers + events each
    void *stage_buf[SZH_STAGE_T][2] = {};
    hipEvent_t stage_ev[SZH_STAGE_T][2] = {};
    void *pinned3 = nullptr; size_t pinned3_cap = 0;
    int streams_independent = -1;                      // -1 not probed yet; 1: work on stream2 proceeds while a kernel on stream is running
    void *coh = nullptr; size_t coh_cap = 0;           // host-coherent (uncached on the GPU) pinned memory the wavefront kernel reads while the host writes   // the regression coefficients on their way to the host chain and back
    int order_nI = -1, order_nJ = -1;
    // tile tickets: by default a workgroup's index is its ticket (SZ_HIP_TICKET_MODE=2), which assumes that the workgroups of one XCD start in index
    // order AND that every XCD gets to run; if a wavefront-kernel wait ever times out the call is repeated once with the atomic ticket, which
    // assumes neither (a GPU shared with other work), and the context keeps that mode
    bool wave_timeout = false, ticket_atomic = false;
    // the coefficient chain beside the running sweep (M-field): a sweep that gave up waiting for the coefficients (seen 5 - 6 times in 480 rounds with
    // several arrays in flight) is answered by ONE repetition with the chain finished before the sweep starts; the context keeps that order
    bool coef_late = false, no_chain_overlap = false;
    // the code book built on the device (SZ_HIP_DEV_BOOK=1, szh_book.h): a call whose book the kernel declined (more distinct symbols than its heap holds, a code
    // word beyond 32 bits, a stream that outgrows the buffers sized before the call) is repeated once with the host's book
    bool book_declined = false, no_dev_book = false;
    unsigned long long *book_pin = nullptr;      // pinned: the book's record and the plan behind it, copied asynchronously, read after the call's final synchronisation
    std::vector<int> chain_codes; std::vector<unsigned char> chain_unpred;   // the chains' outputs, kept across calls (fresh memory page-faults under the chain: ~1 ms for the M-field's 10 MB)
    unsigned char *sec_pin[4] = {nullptr, nullptr, nullptr, nullptr}; size_t sec_pin_cap[4] = {0, 0, 0, 0};   // the coefficient sections of the stream header as the chain threads build them: pinned, they go to the device from where they are
    szhip_chain_pool *chain_pool = nullptr;      // the coefficient chains' persistent threads (created with the first array that has regression blocks)
};

namespace {

// The host side of every path, one file per path (all inside this anonymous namespace, one translation unit: the kernels' templates are
// instantiated once):
#include "szhip_rt.inc"      // buffers, streams, staging copies, launchers of the sweep kernels
#include "szhip_steps.inc"   // the steps of a call that the paths below share
#include "szhip_sz21.inc"    // SZ 2.1: the hot path (SZ_compress_args / SZ_decompress of float and double arrays)
#include "szhip_sz14.inc"    // SZ 1.4 container, MSST19
#include "szhip_pwr.inc"     // point-wise relative bounds
#include "szhip_omprules.inc" // the OpenMP container's rules, once, for the three files below
#include "szhip_omp.inc"     // the reference's OpenMP container
#include "szhip_ompbatch.inc" // ... over many same-shape arrays in one call
#include "szhip_ompregion.inc" // ... sub-boxes of many streams in one call
#include "szhip_rangebatch.inc" // the value range of many arrays in one launch
#include "szhip_quality.inc" // an array against its decoded copy: the error report, for one pair and for many

} // namespace

// no work of the context is in flight behind this
static void drain(szhip_ctx *ctx)
{
    if (ctx->stream3) hipStreamSynchronize(ctx->stream3);
    hipStreamSynchronize(ctx->stream2);
    hipStreamSynchronize(ctx->stream);
}
// (an early exit must not leave work in flight)
static int drained_on_failure(szhip_ctx *ctx, int rc) { if (rc != SZHIP_OK) drain(ctx); return rc; }
// (the same for the paths that use the first stream only)
static int synced_on_failure(szhip_ctx *ctx, int rc) { if (rc != SZHIP_OK) hipStreamSynchronize(ctx->stream); return rc; }

// runs one call; a wavefront-kernel wait that timed out under the index ticket is answered by ONE repetition with the atomic ticket (see szhip_ctx)
template <class F>
static int with_ticket_fallback(szhip_ctx *ctx, F &&run)
{
    ctx->wave_timeout = false; ctx->hdec_unconverged = false; ctx->coef_late = false; ctx->book_declined = false;
    auto again = [&]() { drain(ctx); return run(); };
    int rc = run();
    if (rc == SZHIP_ERR_INTERNAL && ctx->book_declined && !ctx->no_dev_book) {            // (compression with SZ_HIP_DEV_BOOK=1 only)
        ctx->no_dev_book = true; ctx->wave_timeout = false; rc = again(); ctx->no_dev_book = false;
    }
    if (rc == SZHIP_OK && !ctx->no_chain_overlap && tune_int("SZ_HIP_TEST_CHAIN_FALLBACK", 0)) { ctx->coef_late = true; rc = SZHIP_ERR_INTERNAL; }   // tests: exercise the repetition
    if (rc == SZHIP_ERR_INTERNAL && ctx->coef_late && !ctx->no_chain_overlap) {           // (compression of arrays with regression blocks only)
        ctx->no_chain_overlap = true; ctx->wave_timeout = false; rc = again();
    }
    if (rc == SZHIP_ERR_INTERNAL && ctx->hdec_unconverged && !ctx->hdec_sync_rounds) {      // (decompression only)
        ctx->hdec_sync_rounds = true; ctx->wave_timeout = false; rc = again(); ctx->hdec_sync_rounds = false;
    }
    if (rc == SZHIP_OK && !ctx->ticket_atomic && tune_int("SZ_HIP_TEST_TICKET_FALLBACK", 0)) { ctx->wave_timeout = true; rc = SZHIP_ERR_INTERNAL; }   // tests: exercise the repetition
    if (rc == SZHIP_ERR_INTERNAL && ctx->wave_timeout && !ctx->ticket_atomic) {
        ctx->ticket_atomic = true; rc = again();
    }
    return rc;
}

// a compress call under compress_call_guard: a failed first attempt clears *out and *out_size, so a repetition starts from the caller's values
template <class F>
static int guarded_compress(szhip_ctx *ctx, unsigned char **out, size_t *out_size, F &&run)
{
    const compress_call_guard in_flight;
    unsigned char *const out0 = *out; const size_t cap0 = *out_size;
    return drained_on_failure(ctx, with_ticket_fallback(ctx, [&]() { *out = out0; *out_size = cap0; return run(); }));
}

// the extents an entry point takes: a 3-D array, or (r0 == 0) a 2-D one ...
static bool dims_3d_2d(size_t r0, size_t r1, size_t r2)
{
    return !((r0 != 0 && r0 < 2) || r1 < 2 || r2 < 2 || r0 > 0x7fffffff || r1 > 0x7fffffff || r2 > 0x7fffffff);
}
// ... or (r0 == 0 and r1 == 0) a 1-D one
static bool dims_3d_2d_1d(size_t r0, size_t r1, size_t r2)
{
    return !((r0 != 0 && r0 < 2) || (r1 < 2 && !(r0 == 0 && r1 == 0)) || r2 < 2 || r0 > 0x7fffffff || r1 > 0x7fffffff || r2 > 0x7fffffff);
}

extern "C" {


// Every stream of a context has the default priority (which streams share a hardware queue is settled by settle_streams instead; streams
// of different priorities were tried for that, round 4).
static int create_ctx(szhip_ctx **out, int device)
{
    if (!out) return SZHIP_ERR_ARG;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        fprintf(stderr, "szhip: no HIP device available (%s); this library has no CPU fallback\n", hipGetErrorString(e));
        return SZHIP_ERR_NODEVICE;
    }
    if (device < 0 || device >= count) return SZHIP_ERR_ARG;
    szhip_ctx *ctx = new szhip_ctx();
    ctx->device = device;
    { int c = 0; if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && c > 0) ctx->cus = c; }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx; return SZHIP_ERR_NODEVICE;
    }
    for (int i = 0; i < 6; ++i) if (hipEventCreate(&ctx->ev[i]) != hipSuccess) { delete ctx; return SZHIP_ERR_NODEVICE; }
    if (hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fit, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_feed, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_sec, hipEventDisableTiming) != hipSuccess) { delete ctx; return SZHIP_ERR_NODEVICE; }
    *out = ctx;
    return SZHIP_OK;
}

int szhip_create(szhip_ctx **out, int device)
{
    const int rc = create_ctx(out, device);
    if (rc == SZHIP_OK) settle_streams(*out, nullptr, 0);
    return rc;
}

void szhip_destroy(szhip_ctx *ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    delete ctx->chain_pool; ctx->chain_pool = nullptr;
    DevBuf *bufs[] = {&ctx->lor_bits, &ctx->reg_flags, &ctx->reg_rank, &ctx->coef_compact, &ctx->in, &ctx->out, &ctx->codes_nat, &ctx->codes_blk, &ctx->coef, &ctx->blk_lor, &ctx->faceI, &ctx->faceJ, &ctx->rb_down, &ctx->rb_right, &ctx->rb_vals, &ctx->pt_flags, &ctx->feed_word, &ctx->progress,
                      &ctx->order, &ctx->small, &ctx->hist, &ctx->col_zeros, &ctx->col_zeros64, &ctx->seg_bits, &ctx->seg_zeros, &ctx->seg_bitoff, &ctx->seg_zoff, &ctx->seg_hist, &ctx->seg_tab, &ctx->col_off, &ctx->partial,
                      &ctx->samples, &ctx->unpred, &ctx->stream_buf, &ctx->chunk_bits, &ctx->chunk_off, &ctx->code_tab,
                      &ctx->len_tab, &ctx->dec_tab, &ctx->starts, &ctx->ends, &ctx->counts, &ctx->offs, &ctx->dirty, &ctx->zcnt, &ctx->zpos,
                      &ctx->pwr_log, &ctx->pwr_signs, &ctx->pwr_small, &ctx->coef_dec, &ctx->msst_ptab, &ctx->msst_cells, &ctx->msst_rec, &ctx->msst_pe, &ctx->book_tree, &ctx->book_rec, &ctx->book_stage, &ctx->batch_rec, &ctx->batch_blob, &ctx->in2, &ctx->quality};
    for (DevBuf *b : bufs) if (b->p) hipFree(b->p);
    if (ctx->pinned) hipHostFree(ctx->pinned);
    if (ctx->pinned2) hipHostFree(ctx->pinned2);
    if (ctx->pinned3) hipHostFree(ctx->pinned3);
    if (ctx->coh) hipHostFree(ctx->coh);
    if (ctx->hdec_res) hipHostFree(ctx->hdec_res);
    if (ctx->book_pin) hipHostFree(ctx->book_pin);
    for (int w = 0; w < SZH_STAGE_T; ++w) for (int k = 0; k < 2; ++k) { if (ctx->stage_buf[w][k]) hipHostFree(ctx->stage_buf[w][k]); if (ctx->stage_ev[w][k]) hipEventDestroy(ctx->stage_ev[w][k]); }
    for (int i = 0; i < 6; ++i) if (ctx->ev[i]) hipEventDestroy(ctx->ev[i]);
    if (ctx->ev_in) hipEventDestroy(ctx->ev_in);
    if (ctx->ev_fit) hipEventDestroy(ctx->ev_fit);
    if (ctx->ev_feed) hipEventDestroy(ctx->ev_feed);
    if (ctx->ev_sec) hipEventDestroy(ctx->ev_sec);
    for (int e = 0; e < 4; ++e) if (ctx->sec_pin[e]) hipHostFree(ctx->sec_pin[e]);
    if (ctx->stream2) hipStreamDestroy(ctx->stream2);
    if (ctx->stream3) hipStreamDestroy(ctx->stream3);
    if (ctx->ev_perm) hipEventDestroy(ctx->ev_perm);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *szhip_last_error(szhip_ctx *ctx) { return ctx ? ctx->err : "no context"; }

// ---- several arrays in flight (szhip.h): `lanes` contexts, one host thread each, one queue
struct szhip_pool_job {
    int dtype; const void *data; int on_dev; size_t r0, r1, r2; double eb; szhip_params prm; const unsigned char *meta; size_t meta_len;
    int out_on_device; unsigned char *out; size_t out_size; szhip_stats stats; int rc; bool done;
};
struct szhip_pool {
    std::vector<szhip_ctx *> ctx;
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::deque<int> queue;                      // tickets waiting for a lane
    std::vector<szhip_pool_job> jobs;           // ring of tickets
    std::vector<bool> used;
    bool stop = false;
};
static void szhip_pool_worker(szhip_pool *p, int lane)
{
    for (;;) {
        int t;
        {
            std::unique_lock<std::mutex> lk(p->mu);
            p->cv_work.wait(lk, [&] { return p->stop || !p->queue.empty(); });
            if (p->queue.empty()) return;
            t = p->queue.front(); p->queue.pop_front();
        }
        szhip_pool_job &j = p->jobs[t];
        j.rc = szhip_compress(p->ctx[lane], j.dtype, j.data, j.on_dev, j.r0, j.r1, j.r2, j.eb, &j.prm, j.meta, j.meta_len, j.out_on_device,
                              &j.out, &j.out_size, &j.stats);
        { std::lock_guard<std::mutex> lk(p->mu); j.done = true; }
        p->cv_done.notify_all();
    }
}
int szhip_pool_create(szhip_pool **out, int device, int lanes)
{
    if (!out || lanes < 1 || lanes > 16) return SZHIP_ERR_ARG;
    szhip_pool *p = new szhip_pool();
    for (int i = 0; i < lanes; ++i) {
        szhip_ctx *c = nullptr;
        const int rc = create_ctx(&c, device);
        if (rc != SZHIP_OK) { for (szhip_ctx *x : p->ctx) szhip_destroy(x); delete p; return rc; }
        c->gate = lanes > 1;
        // (against the earlier lanes' main AND second streams: a lane's fit pass behind another lane's sweep is as bad as two sweeps in a row)
        { std::vector<hipStream_t> mains; for (szhip_ctx *x : p->ctx) { mains.push_back(x->stream); mains.push_back(x->stream2); } settle_streams(c, mains.data(), (int)mains.size(), lanes == 1); }
        p->ctx.push_back(c);
    }
    p->jobs.resize(64); p->used.assign(64, false);
    for (int i = 0; i < lanes; ++i) p->workers.emplace_back(szhip_pool_worker, p, i);
    *out = p;
    return SZHIP_OK;
}
void szhip_pool_destroy(szhip_pool *p)
{
    if (!p) return;
    { std::lock_guard<std::mutex> lk(p->mu); p->stop = true; }
    p->cv_work.notify_all();
    for (auto &w : p->workers) if (w.joinable()) w.join();
    for (szhip_ctx *c : p->ctx) szhip_destroy(c);
    delete p;
}
int szhip_pool_submit(szhip_pool *p, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, double eb,
                      const szhip_params *params, const unsigned char *meta, size_t meta_len, int out_on_device,
                      unsigned char *out_buf, size_t out_cap, int *ticket)
{
    if (!p || !data || !params || !meta || !ticket) return SZHIP_ERR_ARG;
    std::lock_guard<std::mutex> lk(p->mu);
    int t = -1;
    for (size_t i = 0; i < p->used.size(); ++i) if (!p->used[i]) { t = (int)i; break; }
    if (t < 0) return SZHIP_ERR_ARG;                         // 64 calls waiting to be collected: wait for some first
    szhip_pool_job &j = p->jobs[t];
    j = szhip_pool_job();
    j.dtype = dtype; j.data = data; j.on_dev = data_on_device; j.r0 = r0; j.r1 = r1; j.r2 = r2; j.eb = eb; j.prm = *params;
    j.meta = meta; j.meta_len = meta_len; j.out_on_device = out_on_device; j.out = out_on_device == 2 ? out_buf : nullptr;
    j.out_size = out_on_device == 2 ? out_cap : 0; j.rc = SZHIP_ERR_INTERNAL; j.done = false;
    p->used[t] = true;
    p->queue.push_back(t);
    *ticket = t;
    p->cv_work.notify_one();
    return SZHIP_OK;
}
int szhip_pool_wait(szhip_pool *p, int ticket, unsigned char **out, size_t *out_size, szhip_stats *stats)
{
    if (!p || ticket < 0 || ticket >= (int)p->jobs.size()) return SZHIP_ERR_ARG;
    std::unique_lock<std::mutex> lk(p->mu);
    if (!p->used[ticket]) return SZHIP_ERR_ARG;
    p->cv_done.wait(lk, [&] { return p->jobs[ticket].done; });
    szhip_pool_job &j = p->jobs[ticket];
    if (out) *out = j.out;
    if (out_size) *out_size = j.out_size;
    if (stats) *stats = j.stats;
    p->used[ticket] = false;
    return j.rc;
}


int szhip_stage_input(szhip_ctx *ctx, const void *host_data, size_t bytes, void **device_ptr)
{
    if (!ctx || !host_data || !device_ptr) return SZHIP_ERR_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    TRY(ensure(ctx, ctx->in, bytes));
    TRY(staged_copy(ctx, ctx->in.p, host_data, bytes, true));
    *device_ptr = ctx->in.p;
    return SZHIP_OK;
}

int szhip_stage_input_batch(szhip_ctx *ctx, const void *const *host_data, int count, size_t bytes, const void **device_ptrs)
{
    if (!ctx || !host_data || !device_ptrs || count < 1 || bytes == 0) return SZHIP_ERR_ARG;
    for (int i = 0; i < count; ++i) if (!host_data[i]) return SZHIP_ERR_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    std::vector<const void *> d;
    TRY(synced_on_failure(ctx, batch_stage(ctx, ctx->in, count, bytes, ctx->stream, [&](int i) { return host_data[i]; }, d)));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return SZHIP_ERR_NODEVICE;
    for (int i = 0; i < count; ++i) device_ptrs[i] = d[i];
    return SZHIP_OK;
}
int szhip_stage_input_batch_lens(szhip_ctx *ctx, const void *const *host_data, int count, const size_t *bytes, const void **device_ptrs)
{
    if (!ctx || !host_data || !device_ptrs || !bytes || count < 1) return SZHIP_ERR_ARG;
    for (int i = 0; i < count; ++i) if (!host_data[i] || bytes[i] == 0) return SZHIP_ERR_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    std::vector<const void *> d;
    TRY(synced_on_failure(ctx, batch_stage(ctx, ctx->in, count, 0, ctx->stream, [&](int i) { return host_data[i]; }, d, nullptr, bytes)));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return SZHIP_ERR_NODEVICE;
    for (int i = 0; i < count; ++i) device_ptrs[i] = d[i];
    return SZHIP_OK;
}

// include/szhip.h, "Device pointers and ordering": a pointer to VALUES (`data`, `out` of a decompress call) is aligned to its element, on the host or on the device;
// refused here, before anything is launched; then the context's device is made current.  Byte pointers (streams, parameter bytes, a caller's stream buffer) take any alignment.
static int check_alignment_set_device(szhip_ctx *ctx, int dtype, const void *p)
{
    if (((uintptr_t)p & (dtype == SZHIP_F32 ? 3u : 7u)) != 0) {
        snprintf(ctx->err, sizeof(ctx->err), "pointer %p is not aligned to its %d-byte elements", p, dtype == SZHIP_F32 ? 4 : 8);
        return SZHIP_ERR_ARG;
    }
    return hipSetDevice(ctx->device) != hipSuccess ? SZHIP_ERR_NODEVICE : SZHIP_OK;
}
// the float or the double instance of a path's host code
#define BY_DTYPE(dtype, fn, ...) ((dtype) == SZHIP_F32 ? fn<float>(__VA_ARGS__) : fn<double>(__VA_ARGS__))

int szhip_minmax(szhip_ctx *ctx, int dtype, const void *data, int on_dev, size_t n, double *vmin, double *vmax)
{
    if (!ctx || !data || !n || !vmin || !vmax) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, data));
    return BY_DTYPE(dtype, minmax_impl, ctx, data, on_dev, n, vmin, vmax);
}

// the refusals of the batch calls over arrays of n values, before anything is launched: SZHIP_ERR_ARG
static int batch_pointers(szhip_ctx *ctx, int dtype, const void *const *p, int count, size_t n)
{
    if (!ctx || !p || count < 1 || n == 0 || (dtype != SZHIP_F32 && dtype != SZHIP_F64)) return SZHIP_ERR_ARG;
    for (int i = 0; i < count; ++i) {
        if (!p[i]) { snprintf(ctx->err, sizeof(ctx->err), "array %d of the batch: a null pointer", i); return SZHIP_ERR_ARG; }
        if (((uintptr_t)p[i] & (dtype == SZHIP_F32 ? 3u : 7u)) != 0) {
            snprintf(ctx->err, sizeof(ctx->err), "array %d of the batch: pointer %p is not aligned to its %d-byte elements", i, p[i], dtype == SZHIP_F32 ? 4 : 8);
            return SZHIP_ERR_ARG;
        }
    }
    return SZHIP_OK;
}

int szhip_minmax_batch(szhip_ctx *ctx, int dtype, const void *const *data, int count, int data_on_device, size_t n, double *vmin, double *vmax, szhip_stats *stats)
{
    if (!vmin || !vmax) return SZHIP_ERR_ARG;
    TRY(batch_pointers(ctx, dtype, data, count, n));
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    return synced_on_failure(ctx, BY_DTYPE(dtype, minmax_batch_impl, ctx, data, count, data_on_device, 1, 1, n, n, n, nullptr, vmin, vmax, stats));
}
static int check_view(szhip_ctx *ctx, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1);
int szhip_minmax_batch_view(szhip_ctx *ctx, int dtype, const void *const *data, int count, int data_on_device, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1,
                            double *vmin, double *vmax, szhip_stats *stats)
{
    if (!vmin || !vmax) return SZHIP_ERR_ARG;
    if (r0 < 1 || r1 < 1 || r2 < 1 || r0 > 0x7fffffff || r1 > 0x7fffffff || r2 > 0x7fffffff) return SZHIP_ERR_ARG;
    TRY(batch_pointers(ctx, dtype, data, count, 1));
    TRY(check_view(ctx, r0, r1, r2, pitch0, pitch1));
    if ((double)r0 * (double)r1 * (double)r2 >= 4294967296.0) { snprintf(ctx->err, sizeof(ctx->err), "szhip_minmax_batch_view: sub-boxes of 2^32 values or more"); return SZHIP_ERR_UNSUP; }
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    if (pitch1 == r2 && pitch0 == r1 * r2) { const size_t n = r0 * r1 * r2; r0 = r1 = 1; r2 = pitch0 = pitch1 = n; }      // (the contiguous call, exactly)
    return synced_on_failure(ctx, BY_DTYPE(dtype, minmax_batch_impl, ctx, data, count, data_on_device, r0, r1, r2, pitch0, pitch1, nullptr, vmin, vmax, stats));
}

int szhip_compress(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, double eb,
                   const szhip_params *params, const unsigned char *meta, size_t meta_len, int out_on_device,
                   unsigned char **out, size_t *out_size, szhip_stats *stats)
{
    if (!ctx || !data || !params || !meta || !out || !out_size) return SZHIP_ERR_ARG;
    if (!dims_3d_2d(r0, r1, r2)) return SZHIP_ERR_ARG;
    if (!(eb > 0)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, data));
    return guarded_compress(ctx, out, out_size, [&]() {
               return BY_DTYPE(dtype, compress_impl, ctx, data, data_on_device, r0, r1, r2, eb, params, meta, meta_len, out_on_device, out, out_size, stats); });
}

int szhip_compress_sz14(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, double eb,
                        double value_range, double median, const szhip_params *params, const unsigned char *meta, size_t meta_len,
                        int out_on_device, unsigned char **out, size_t *out_size, szhip_stats *stats)
{
    if (!ctx || !data || !params || !meta || !out || !out_size) return SZHIP_ERR_ARG;
    if (!dims_3d_2d_1d(r0, r1, r2)) return SZHIP_ERR_ARG;
    if (!(eb > 0)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, data));
    return guarded_compress(ctx, out, out_size, [&]() {
               return BY_DTYPE(dtype, compress14_impl, ctx, data, data_on_device, r0, r1, r2, eb, value_range, median, params, meta, meta_len, nullptr, out_on_device, out, out_size, stats); });
}

int szhip_decompress_sz14(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len, size_t body_off,
                          size_t r0, size_t r1, size_t r2, void *out, int out_on_device, szhip_stats *stats)
{
    if (!ctx || !stream || !out || body_off >= stream_len) return SZHIP_ERR_ARG;
    if (!dims_3d_2d_1d(r0, r1, r2)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, out));
    return drained_on_failure(ctx, with_ticket_fallback(ctx, [&]() {
               return BY_DTYPE(dtype, decompress14_impl, ctx, stream, stream_on_device, stream_len, body_off, 0, r0, r1, r2, out, out_on_device, stats); }));
}

int szhip_compress_omp(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, double eb, int thread_num,
                       const szhip_params *params, const unsigned char *meta, size_t meta_len, int out_on_device, unsigned char **out, size_t *out_size,
                       szhip_stats *stats)
{
    if (!ctx || !data || !params || !meta || !out || !out_size) return SZHIP_ERR_ARG;
    if (r0 < 1 || r1 < 1 || r2 < 1 || r0 > 0x7fffffff || r1 > 0x7fffffff || r2 > 0x7fffffff || thread_num < 1) return SZHIP_ERR_ARG;
    if (!(eb > 0)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, data));
    return synced_on_failure(ctx,
               BY_DTYPE(dtype, compress_omp_impl, ctx, data, data_on_device, r0, r1, r2, r1 * r2, r2, eb, thread_num, params, meta, meta_len, out_on_device, out, out_size, stats));
}

int szhip_decompress_omp(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len, size_t body_off,
                         size_t r0, size_t r1, size_t r2, void *out, int out_on_device, szhip_stats *stats)
{
    if (!ctx || !stream || !out || body_off >= stream_len) return SZHIP_ERR_ARG;
    if (r0 < 1 || r1 < 1 || r2 < 1 || r0 > 0x7fffffff || r1 > 0x7fffffff || r2 > 0x7fffffff) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, out));
    return synced_on_failure(ctx,
               BY_DTYPE(dtype, decompress_omp_impl, ctx, stream, stream_on_device, stream_len, body_off, r0, r1, r2, out, out_on_device, 0, 0, stats));
}

// the refusals of a batch call, before anything is launched or written: SZHIP_ERR_ARG
static int batch_args(szhip_ctx *ctx, int dtype, const szhip_batch_item *items, int count, size_t r0, size_t r1, size_t r2, bool compress)
{
    if (!ctx || !items || count < 1 || (dtype != SZHIP_F32 && dtype != SZHIP_F64)) return SZHIP_ERR_ARG;
    if (r0 < 1 || r1 < 1 || r2 < 1 || r0 > 0x7fffffff || r1 > 0x7fffffff || r2 > 0x7fffffff) return SZHIP_ERR_ARG;
    for (int i = 0; i < count; ++i) {
        const szhip_batch_item &it = items[i];
        const void *values = compress ? it.data : (const void *)it.out;
        if (!values || (compress ? !it.meta || !(it.eb > 0) || !((dtype == SZHIP_F32 ? (double)(float)it.eb : it.eb) > 0) : !it.stream || it.body_off >= it.stream_len)) {
            snprintf(ctx->err, sizeof(ctx->err), "item %d of the batch: a null pointer, a bound that is not positive or an empty stream", i);
            return SZHIP_ERR_ARG;
        }
        if (((uintptr_t)values & (dtype == SZHIP_F32 ? 3u : 7u)) != 0) {
            snprintf(ctx->err, sizeof(ctx->err), "item %d of the batch: pointer %p is not aligned to its %d-byte elements", i, values, dtype == SZHIP_F32 ? 4 : 8);
            return SZHIP_ERR_ARG;
        }
    }
    return SZHIP_OK;
}

// (the contiguous call: pitch0 = r1 * r2, pitch1 = r2)
static int compress_omp_batch_entry(szhip_ctx *ctx, int dtype, szhip_batch_item *items, int count, int data_on_device, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1,
                                    int thread_num, const szhip_params *params, size_t meta_len, int out_on_device, unsigned char **blob, size_t *blob_size, szhip_stats *stats)
{
    if (!params || !blob || !blob_size || thread_num < 1) return SZHIP_ERR_ARG;
    TRY(batch_args(ctx, dtype, items, count, r0, r1, r2, true));
    TRY(check_view(ctx, r0, r1, r2, pitch0, pitch1));
    if (out_on_device != 0 && out_on_device != 1) { snprintf(ctx->err, sizeof(ctx->err), "a batch writes into a host blob (0) or the context's device blob (1)"); return SZHIP_ERR_UNSUP; }
    if (data_on_device && (pitch1 != r2 || pitch0 != r1 * r2) && ctx->in.p)      // device views: the gather's copies go into the context's input buffer
        for (int i = 0; i < count; ++i)
            if ((const char *)items[i].data >= (const char *)ctx->in.p && (const char *)items[i].data < (const char *)ctx->in.p + ctx->in.cap) {
                snprintf(ctx->err, sizeof(ctx->err), "item %d of the batch: a device view inside the context's input buffer (szhip_stage_input), which the call itself uses", i);
                return SZHIP_ERR_ARG;
            }
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    for (int i = 0; i < count; ++i) { items[i].offset = items[i].size = 0; items[i].rc = SZHIP_OK; items[i].intervals = 0; items[i].n_unpred = 0; items[i].quant_kernel = 0; items[i].batched = 0; }
    *blob = nullptr; *blob_size = 0;
    return synced_on_failure(ctx, BY_DTYPE(dtype, compress_omp_batch_impl, ctx, items, count, data_on_device, nullptr, r0, r1, r2, pitch0, pitch1, thread_num, params, meta_len, out_on_device,
                                           blob, blob_size, stats));
}
static int decompress_omp_batch_entry(szhip_ctx *ctx, int dtype, szhip_batch_item *items, int count, int stream_on_device, size_t r0, size_t r1, size_t r2,
                                      int out_on_device, size_t pitch0, size_t pitch1, szhip_stats *stats)
{
    TRY(batch_args(ctx, dtype, items, count, r0, r1, r2, false));
    TRY(check_view(ctx, r0, r1, r2, pitch0, pitch1));
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    for (int i = 0; i < count; ++i) { items[i].rc = SZHIP_OK; items[i].intervals = 0; items[i].n_unpred = 0; items[i].quant_kernel = 0; items[i].batched = 0; }
    return synced_on_failure(ctx, BY_DTYPE(dtype, decompress_omp_batch_impl, ctx, items, count, stream_on_device, nullptr, r0, r1, r2, out_on_device, pitch0, pitch1, stats));
}

int szhip_compress_omp_batch(szhip_ctx *ctx, int dtype, szhip_batch_item *items, int count, int data_on_device, size_t r0, size_t r1, size_t r2, int thread_num,
                             const szhip_params *params, size_t meta_len, int out_on_device, unsigned char **blob, size_t *blob_size, szhip_stats *stats)
{
    return compress_omp_batch_entry(ctx, dtype, items, count, data_on_device, r0, r1, r2, r1 * r2, r2, thread_num, params, meta_len, out_on_device, blob, blob_size, stats);
}
int szhip_compress_omp_batch_view(szhip_ctx *ctx, int dtype, szhip_batch_item *items, int count, int data_on_device, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1,
                                  int thread_num, const szhip_params *params, size_t meta_len, int out_on_device, unsigned char **blob, size_t *blob_size, szhip_stats *stats)
{
    return compress_omp_batch_entry(ctx, dtype, items, count, data_on_device, r0, r1, r2, pitch0, pitch1, thread_num, params, meta_len, out_on_device, blob, blob_size, stats);
}

int szhip_decompress_omp_batch(szhip_ctx *ctx, int dtype, szhip_batch_item *items, int count, int stream_on_device, size_t r0, size_t r1, size_t r2,
                               int out_on_device, szhip_stats *stats)
{
    return decompress_omp_batch_entry(ctx, dtype, items, count, stream_on_device, r0, r1, r2, out_on_device, r1 * r2, r2, stats);
}
int szhip_decompress_omp_batch_view(szhip_ctx *ctx, int dtype, szhip_batch_item *items, int count, int stream_on_device, size_t r0, size_t r1, size_t r2,
                                    int out_on_device, size_t pitch0, size_t pitch1, szhip_stats *stats)
{
    return decompress_omp_batch_entry(ctx, dtype, items, count, stream_on_device, r0, r1, r2, out_on_device, pitch0, pitch1, stats);
}

// ---- arrays of different shapes in one call
// the refusals of the shapes, before anything is launched or written: SZHIP_ERR_ARG (an extent that is no extent, no thread_num), SZHIP_ERR_UNSUP (an item of 2^32 values)
static int batch_shapes_args(szhip_ctx *ctx, const szhip_batch_shape *shapes, int count, bool compress)
{
    if (!shapes) return SZHIP_ERR_ARG;
    for (int i = 0; i < count; ++i) {
        const szhip_batch_shape &s = shapes[i];
        if (s.r0 < 1 || s.r1 < 1 || s.r2 < 1 || s.r0 > 0x7fffffff || s.r1 > 0x7fffffff || s.r2 > 0x7fffffff || (compress && s.thread_num < 1)) {
            snprintf(ctx->err, sizeof(ctx->err), "item %d of the batch: extents %zu x %zu x %zu, thread_num %d", i, s.r0, s.r1, s.r2, s.thread_num);
            return SZHIP_ERR_ARG;
        }
    }
    for (int i = 0; i < count; ++i)
        if ((double)shapes[i].r0 * (double)shapes[i].r1 * (double)shapes[i].r2 >= 4294967296.0) {
            snprintf(ctx->err, sizeof(ctx->err), "item %d of the batch: 2^32 values or more", i);
            return SZHIP_ERR_UNSUP;
        }
    return SZHIP_OK;
}
int szhip_compress_omp_batch_shapes(szhip_ctx *ctx, int dtype, szhip_batch_item *items, const szhip_batch_shape *shapes, int count, int data_on_device, const szhip_params *params,
                                    size_t meta_len, int out_on_device, unsigned char **blob, size_t *blob_size, szhip_stats *stats)
{
    if (!params || !blob || !blob_size) return SZHIP_ERR_ARG;
    TRY(batch_args(ctx, dtype, items, count, 1, 1, 1, true));
    TRY(batch_shapes_args(ctx, shapes, count, true));
    if (out_on_device != 0 && out_on_device != 1) { snprintf(ctx->err, sizeof(ctx->err), "a batch writes into a host blob (0) or the context's device blob (1)"); return SZHIP_ERR_UNSUP; }
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    for (int i = 0; i < count; ++i) { items[i].offset = items[i].size = 0; items[i].rc = SZHIP_OK; items[i].intervals = 0; items[i].n_unpred = 0; items[i].quant_kernel = 0; items[i].batched = 0; }
    *blob = nullptr; *blob_size = 0;
    return synced_on_failure(ctx, BY_DTYPE(dtype, compress_omp_batch_impl, ctx, items, count, data_on_device, shapes, 0, 0, 0, 0, 0, 0, params, meta_len, out_on_device, blob, blob_size, stats));
}
int szhip_decompress_omp_batch_shapes(szhip_ctx *ctx, int dtype, szhip_batch_item *items, const szhip_batch_shape *shapes, int count, int stream_on_device, int out_on_device,
                                      szhip_stats *stats)
{
    TRY(batch_args(ctx, dtype, items, count, 1, 1, 1, false));
    TRY(batch_shapes_args(ctx, shapes, count, false));
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    for (int i = 0; i < count; ++i) { items[i].rc = SZHIP_OK; items[i].intervals = 0; items[i].n_unpred = 0; items[i].quant_kernel = 0; items[i].batched = 0; }
    return synced_on_failure(ctx, BY_DTYPE(dtype, decompress_omp_batch_impl, ctx, items, count, stream_on_device, shapes, 0, 0, 0, out_on_device, 0, 0, stats));
}
int szhip_minmax_batch_lens(szhip_ctx *ctx, int dtype, const void *const *data, const size_t *lens, int count, int data_on_device, double *vmin, double *vmax, szhip_stats *stats)
{
    if (!vmin || !vmax || !lens) return SZHIP_ERR_ARG;
    TRY(batch_pointers(ctx, dtype, data, count, 1));
    size_t longest = 0;
    for (int i = 0; i < count; ++i) {
        if (lens[i] == 0) { snprintf(ctx->err, sizeof(ctx->err), "array %d of the batch: no values", i); return SZHIP_ERR_ARG; }
        if (lens[i] >= ((size_t)1 << 32)) { snprintf(ctx->err, sizeof(ctx->err), "array %d of the batch: 2^32 values or more", i); return SZHIP_ERR_UNSUP; }
        longest = lens[i] > longest ? lens[i] : longest;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    return synced_on_failure(ctx, BY_DTYPE(dtype, minmax_batch_impl, ctx, data, count, data_on_device, 1, 1, longest, longest, longest, lens, vmin, vmax, stats));
}

int szhip_decompress_omp_region(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len, size_t body_off,
                                size_t r0, size_t r1, size_t r2, const size_t lo[3], const size_t hi[3], void *out, int out_on_device, szhip_stats *stats)
{
    if (!ctx || !stream || !out || !lo || !hi || body_off >= stream_len) return SZHIP_ERR_ARG;
    if (r0 < 1 || r1 < 1 || r2 < 1 || r0 > 0x7fffffff || r1 > 0x7fffffff || r2 > 0x7fffffff) return SZHIP_ERR_ARG;
    const size_t r[3] = {r0, r1, r2};
    for (int k = 0; k < 3; ++k)
        if (lo[k] >= hi[k] || hi[k] > r[k]) {
            snprintf(ctx->err, sizeof(ctx->err), "region [%zu, %zu) of dimension %d is empty or beyond its extent %zu", lo[k], hi[k], k, r[k]);
            return SZHIP_ERR_ARG;
        }
    TRY(check_alignment_set_device(ctx, dtype, out));
    return synced_on_failure(ctx,
               BY_DTYPE(dtype, decompress_omp_region_impl, ctx, stream, stream_on_device, stream_len, body_off, r0, r1, r2, lo, hi, out, out_on_device, stats));
}

// ---- sub-boxes of many streams in one call.  SZHIP_ERR_ARG before anything is launched or written: the batch calls' refusals, an empty region or
// one beyond its item's extents, pitches that break the view rule
int szhip_decompress_omp_batch_region(szhip_ctx *ctx, int dtype, szhip_batch_item *items, const szhip_batch_shape *shapes, szhip_batch_region *regions, int count,
                                      int stream_on_device, int out_on_device, szhip_stats *stats)
{
    if (!regions) return SZHIP_ERR_ARG;
    TRY(batch_args(ctx, dtype, items, count, 1, 1, 1, false));
    TRY(batch_shapes_args(ctx, shapes, count, false));
    for (int i = 0; i < count; ++i) {
        const szhip_batch_region &rg = regions[i];
        const size_t r[3] = {shapes[i].r0, shapes[i].r1, shapes[i].r2};
        for (int k = 0; k < 3; ++k)
            if (rg.lo[k] >= rg.hi[k] || rg.hi[k] > r[k]) {
                snprintf(ctx->err, sizeof(ctx->err), "item %d of the batch: region [%zu, %zu) of dimension %d is empty or beyond its extent %zu", i, rg.lo[k], rg.hi[k], k, r[k]);
                return SZHIP_ERR_ARG;
            }
        if (rg.pitch0 != 0 || rg.pitch1 != 0) TRY(check_view(ctx, rg.hi[0] - rg.lo[0], rg.hi[1] - rg.lo[1], rg.hi[2] - rg.lo[2], rg.pitch0, rg.pitch1));
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    for (int i = 0; i < count; ++i) {
        items[i].rc = SZHIP_OK; items[i].intervals = 0; items[i].n_unpred = 0; items[i].quant_kernel = 0; items[i].batched = 0;
        regions[i].n_boxes = 0; regions[i].shares = i;
    }
    return synced_on_failure(ctx, BY_DTYPE(dtype, decompress_omp_batch_region_impl, ctx, items, shapes, regions, count, stream_on_device, out_on_device, stats));
}

// ---- views (szhip.h): a sub-box of r0 x r1 x r2 values whose planes lie pitch0 and whose rows pitch1 elements apart
static int check_view(szhip_ctx *ctx, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1)
{
    if (pitch1 < r2 || pitch1 > ((size_t)1 << 48) || (r0 != 0 && (pitch0 / pitch1 < r1 || pitch0 > ((size_t)1 << 48)))) {      // (a 2-D view: pitch0 is not looked at)
        snprintf(ctx->err, sizeof(ctx->err), "view pitches %zu / %zu below its extents %zu x %zu x %zu (pitch1 >= r2, pitch0 >= r1 * pitch1)", pitch0, pitch1, r0, r1, r2);
        return SZHIP_ERR_ARG;
    }
    return SZHIP_OK;
}
static bool view_dims_ok(size_t r0, size_t r1, size_t r2)      // 3-D, or (r0 == 0) 2-D; the launch grids count 16-byte pieces in 32 bits of workgroups
{
    return r1 >= 1 && r2 >= 1 && r0 <= 0x7fffffff && r1 <= 0x7fffffff && r2 <= 0x7fffffff - 64 &&       /* (the kernels step through a row in `int`, 16 bytes at a time) */ (double)(r0 ? r0 : 1) * (double)r1 * ((double)r2 / 2 + 2) < 256.0 * 4.0e9;
}

int szhip_pack_view(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1, void **d_packed)
{
    if (!ctx || !data || !d_packed || !view_dims_ok(r0, r1, r2)) return SZHIP_ERR_ARG;
    TRY(check_view(ctx, r0, r1, r2, pitch0, pitch1));
    TRY(check_alignment_set_device(ctx, dtype, data));
    const size_t n0 = r0 ? r0 : 1;
    TRY(ensure(ctx, ctx->in, n0 * r1 * r2 * (dtype == SZHIP_F32 ? 4 : 8)));
    TRY(synced_on_failure(ctx, BY_DTYPE(dtype, pack_view_impl, ctx, data, data_on_device, n0, r1, r2, r0 ? pitch0 : 0, pitch1, ctx->in.p)));
    *d_packed = ctx->in.p;
    return SZHIP_OK;
}

int szhip_scatter_view(szhip_ctx *ctx, int dtype, const void *d_packed, size_t r0, size_t r1, size_t r2, void *out, int out_on_device, size_t pitch0, size_t pitch1)
{
    if (!ctx || !d_packed || !out || !view_dims_ok(r0, r1, r2)) return SZHIP_ERR_ARG;
    TRY(check_view(ctx, r0, r1, r2, pitch0, pitch1));
    TRY(check_alignment_set_device(ctx, dtype, out));
    TRY(check_alignment_set_device(ctx, dtype, d_packed));
    return synced_on_failure(ctx, BY_DTYPE(dtype, scatter_view_impl, ctx, d_packed, r0 ? r0 : 1, r1, r2, out, out_on_device, r0 ? pitch0 : 0, pitch1));
}

int szhip_compress_omp_view(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1, double eb,
                            int thread_num, const szhip_params *params, const unsigned char *meta, size_t meta_len, int out_on_device, unsigned char **out,
                            size_t *out_size, szhip_stats *stats)
{
    if (!ctx || !data || !params || !meta || !out || !out_size) return SZHIP_ERR_ARG;
    if (r0 < 1 || r1 < 1 || r2 < 1 || r0 > 0x7fffffff || r1 > 0x7fffffff || r2 > 0x7fffffff || thread_num < 1) return SZHIP_ERR_ARG;
    if (!(eb > 0)) return SZHIP_ERR_ARG;
    TRY(check_view(ctx, r0, r1, r2, pitch0, pitch1));
    TRY(check_alignment_set_device(ctx, dtype, data));
    if (!data_on_device && (pitch1 != r2 || pitch0 != r1 * r2)) {      // a view on the host: its rows alone go to the device, packed; then the contiguous call
        if (r0 * r1 * r2 >= ((size_t)1 << 40)) return SZHIP_ERR_UNSUP;
        TRY(ensure(ctx, ctx->in, r0 * r1 * r2 * (dtype == SZHIP_F32 ? 4 : 8)));
        TRY(synced_on_failure(ctx, BY_DTYPE(dtype, pack_view_impl, ctx, data, 0, r0, r1, r2, pitch0, pitch1, ctx->in.p)));
        data = ctx->in.p; data_on_device = 1; pitch0 = r1 * r2; pitch1 = r2;
    }
    return synced_on_failure(ctx,
               BY_DTYPE(dtype, compress_omp_impl, ctx, data, data_on_device, r0, r1, r2, pitch0, pitch1, eb, thread_num, params, meta, meta_len, out_on_device, out, out_size, stats));
}

int szhip_decompress_omp_view(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len, size_t body_off,
                              size_t r0, size_t r1, size_t r2, void *out, int out_on_device, size_t pitch0, size_t pitch1, szhip_stats *stats)
{
    if (!ctx || !stream || !out || body_off >= stream_len) return SZHIP_ERR_ARG;
    if (r0 < 1 || r1 < 1 || r2 < 1 || r0 > 0x7fffffff || r1 > 0x7fffffff || r2 > 0x7fffffff) return SZHIP_ERR_ARG;
    TRY(check_view(ctx, r0, r1, r2, pitch0, pitch1));
    TRY(check_alignment_set_device(ctx, dtype, out));
    return synced_on_failure(ctx,
               BY_DTYPE(dtype, decompress_omp_impl, ctx, stream, stream_on_device, stream_len, body_off, r0, r1, r2, out, out_on_device, pitch0, pitch1, stats));
}

// ---- an array against its decoded copy (szhip.h): the error report
static int compare_args(szhip_ctx *ctx, int dtype, const void *ori, const void *dec, size_t r0, size_t r1, size_t r2, szhip_quality *q)
{
    if (!ctx || !ori || !dec || !q || (dtype != SZHIP_F32 && dtype != SZHIP_F64)) return SZHIP_ERR_ARG;
    if (r0 < 1 || r1 < 1 || r2 < 1 || r0 > 0x7fffffff || r1 > 0x7fffffff || (double)r0 * (double)r1 * (double)r2 >= 1099511627776.0) return SZHIP_ERR_ARG;
    return SZHIP_OK;
}

int szhip_compare_view(szhip_ctx *ctx, int dtype, const void *ori, int ori_on_device, size_t o_pitch0, size_t o_pitch1, const void *dec, int dec_on_device,
                       size_t d_pitch0, size_t d_pitch1, size_t r0, size_t r1, size_t r2, double abs_bound, double pw_rel_bound, unsigned flags, szhip_quality *q)
{
    TRY(compare_args(ctx, dtype, ori, dec, r0, r1, r2, q));
    TRY(check_view(ctx, r0, r1, r2, o_pitch0, o_pitch1));
    TRY(check_view(ctx, r0, r1, r2, d_pitch0, d_pitch1));
    TRY(check_alignment_set_device(ctx, dtype, ori));
    TRY(check_alignment_set_device(ctx, dtype, dec));
    return synced_on_failure(ctx, BY_DTYPE(dtype, quality_impl, ctx, ori, ori_on_device, o_pitch0, o_pitch1, dec, dec_on_device, d_pitch0, d_pitch1, r0, r1, r2,
                                           abs_bound, pw_rel_bound, flags, q));
}

int szhip_compare(szhip_ctx *ctx, int dtype, const void *ori, int ori_on_device, const void *dec, int dec_on_device, size_t n, double abs_bound, double pw_rel_bound,
                  unsigned flags, szhip_quality *q)
{
    TRY(compare_args(ctx, dtype, ori, dec, 1, 1, 1, q));
    if (n == 0 || n >= ((size_t)1 << 40)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, ori));
    TRY(check_alignment_set_device(ctx, dtype, dec));
    return synced_on_failure(ctx, BY_DTYPE(dtype, quality_impl, ctx, ori, ori_on_device, n, n, dec, dec_on_device, n, n, 1, 1, n, abs_bound, pw_rel_bound, flags, q));
}

int szhip_compare_batch(szhip_ctx *ctx, int dtype, const void *const *ori, const void *const *dec, int count, int on_device, size_t n, const double *abs_bound,
                        const double *pw_rel_bound, unsigned flags, szhip_quality *out, szhip_stats *stats)
{
    if (!abs_bound || !out) return SZHIP_ERR_ARG;
    TRY(batch_pointers(ctx, dtype, ori, count, n));
    TRY(batch_pointers(ctx, dtype, dec, count, n));
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    return synced_on_failure(ctx, BY_DTYPE(dtype, quality_batch_impl, ctx, ori, n, n, dec, n, n, count, on_device, 1, 1, n, abs_bound, pw_rel_bound, flags, out, stats));
}
int szhip_compare_batch_view(szhip_ctx *ctx, int dtype, const void *const *ori, size_t o_pitch0, size_t o_pitch1, const void *const *dec, size_t d_pitch0, size_t d_pitch1,
                             int count, int on_device, size_t r0, size_t r1, size_t r2, const double *abs_bound, const double *pw_rel_bound, unsigned flags,
                             szhip_quality *out, szhip_stats *stats)
{
    if (!abs_bound || !out) return SZHIP_ERR_ARG;
    if (r0 < 1 || r1 < 1 || r2 < 1 || r0 > 0x7fffffff || r1 > 0x7fffffff || r2 > 0x7fffffff) return SZHIP_ERR_ARG;
    TRY(batch_pointers(ctx, dtype, ori, count, 1));
    TRY(batch_pointers(ctx, dtype, dec, count, 1));
    TRY(check_view(ctx, r0, r1, r2, o_pitch0, o_pitch1));
    TRY(check_view(ctx, r0, r1, r2, d_pitch0, d_pitch1));
    if ((double)r0 * (double)r1 * (double)r2 >= 4294967296.0) { snprintf(ctx->err, sizeof(ctx->err), "szhip_compare_batch_view: boxes of 2^32 values or more"); return SZHIP_ERR_UNSUP; }
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    if (o_pitch1 == r2 && o_pitch0 == r1 * r2 && d_pitch1 == r2 && d_pitch0 == r1 * r2) {      // (the contiguous call, exactly)
        const size_t n = r0 * r1 * r2;
        r0 = r1 = 1; r2 = o_pitch0 = o_pitch1 = d_pitch0 = d_pitch1 = n;
    }
    return synced_on_failure(ctx, BY_DTYPE(dtype, quality_batch_impl, ctx, ori, o_pitch0, o_pitch1, dec, d_pitch0, d_pitch1, count, on_device, r0, r1, r2, abs_bound, pw_rel_bound, flags,
                                           out, stats));
}

int szhip_pwr_prepare(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t n, double vmin, double vmax, double pwr_ratio,
                      void **d_log, unsigned char *signs_host, int *positive, double *real_precision, double *value_range, double *median,
                      double *min_log_value)
{
    if (!ctx || !data || !n || !d_log || !positive || !real_precision || !value_range || !median || !min_log_value || !(pwr_ratio > 0)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, data));
    return synced_on_failure(ctx,
               BY_DTYPE(dtype, pwr_prepare_impl, ctx, data, data_on_device, n, vmin, vmax, pwr_ratio, d_log, signs_host, positive, real_precision, value_range, median, min_log_value));
}

int szhip_msst_prepare(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t n, double vmax, double pwr_ratio, void **d_prepared,
                       unsigned char *signs_host, int *positive, double *near_zero, double *median_log, double *min_log_value)
{
    if (!ctx || !data || !d_prepared || !positive || !near_zero || !median_log || !min_log_value || n == 0 || !(pwr_ratio > 0)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, data));
    return synced_on_failure(ctx,
               BY_DTYPE(dtype, msst_prepare_impl, ctx, data, data_on_device, n, vmax, pwr_ratio, d_prepared, signs_host, positive, near_zero, median_log, min_log_value));
}

int szhip_compress_sz14_pwr(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, double eb,
                            double value_range, double median, const szhip_params *params, const unsigned char *meta, size_t meta_len,
                            const szhip_pwr *pwr, int out_on_device, unsigned char **out, size_t *out_size, szhip_stats *stats)
{
    if (!ctx || !data || !params || !meta || !out || !out_size || !pwr || (pwr->signs_blob_size && !pwr->signs_blob)) return SZHIP_ERR_ARG;
    if (!dims_3d_2d_1d(r0, r1, r2)) return SZHIP_ERR_ARG;
    if (!(eb > 0)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, data));
    return guarded_compress(ctx, out, out_size, [&]() {
               return BY_DTYPE(dtype, compress14_impl, ctx, data, data_on_device, r0, r1, r2, eb, value_range, median, params, meta, meta_len, pwr, out_on_device, out, out_size, stats); });
}

int szhip_sz14_pwr_locate(int dtype, const unsigned char *stream, size_t stream_len, size_t body_off, size_t *blob_off, size_t *blob_size, double *min_log_value)
{
    if (!stream || !blob_off || !blob_size || !min_log_value) return SZHIP_ERR_ARG;
    const size_t es = dtype == SZHIP_F32 ? 4 : 8;
    if (stream_len < 4) return SZHIP_ERR_STREAM;
    const size_t x = (stream[3] & 0x08) ? 2 : 0;                                    // table-driven form: plus_bits, max_bits after reqLength (:164-168)
    const size_t fixed = 4 + 1 + 8 + 4 + 4 + es + 1 + x + 8 + 8 + 8 + 8 + es;      // ... up to the type array (TightDataPointStorageF.c:133-240)
    if (body_off + fixed > stream_len) return SZHIP_ERR_STREAM;
    const unsigned char *q = stream + body_off + 4 + 1 + 8;
    *blob_size = szhost_get_u32be(q); q += 4 + 4 + es + 1 + x + 8;
    const uint64_t type_size = szhost_get_u64be(q); q += 8 + 8 + 8;
    *min_log_value = dtype == SZHIP_F32 ? (double)szhost_get_f32be(q) : szhost_get_f64be(q);
    if (type_size > stream_len || *blob_size > stream_len || body_off + fixed + type_size + *blob_size > stream_len) return SZHIP_ERR_STREAM;
    *blob_off = body_off + fixed + (size_t)type_size;
    return SZHIP_OK;
}

int szhip_decompress_sz14_pwr(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len, size_t body_off,
                              size_t r0, size_t r1, size_t r2, const unsigned char *signs_host, void *out, int out_on_device, szhip_stats *stats)
{
    if (!ctx || !stream || !out || body_off >= stream_len) return SZHIP_ERR_ARG;
    if (!dims_3d_2d_1d(r0, r1, r2)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, out));
    // the fixed fields in front of the type array are read on the host: of a device-resident stream they are fetched, the rest stays where it is
    unsigned char head[160]; const unsigned char *hs = stream;
    if (stream_on_device) {
        const size_t want = std::min<size_t>(stream_len, body_off + 80);
        if (want > sizeof(head)) return SZHIP_ERR_ARG;
        HIPCHK(hipMemcpyAsync(head, stream, want, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        hs = head;
    }
    size_t bo, bs; double thr;
    if (szhip_sz14_pwr_locate(dtype, hs, stream_len, body_off, &bo, &bs, &thr) != SZHIP_OK) return SZHIP_ERR_STREAM;
    const bool msst = (hs[3] & 0x08) != 0;                       // TightDataPointStorageF.c:81
    return drained_on_failure(ctx, with_ticket_fallback(ctx, [&]() {
               return BY_DTYPE(dtype, decompress14_pwr_impl, ctx, stream, stream_on_device ? 1 : 0, stream_len, body_off, r0, r1, r2, signs_host, thr, msst, out, out_on_device, stats); }));
}

int szhip_decompress(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len, size_t body_off,
                     size_t r0, size_t r1, size_t r2, void *out, int out_on_device, szhip_stats *stats)
{
    if (!ctx || !stream || !out || body_off >= stream_len) return SZHIP_ERR_ARG;
    if (!dims_3d_2d(r0, r1, r2)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, out));
    return with_ticket_fallback(ctx, [&]() {
               return BY_DTYPE(dtype, decompress_impl, ctx, stream, stream_on_device, stream_len, body_off, r0, r1, r2, out, out_on_device, stats); });
}

int szhip_huff_book(szhip_ctx *ctx, const void *hist, unsigned intervals, unsigned char *out_tree, size_t out_tree_cap,
                    uint64_t *out_code64, uint8_t *out_len8, szhip_book_record *record)
{
    if (!ctx || !hist || !out_tree || !out_code64 || !out_len8 || !record || intervals == 0 || intervals > 65536) return SZHIP_ERR_ARG;
    static_assert(sizeof(szhip_book_record) == sizeof(szh_book_rec), "the public record mirrors the kernel's");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    bool on_device = false;
#ifndef SZH_SYNC_LAUNCH
    { hipPointerAttribute_t pa; if (hipPointerGetAttributes(&pa, hist) == hipSuccess) on_device = pa.type == hipMemoryTypeDevice; else (void)hipGetLastError(); }
#endif
    const size_t tree_cap = std::min<size_t>(std::max<size_t>(out_tree_cap, 1), 1 + (size_t)9 * (2 * SZH_BOOK_CAP - 1));
    TRY(ensure(ctx, ctx->code_tab, (size_t)intervals * 8)); TRY(ensure(ctx, ctx->len_tab, (size_t)intervals));
    TRY(ensure(ctx, ctx->book_tree, tree_cap)); TRY(ensure(ctx, ctx->book_rec, 32 + SZH_PLAN_COUNT * 8));
    const unsigned *d_hist = (const unsigned *)hist;
    if (!on_device) {
        TRY(ensure(ctx, ctx->hist, (size_t)(65536 + 8192) * 4 + 64));
        HIPCHK(hipMemcpyAsync(ctx->hist.p, hist, (size_t)intervals * 4, hipMemcpyHostToDevice, st));
        d_hist = (const unsigned *)ctx->hist.p;
    }
    HIPCHK(hipMemsetAsync(ctx->code_tab.p, 0xA5, (size_t)intervals * 8, st));
    HIPCHK(hipMemsetAsync(ctx->len_tab.p, 0xA5, (size_t)intervals, st));
    HIPCHK(hipMemsetAsync(ctx->book_tree.p, 0xA5, tree_cap, st));
    hipLaunchKernelGGL(k_huff_book, dim3(1), dim3(256), 0, st, d_hist, intervals, SZH_BOOK_TAB_RAW, (unsigned char *)ctx->book_tree.p, (unsigned)std::min<size_t>(out_tree_cap, tree_cap),
                       (u64 *)ctx->code_tab.p, (uint8_t *)ctx->len_tab.p, (szh_book_rec *)ctx->book_rec.p, (u64 *)nullptr, (u64)0, 0u, (u64)0, (u64)0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_code64, ctx->code_tab.p, (size_t)intervals * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_len8, ctx->len_tab.p, (size_t)intervals, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_tree, ctx->book_tree.p, std::min<size_t>(out_tree_cap, tree_cap), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(record, ctx->book_rec.p, sizeof(*record), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SZHIP_OK;
}

// ---- the copy-shaped passes of the drop-in calls for device-resident arrays (szhip.h; kernels: szh_store.h)
static unsigned store_grid(size_t n, int dtype)       // a lane per 16-byte piece, grid-stride beyond 2048 workgroups
{
    const size_t pieces = n / (dtype == SZHIP_F32 ? 4 : 2) + 1;
    return (unsigned)std::min<size_t>((pieces + 255) / 256, 2048);
}
static bool store_count_ok(size_t n) { return n >= 1 && n < ((size_t)1 << 59); }

int szhip_store_be(szhip_ctx *ctx, int dtype, const void *d_src, size_t n, const void *zero_replacement, unsigned char *dst, int dst_on_device)
{
    if (!ctx || !d_src || !dst || !store_count_ok(n) || (dtype != SZHIP_F32 && dtype != SZHIP_F64)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, d_src));
    const size_t bytes = n * (dtype == SZHIP_F32 ? 4 : 8);
    unsigned char *d_dst = dst;
    if (!dst_on_device) { TRY(ensure(ctx, ctx->stream_buf, bytes)); d_dst = (unsigned char *)ctx->stream_buf.p; }
    if (dtype == SZHIP_F32) {
        float r = 0; if (zero_replacement) memcpy(&r, zero_replacement, 4);
        hipLaunchKernelGGL((k_store_be<float>), dim3(store_grid(n, dtype)), dim3(256), 0, ctx->stream, (const float *)d_src, d_dst, (int64_t)n, zero_replacement ? 1 : 0, r);
    } else {
        double r = 0; if (zero_replacement) memcpy(&r, zero_replacement, 8);
        hipLaunchKernelGGL((k_store_be<double>), dim3(store_grid(n, dtype)), dim3(256), 0, ctx->stream, (const double *)d_src, d_dst, (int64_t)n, zero_replacement ? 1 : 0, r);
    }
    HIPCHK(hipGetLastError());
    if (!dst_on_device) return synced_on_failure(ctx, staged_copy(ctx, dst, d_dst, bytes, false));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SZHIP_OK;
}

int szhip_load_be(szhip_ctx *ctx, int dtype, const unsigned char *src, int src_on_device, size_t n, void *d_out)
{
    if (!ctx || !src || !d_out || !store_count_ok(n) || (dtype != SZHIP_F32 && dtype != SZHIP_F64)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, d_out));
    const size_t bytes = n * (dtype == SZHIP_F32 ? 4 : 8);
    const unsigned char *d_src = src;
    if (!src_on_device) {
        TRY(ensure(ctx, ctx->stream_buf, bytes));
        TRY(synced_on_failure(ctx, staged_copy(ctx, ctx->stream_buf.p, src, bytes, true)));
        d_src = (const unsigned char *)ctx->stream_buf.p;
    }
    if (dtype == SZHIP_F32) hipLaunchKernelGGL((k_load_be<float>), dim3(store_grid(n, dtype)), dim3(256), 0, ctx->stream, d_src, (float *)d_out, (int64_t)n);
    else hipLaunchKernelGGL((k_load_be<double>), dim3(store_grid(n, dtype)), dim3(256), 0, ctx->stream, d_src, (double *)d_out, (int64_t)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SZHIP_OK;
}

int szhip_fill(szhip_ctx *ctx, int dtype, const void *value, size_t n, void *d_out)
{
    if (!ctx || !value || !d_out || !store_count_ok(n) || (dtype != SZHIP_F32 && dtype != SZHIP_F64)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, d_out));
    if (dtype == SZHIP_F32) { float v; memcpy(&v, value, 4); hipLaunchKernelGGL((k_fill<float>), dim3(store_grid(n, dtype)), dim3(256), 0, ctx->stream, (float *)d_out, (int64_t)n, v); }
    else { double v; memcpy(&v, value, 8); hipLaunchKernelGGL((k_fill<double>), dim3(store_grid(n, dtype)), dim3(256), 0, ctx->stream, (double *)d_out, (int64_t)n, v); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SZHIP_OK;
}

int szhip_clamp(szhip_ctx *ctx, int dtype, void *d_data, size_t n, double vmin, double vmax)
{
    if (!ctx || !d_data || !store_count_ok(n) || (dtype != SZHIP_F32 && dtype != SZHIP_F64)) return SZHIP_ERR_ARG;
    TRY(check_alignment_set_device(ctx, dtype, d_data));
    if (dtype == SZHIP_F32) hipLaunchKernelGGL((k_clamp<float>), dim3(store_grid(n, dtype)), dim3(256), 0, ctx->stream, (float *)d_data, (int64_t)n, (float)vmin, (float)vmax);
    else hipLaunchKernelGGL((k_clamp<double>), dim3(store_grid(n, dtype)), dim3(256), 0, ctx->stream, (double *)d_data, (int64_t)n, vmin, vmax);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SZHIP_OK;
}

int szhip_copy(szhip_ctx *ctx, void *dst, const void *src, size_t bytes, int to_device)
{
    if (!ctx || !dst || !src) return SZHIP_ERR_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    if (bytes == 0) return SZHIP_OK;
    return synced_on_failure(ctx, staged_copy(ctx, dst, src, bytes, to_device != 0));
}

int szhip_debug_fetch(szhip_ctx *ctx, int which, void *dst, size_t bytes)
{
    if (!ctx || !dst) return SZHIP_ERR_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return SZHIP_ERR_NODEVICE;
    DevBuf *bufs[] = {&ctx->coef, &ctx->blk_lor, &ctx->codes_nat, &ctx->codes_blk, &ctx->hist, &ctx->col_zeros, &ctx->col_off,
                      &ctx->unpred, &ctx->stream_buf, &ctx->rb_down, &ctx->rb_right, &ctx->small, &ctx->in, &ctx->batch_blob};
    if (which < 0 || which >= (int)(sizeof(bufs) / sizeof(bufs[0]))) return SZHIP_ERR_ARG;
    if (!bufs[which]->p || bufs[which]->cap < bytes) return SZHIP_ERR_ARG;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(dst, bufs[which]->p, bytes, hipMemcpyDeviceToHost));
    return SZHIP_OK;
}

} // extern "C"
