// szhip_ompbatch.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace, behind szhip_omp.inc): the OpenMP container over many
// same-shape arrays in one call (include/szhip.h: szhip_compress_omp_batch, szhip_decompress_omp_batch; kernels: szh_ompbatch.h; DESIGN section 4.5.3).
// The steps are those of omp_call / omp_dec, each ONE launch with the array as the grid's second dimension; what a step of the single call keeps in members is here a
// per-array record (szh_ompb_rec) in a device table that is uploaded whole whenever the host has learnt something new about the arrays (the interval counts, the books).
// An array the shared launches do not cover goes through compress_omp_impl / decompress_omp_impl from inside the call.
// The same two functions serve arrays of DIFFERENT shapes (szhip_compress_omp_batch_shapes / szhip_decompress_omp_batch_shapes; DESIGN section 4.5.7): the geometry is
// then per item (ompb_shape on the host, szh_ompb_geo in the device table), the work arrays lie at prefix sums of each item's own lengths, the launches are the k_ompbs_*
// wrappers sized to their largest item, and the conditions that send a whole same-shape batch to the single calls send one item there.
// =====================================================================================================================
// (`g` carries the pitches of the array `base` lies in -- a view's after omp_view_pitches --, pitch0 / pitch1 are the same in elements)
static int omp_form(const szh_omp_geom &g, const void *base, size_t elem, size_t pitch0, size_t pitch1)
{
    if (omp_col_applies(g, base, pitch1 * elem, pitch0 * elem)) return 3;
    return g.vec && ((uintptr_t)base & 15u) == 0 ? 4 : 5;
}
// (`boxes`, `values`: of all arrays of the batch together)
static int ompb_limits(szhip_ctx *ctx, int count, size_t boxes, size_t values)
{
    if (count > 65535 || boxes > ((size_t)1 << 22) || values >= ((size_t)1 << 32))
        FAIL(SZHIP_ERR_UNSUP, "OpenMP-container batch: %d arrays of %zu boxes and %zu values in all (at most 65535 arrays, 2^22 boxes and 2^32 - 1 values)", count, boxes, values);
    return SZHIP_OK;
}
// `count` host arrays of `bytes` bytes each, one behind the other at multiples of 16 into `buf` (asynchronous on `st`; the callers' arrays have been read on return):
// ONE copy through the context's pinned block when they total at most 64 MiB, else array by array.  d[i]: where array i lies then.
// `hv`: the host arrays are VIEWS of `bytes` bytes each (the batched view calls): their rows alone are copied, packed, as staged_copy does with a host view.
// `each` (or null): array i has each[i] bytes, not `bytes` (arrays of different shapes: every one at its own length, still at multiples of 16)
template <class GET>
int batch_stage(szhip_ctx *ctx, DevBuf &buf, int count, size_t bytes, hipStream_t st, GET &&host, std::vector<const void *> &d, const host_view *hv = nullptr,
                const size_t *each = nullptr)
{
    std::vector<size_t> at((size_t)count + 1, 0);
    for (int i = 0; i < count; ++i) at[i + 1] = at[i] + up16(each ? each[i] : bytes);
    const size_t total = at[count];
    d.resize((size_t)count);
    TRY(ensure(ctx, buf, total));
    for (int i = 0; i < count; ++i) d[i] = (const char *)buf.p + at[i];
    if (total <= ((size_t)64 << 20)) {
        TRY(ensure_pinned3(ctx, total));
        for (int i = 0; i < count; ++i) {
            if (hv) host_view_move(*hv, (char *)const_cast<void *>((const void *)host(i)), (char *)ctx->pinned3 + at[i], 0, bytes, true);
            else memcpy((char *)ctx->pinned3 + at[i], host(i), each ? each[i] : bytes);
        }
        HIPCHK(hipMemcpyAsync(buf.p, ctx->pinned3, total, hipMemcpyHostToDevice, st));
    } else for (int i = 0; i < count; ++i) TRY(staged_copy(ctx, (char *)buf.p + at[i], host(i), each ? each[i] : bytes, true, hv));
    return SZHIP_OK;
}
// the device table of a batch in ctx->batch_rec: [totals: 4 u64 per array][records][LISTS lists of `count` array numbers][what a version of the table adds behind]
// (F3G / PACKG: the items of a batched view call that run in a contiguous copy -- gathered views --, apart from those that are addressed where they lie, F3 / F4 / F5 /
//  PACKD: the two take different geometries, so every launch that reads or writes values through the geometry has one list for each.  PACK = PACKD + PACKG.)
enum { OMPB_L_ALL = 0, OMPB_L_F3, OMPB_L_F4, OMPB_L_F5, OMPB_L_ENT, OMPB_L_PACK, OMPB_L_F3G, OMPB_L_PACKD, OMPB_L_PACKG, OMPB_LISTS };
struct ompb_table {
    szhip_ctx *ctx; int count;
    std::vector<szh_ompb_rec> rec; std::vector<int> list[OMPB_LISTS];
    std::vector<szh_ompb_geo> geo;                          // a call on arrays of different shapes: every array's own geometry, between the lists and `extra` (else empty)
    size_t o_rec, o_list, o_geo, o_extra;
    std::vector<unsigned char> image[3];                    // the host copies of the uploads (one per version: a pageable source stays untouched until the next synchronisation)
    ompb_table(szhip_ctx *c, int n, bool with_geo = false) : ctx(c), count(n), rec((size_t)n), geo(with_geo ? (size_t)n : 0)
    {
        memset(rec.data(), 0, rec.size() * sizeof(szh_ompb_rec));
        if (with_geo) memset(geo.data(), 0, geo.size() * sizeof(szh_ompb_geo));
        o_rec = up64((size_t)n * 32); o_list = o_rec + (size_t)n * sizeof(szh_ompb_rec); o_geo = up64(o_list + (size_t)OMPB_LISTS * n * 4);
        o_extra = up64(o_geo + geo.size() * sizeof(szh_ompb_geo));
    }
    int reserve(size_t extra) { return ensure(ctx, ctx->batch_rec, o_extra + extra + 64); }
    unsigned char *dev() const { return (unsigned char *)ctx->batch_rec.p; }
    u64 *totals(int i) const { return (u64 *)dev() + 4 * (size_t)i; }
    const szh_ompb_rec *d_rec() const { return (const szh_ompb_rec *)(dev() + o_rec); }
    const szh_ompb_geo *d_geo() const { return (const szh_ompb_geo *)(dev() + o_geo); }
    const int *d_list(int which) const { return (const int *)(dev() + o_list) + (size_t)which * count; }
    int clear_totals() { HIPCHK(hipMemsetAsync(dev(), 0, (size_t)count * 32, ctx->stream)); return SZHIP_OK; }
    // records, lists and `extra` (placed at o_extra) to the device
    int upload(int version, const std::vector<unsigned char> &extra)
    {
        std::vector<unsigned char> &im = image[version];
        im.assign(o_extra - o_rec + extra.size(), 0);
        memcpy(im.data(), rec.data(), rec.size() * sizeof(szh_ompb_rec));
        for (int l = 0; l < OMPB_LISTS; ++l) if (!list[l].empty()) memcpy(im.data() + (o_list - o_rec) + (size_t)l * count * 4, list[l].data(), list[l].size() * 4);
        if (!geo.empty()) memcpy(im.data() + (o_geo - o_rec), geo.data(), geo.size() * sizeof(szh_ompb_geo));
        if (!extra.empty()) memcpy(im.data() + (o_extra - o_rec), extra.data(), extra.size());
        HIPCHK(hipMemcpyAsync(dev() + o_rec, im.data(), im.size(), hipMemcpyHostToDevice, ctx->stream));
        return SZHIP_OK;
    }
};
// what the host knows of item i's geometry: extents, values, boxes, thread_num, omp_box_grid's verdict on them and its grid
struct ompb_shape { size_t r0, r1, r2, n, nb; int thread_num, rc; szh_omp_geom g; };
static ompb_shape ompb_shape_of(size_t r0, size_t r1, size_t r2) { ompb_shape s; memset(&s, 0, sizeof(s)); s.r0 = r0; s.r1 = r1; s.r2 = r2; s.n = r0 * r1 * r2; s.rc = SZHIP_OK; return s; }
// the items of `l` ordered so that those with equal boxes c0 x c1 x c2 stand together (one k_ompbs_box launch per such run): where the runs end
static std::vector<int> ompb_box_runs(std::vector<int> &l, const std::vector<ompb_shape> &sh)
{
    auto less = [&](int a, int b) {
        const szh_omp_geom &x = sh[a].g, &y = sh[b].g;
        return x.c0 != y.c0 ? x.c0 < y.c0 : x.c1 != y.c1 ? x.c1 < y.c1 : x.c2 < y.c2;
    };
    std::stable_sort(l.begin(), l.end(), less);
    std::vector<int> ends;
    for (size_t k = 0; k < l.size(); ++k) if (k + 1 == l.size() || less(l[k], l[k + 1])) ends.push_back((int)k + 1);
    return ends;
}
// the largest box count among the items l[from .. to): what sizes the first dimension of a launch over them
static size_t ompb_most_boxes(const std::vector<int> &l, int from, int to, const std::vector<ompb_shape> &sh)
{
    size_t m = 1;
    for (int k = from; k < to; ++k) m = std::max(m, sh[l[k]].nb);
    return m;
}
// which list an item of the shared sweeps goes to
static int ompb_form_list(bool gathered, int form) { return gathered ? OMPB_L_F3G : form == 3 ? OMPB_L_F3 : form == 4 ? OMPB_L_F4 : OMPB_L_F5; }
// The sweeps over items of DIFFERENT shapes (k_ompbs_*; DEC: the inverse sweeps): the column form in ONE launch for every item with 32 x 32 faces, the box forms in one
// launch per run of equal boxes (the block is the box's face, the LDS its ring).  `runs`: ompb_box_runs of the lists of forms 4 and 5.  Returns the number of launches.
template <class T, bool DEC>
int ompb_sweep_mixed(hipStream_t st, const ompb_table &tab, const std::vector<ompb_shape> &sh, const std::vector<int> runs[2])
{
    const int n3 = (int)tab.list[OMPB_L_F3].size();
    int launches = n3 ? 1 : 0;
    if (n3) hipLaunchKernelGGL((k_ompbs_col<T, 32, 32, DEC, DEC>), dim3((unsigned)(ompb_most_boxes(tab.list[OMPB_L_F3], 0, n3, sh) / 2), (unsigned)n3), dim3(64), 0, st, tab.d_rec(), tab.d_geo(),
                               tab.d_list(OMPB_L_F3));
    for (int form = 4; form <= 5; ++form) {
        const int which = form == 4 ? OMPB_L_F4 : OMPB_L_F5;
        int from = 0;
        for (int to : runs[form - 4]) {
            const szh_omp_geom &gb = sh[tab.list[which][from]].g;
            const dim3 grid((unsigned)ompb_most_boxes(tab.list[which], from, to, sh), (unsigned)(to - from)), block((unsigned)(gb.c0 * gb.c1));
            const size_t lds = (size_t)4 * gb.c0 * gb.pitch * sizeof(T);
            hipLaunchKernelGGL((form == 4 ? k_ompbs_box<T, DEC, true> : k_ompbs_box<T, DEC, false>), grid, block, lds, st, tab.d_rec(), tab.d_geo(), tab.d_list(which) + from);
            ++launches;
            from = to;
        }
    }
    return launches;
}
// The sweeps over items of ONE shape (k_ompb_*), one launch per form.  `gv`: the items where they lie -- `g` itself in a contiguous call; `g`: the contiguous copies of
// the gathered views.  `fw`: the flag words of the inverse column sweep (0 in a compress call).  Returns the number of launches.
template <class T, bool DEC>
int ompb_sweep_same(hipStream_t st, const ompb_table &tab, const szh_omp_geom &g, const szh_omp_geom &gv, int fw)
{
    const int n3 = (int)tab.list[OMPB_L_F3].size(), n3g = (int)tab.list[OMPB_L_F3G].size(), n4 = (int)tab.list[OMPB_L_F4].size(), n5 = (int)tab.list[OMPB_L_F5].size();
    const size_t nb = (size_t)g.nb;
    const int rows = g.c0 * g.c1;
    const size_t box_lds = (size_t)4 * g.c0 * g.pitch * sizeof(T);
    if (n3) hipLaunchKernelGGL((k_ompb_col<T, 32, 32, DEC, DEC>), dim3((unsigned)(nb / 2), (unsigned)n3), dim3(64), 0, st, gv, tab.d_rec(), tab.d_list(OMPB_L_F3), fw);
    if (n3g) hipLaunchKernelGGL((k_ompb_col<T, 32, 32, DEC, DEC>), dim3((unsigned)(nb / 2), (unsigned)n3g), dim3(64), 0, st, g, tab.d_rec(), tab.d_list(OMPB_L_F3G), fw);
    if (n4) hipLaunchKernelGGL((k_ompb_box<T, DEC, true>), dim3((unsigned)nb, (unsigned)n4), dim3((unsigned)rows), box_lds, st, gv, tab.d_rec(), tab.d_list(OMPB_L_F4));
    if (n5) hipLaunchKernelGGL((k_ompb_box<T, DEC, false>), dim3((unsigned)nb, (unsigned)n5), dim3((unsigned)rows), box_lds, st, gv, tab.d_rec(), tab.d_list(OMPB_L_F5));
    return (n3 ? 1 : 0) + (n3g ? 1 : 0) + (n4 ? 1 : 0) + (n5 ? 1 : 0);
}
// pitch0 / pitch1: the element pitches of the arrays the items' sub-boxes lie in (szhip_compress_omp_batch_view; r1 * r2 and r2: contiguous arrays).  A view on the
// device takes one of two ways, per item (omp_view_packs, as in the single view call): where it lies, through the pitched geometry `gv`, or GATHERED into a contiguous
// copy in the context's input buffer by one k_ompb_crop launch for all such items, where it runs the column form through `g`.  Host views are staged packed.
// One batch compress call: its state, and one member function per step (compress_omp_batch_impl is their sequence).  What the steps rely on:
//  - Context buffers.  prepare() sizes codes_nat, zcnt, samples, col_zeros64, col_off, reg_flags and reg_rank for the BATCH items only: an EARLY single call (sort_items)
//    of a larger item may MOVE any of them.  Harmless: nothing of the batch lies in them yet, and every step reads their addresses where it uses them (fill_static,
//    d_hist), never from a copy taken earlier.  ctx->hist alone is never smaller than a single call asks for (its 65536 + 8192 bins).  The single calls and the gather
//    of the views both use ctx->in: the EARLY calls run first, the gather after them (sweep_and_books), so the sampling launch reads every view where it lies.  chunk_bits (sweep_and_books),
//    unpred (pack) and batch_blob (pack) are sized when their content is known; the LATE calls run when the batch is through with all of them.
//  - The table moves when it is reserved again (prepare, pack) and the totals with it: fill_static() is repeated after every tab.reserve and every change of `src`.
//  - `tab` is a member: its image[version] vectors, the pageable sources of the asynchronous uploads (one per version), outlive every upload.
template <class T>
struct ompb_enc : call_base {
    enum { BATCH, EARLY, LATE, FAILED };                      // an item: in the shared launches; the single call before / behind them; refused
    szhip_batch_item *const items; const int count, data_on_device; const bool mixed; const size_t r0, r1, r2, in_pitch0, in_pitch1; const int thread_num;
    const szhip_params *const prm; const size_t meta_len; const int out_on_device;
    const bool host_view_in = !data_on_device && (in_pitch1 != r2 || in_pitch0 != r1 * r2);      // (staged packed: contiguous from there on)
    const size_t pitch0 = host_view_in ? r1 * r2 : in_pitch0, pitch1 = host_view_in ? r2 : in_pitch1;
    const bool view = pitch1 != r2 || pitch0 != r1 * r2;
    const unsigned max_radius = prm->max_quant_intervals / 2; const bool optimise = prm->quantization_intervals == 0;
    std::vector<int> state; std::vector<ompb_shape> sh;
    szh_omp_geom g, gv; bool shared = false;                  // the same-shape call's grid; `gv`: of the items where they lie
    // the work arrays of the shared launches: item i's codes behind those of the items before it (n is a multiple of 8: 16-byte reads stay aligned), its per-box
    // tables -- nb or nb + 1 entries -- at multiples of 16 entries (every table keeps the alignment its allocation gives it in the single call)
    std::vector<size_t> o_code, o_box, o_hb; size_t n_codes = 0, n_slots = 0, hb_bytes = 0, hist_lds = 16, lds3_max = 16, pos = 0;
    std::vector<char> gathered; std::vector<const T *> d_in, src;                        // where array i lies on the device; where the shared launches read it (a gathered view: its contiguous copy)
    std::vector<std::vector<unsigned char>> fb;               // the streams of the single calls, on the host until the blob is laid out
    ompb_table tab{ctx, count, mixed};
    unsigned char *d_blob = nullptr;
    unsigned *d_hist() const { return (unsigned *)ctx->hist.p; }      // (read where it is used: see the context buffers above)
    std::vector<unsigned> iv; std::vector<int> box_runs[2]; int n_ent = 0, n_pack = 0;
    std::vector<std::vector<unsigned char>> hdr; std::vector<std::vector<u64>> packed;
    std::vector<u64> E, total_bits; std::vector<size_t> off_pay, cap_len;

    size_t p0(int i) const { return mixed ? sh[i].r1 * sh[i].r2 : pitch0; }      // the element pitches of the array item i lies in
    size_t p1(int i) const { return mixed ? sh[i].r2 : pitch1; }
    // ---- the grids (a shape the single call refuses: that item alone), the limits, who can share launches, the places of the work arrays; the inputs staged
    int inputs(const szhip_batch_shape *shapes) {
        state.assign((size_t)count, BATCH); sh.resize((size_t)count);
        memset(&g, 0, sizeof(g));
        if (mixed) {
            for (int i = 0; i < count; ++i) {
                ompb_shape &s = sh[i];
                s.r0 = shapes[i].r0; s.r1 = shapes[i].r1; s.r2 = shapes[i].r2; s.thread_num = shapes[i].thread_num; s.n = s.r0 * s.r1 * s.r2;
                s.rc = omp_box_grid(ctx, s.thread_num, s.r0, s.r1, s.r2, &s.g);
                s.nb = s.rc == SZHIP_OK ? (size_t)s.g.nb : 0;
                if (s.rc != SZHIP_OK) { state[i] = FAILED; items[i].rc = s.rc; }
            }
        } else {
            TRY(omp_box_grid(ctx, thread_num, r0, r1, r2, &g));
            const ompb_shape s = {r0, r1, r2, r0 * r1 * r2, (size_t)g.nb, thread_num, SZHIP_OK, g};
            sh.assign((size_t)count, s);
        }
        gv = g;
        if (view) omp_view_pitches(&gv, pitch0, pitch1, sizeof(T));
        size_t sum_n = 0, sum_nb = 0;
        for (const ompb_shape &s : sh) { sum_n += s.n; sum_nb += s.nb; }
        TRY(ompb_limits(ctx, count, sum_nb, sum_n));
        S.n_elements = (uint64_t)sum_n; S.n_blocks = (uint64_t)sum_nb;
        // an array that misses box_hist's conditions whatever its intervals, or whose samples the walk of k_sample_walk takes: through the single call (one shape: every array)
        for (int i = 0; i < count; ++i) {
            if (state[i] != BATCH) continue;
            if (omp_box_hist_shape(sh[i].g.bel) && sh[i].r0 > 1 && sh[i].r1 > 1) shared = true; else state[i] = EARLY;
        }
        o_code.assign((size_t)count, 0); o_box = o_code; o_hb = o_code;
        for (int i = 0; i < count; ++i) if (state[i] == BATCH) { o_code[i] = n_codes; n_codes += sh[i].n; o_box[i] = n_slots; n_slots += (sh[i].nb + 1 + 15) / 16 * 16; }
        // 1. host arrays one behind the other into the context's input buffer
        d_in.resize((size_t)count);
        if (data_on_device) for (int i = 0; i < count; ++i) d_in[i] = (const T *)items[i].data;
        else {
            const host_view hv = {r1, r2 * sizeof(T), in_pitch0 * sizeof(T), in_pitch1 * sizeof(T)};
            std::vector<const void *> d; std::vector<size_t> each;
            if (mixed) for (const ompb_shape &s : sh) each.push_back(s.n * sizeof(T));
            TRY(batch_stage(ctx, ctx->in, count, r0 * r1 * r2 * sizeof(T), st, [&](int i) { return items[i].data; }, d, host_view_in ? &hv : nullptr, mixed ? each.data() : nullptr));
            for (int i = 0; i < count; ++i) d_in[i] = (const T *)d[i];
        }
        src = d_in;
        gathered.assign((size_t)count, 0);
        if (view) for (int i = 0; i < count; ++i) gathered[i] = omp_view_packs(g, d_in[i], pitch0, pitch1, sizeof(T)) ? 1 : 0;
        fb.resize((size_t)count);
        return SZHIP_OK;
    }
    // the single call for array i, from the device copy of it
    void single(int i) {
        unsigned char *p = nullptr; size_t len = 0; szhip_stats s1;
        memset(&s1, 0, sizeof(s1));
        const int rc = compress_omp_impl<T>(ctx, d_in[i], 1, sh[i].r0, sh[i].r1, sh[i].r2, p0(i), p1(i), items[i].eb, sh[i].thread_num, prm, items[i].meta, meta_len, 0, &p, &len, &s1);
        items[i].rc = rc; items[i].batched = 0;
        if (rc == SZHIP_OK) {
            fb[i].assign(p, p + len); free(p);
            items[i].intervals = s1.intervals; items[i].n_unpred = s1.n_unpred; items[i].quant_kernel = s1.quant_kernel;
        } else { hipStreamSynchronize(st); state[i] = FAILED; }
    }
    // ---- the buffers and per-array tables of the shared launches.  2. the interval optimiser: one sampling launch, one read-back, pick_intervals per array
    int prepare() {
        if (shared) {
            TRY(tab.reserve(view ? (size_t)count * 16 : 0));       // (a view call: the gather's pairs of addresses behind the lists)
            TRY(ensure(ctx, ctx->codes_nat, n_codes * 2 + 64));
            TRY(ensure(ctx, ctx->zcnt, n_slots * 4)); TRY(ensure(ctx, ctx->samples, n_slots * sizeof(T)));
            TRY(ensure(ctx, ctx->col_zeros64, n_slots * 8)); TRY(ensure(ctx, ctx->col_off, n_slots * 8));
            TRY(ensure(ctx, ctx->reg_flags, n_slots * 8)); TRY(ensure(ctx, ctx->reg_rank, n_slots * 8));
            TRY(ensure(ctx, ctx->hist, std::max((size_t)count * std::max<size_t>(optimise ? max_radius : 0, 1024), (size_t)65536 + 8192) * 4 + 8192 * 4 + 64));
        }
        if (mixed) for (int i = 0; i < count; ++i) {                // every item's own geometry, for every launch of the call
            if (state[i] != BATCH) continue;
            szh_ompb_geo &e = tab.geo[i];
            e.g = sh[i].g; e.G = szh_make_geom3((int)sh[i].r0, (int)sh[i].r1, (int)sh[i].r2); e.nrows = szh_sample_row_limit(e.G, prm->sample_distance);
            e.per_wg = omp_hist_per_wg(e.g.bel); e.fw = 0;
        }
        return choose_intervals();
    }
    void fill_static() {
        for (int i = 0; i < count; ++i) {
            szh_ompb_rec &r = tab.rec[i];
            const T ebT = (T)items[i].eb;
            r.data = src[i]; r.eb = (double)ebT; r.recip = (double)(T)(1 / ebT);
            r.codes = (uint16_t *)ctx->codes_nat.p + o_code[i];
            r.ucount = (unsigned *)ctx->zcnt.p + o_box[i]; r.ucount64 = (u64 *)ctx->col_zeros64.p + o_box[i]; r.first = (T *)ctx->samples.p + o_box[i];
            r.box_bytes = (u64 *)ctx->reg_flags.p + o_box[i]; r.box_off = (u64 *)ctx->reg_rank.p + o_box[i]; r.uoff = (u64 *)ctx->col_off.p + o_box[i];
            r.totals = tab.totals(i);
        }
    }
    int choose_intervals() {
        iv.assign((size_t)count, prm->quantization_intervals);
        HIPCHK(hipEventRecord(ctx->ev[0], st));
        if (shared && optimise) {
            const szh_geom3 G = mixed ? szh_make_geom3(1, 1, 1) : szh_make_geom3((int)r0, (int)r1, (int)r2);
            int64_t nrows = mixed ? 0 : szh_sample_row_limit(G, prm->sample_distance);      // (different shapes: the longest item's, which sizes the grid)
            TRY(ensure_pinned(ctx, (size_t)count * max_radius * 4 + 64));
            HIPCHK(hipMemsetAsync(d_hist(), 0, (size_t)count * max_radius * 4, st));
            TRY(tab.clear_totals());
            fill_static();
            for (int i = 0; i < count; ++i) {
                tab.rec[i].radius_hist = d_hist() + (size_t)i * max_radius;
                if (state[i] != BATCH) continue;
                tab.list[OMPB_L_ALL].push_back(i);
                if (mixed) nrows = std::max(nrows, tab.geo[i].nrows);
            }
            const int n_all = (int)tab.list[OMPB_L_ALL].size();
            TRY(tab.upload(0, {}));
            if (nrows > 0) {
                const int grid = (int)std::min<int64_t>((nrows + 255) / 256, 1024);
                if (mixed) hipLaunchKernelGGL((k_ompbs_sample<T>), dim3((unsigned)grid, (unsigned)n_all), dim3(256), 0, st, tab.d_rec(), tab.d_geo(), tab.d_list(OMPB_L_ALL), prm->sample_distance,
                                              max_radius);
                else if (view) hipLaunchKernelGGL((k_ompb_sample_view<T>), dim3((unsigned)grid, (unsigned)count), dim3(256), 0, st, G, tab.d_rec(), tab.d_list(OMPB_L_ALL), (int64_t)pitch0, (int64_t)pitch1, nrows,
                                             prm->sample_distance, max_radius);         // (every view where it lies: the gather comes behind the single calls, which use its buffer)
                else hipLaunchKernelGGL((k_ompb_sample<T>), dim3((unsigned)grid, (unsigned)count), dim3(256), 0, st, G, tab.d_rec(), tab.d_list(OMPB_L_ALL), nrows, prm->sample_distance, max_radius);
                HIPCHK(hipGetLastError());
            }
            const unsigned *h_rh = (const unsigned *)ctx->pinned;
            HIPCHK(hipMemcpyAsync(ctx->pinned, d_hist(), (size_t)count * max_radius * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            const double h0 = now_ms();
            for (int i = 0; i < count; ++i) if (state[i] == BATCH) iv[i] = pick_intervals(h_rh + (size_t)i * max_radius, max_radius, prm->pred_threshold, 32u);
            host_ms += now_ms() - h0;
        }
        HIPCHK(hipEventRecord(ctx->ev[1], st));
        if (shared && optimise) { HIPCHK(hipEventSynchronize(ctx->ev[1])); float ms = 0; hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); S.ms_prequant = ms; }
        return SZHIP_OK;
    }
    // ---- who stays in the shared launches (box_hist of the single call), in which sweep form; the others run now, while nothing of the batch is on the device yet
    int sort_items() {
        for (int i = 0; i < count; ++i) {
            if (state[i] == BATCH && (iv[i] > 65536 || iv[i] < 4)) {
                state[i] = FAILED; items[i].rc = SZHIP_ERR_UNSUP;
                snprintf(ctx->err, sizeof(ctx->err), "quantization interval count %u outside [4,65536]", iv[i]);
            }
            const size_t nb = sh[i].nb;
            if (state[i] == BATCH && !omp_box_hist_book(iv[i], nb)) state[i] = EARLY;      // (more than 1024 intervals among them)
            if (state[i] == EARLY) { single(i); continue; }
            if (state[i] != BATCH) continue;
            const int form = gathered[i] ? 3 : omp_form(mixed ? sh[i].g : gv, d_in[i], sizeof(T), p0(i), p1(i));      // (a gathered view: the column form in its contiguous, aligned copy)
            items[i].intervals = iv[i]; items[i].quant_kernel = form; items[i].batched = 1;
            tab.list[ompb_form_list(gathered[i] != 0, form)].push_back(i);
            tab.list[OMPB_L_ENT].push_back(i);
            const int rshift = omp_hist_rshift(iv[i], sh[i].g.bel);
            szh_ompb_rec &r = tab.rec[i];
            r.intervals = iv[i]; r.rshift = rshift; r.count_in_hist = form == 3 ? 1 : 0;
            hist_lds = std::max(hist_lds, ((size_t)iv[i] << rshift) * 4);
            o_hb[i] = hb_bytes; hb_bytes += nb * iv[i] * 4;
        }
        n_ent = (int)tab.list[OMPB_L_ENT].size();
        if (mixed) { box_runs[0] = ompb_box_runs(tab.list[OMPB_L_F4], sh); box_runs[1] = ompb_box_runs(tab.list[OMPB_L_F5], sh); }
        hdr.resize((size_t)count); packed.resize((size_t)count);
        E.assign((size_t)count, 0); total_bits = E; off_pay.assign((size_t)count, 0); cap_len = off_pay;
        return SZHIP_OK;
    }
    // ---- 3. the gather of the views, the sweeps: one launch per form
    int sweep_and_books() {
        if (n_ent == 0) return SZHIP_OK;
        TRY(ensure(ctx, ctx->chunk_bits, hb_bytes));
        TRY(tab.clear_totals());
        HIPCHK(hipMemsetAsync(d_hist(), 0, (size_t)count * 1024 * 4, st));
        // the gathered views: their contiguous copies one behind the other in the context's input buffer (the single calls of sort_items are through with it), the pairs
        // {view, copy} behind the lists of the table
        const int n3g = (int)tab.list[OMPB_L_F3G].size();
        std::vector<unsigned char> pairs;
        if (n3g) {
            const size_t stride = up16(r0 * r1 * r2 * sizeof(T));
            TRY(ensure(ctx, ctx->in, (size_t)n3g * stride));
            pairs.resize((size_t)n3g * 16);
            u64 *pp = (u64 *)pairs.data();
            for (int k = 0; k < n3g; ++k) {
                const int i = tab.list[OMPB_L_F3G][k];
                src[i] = (const T *)((const char *)ctx->in.p + (size_t)k * stride);
                pp[2 * k] = (u64)(uintptr_t)d_in[i]; pp[2 * k + 1] = (u64)(uintptr_t)src[i];
            }
        }
        fill_static();
        for (int i : tab.list[OMPB_L_ENT]) { tab.rec[i].hist_box = (unsigned *)((char *)ctx->chunk_bits.p + o_hb[i]); tab.rec[i].hist = d_hist() + (size_t)i * 1024; }
        TRY(tab.upload(1, pairs));
        if (n3g) {                                               // ONE gather launch for all of them
            const int cpr = (int)((r2 + 16 / sizeof(T) - 1) / (16 / sizeof(T)));
            const int64_t total = (int64_t)(r0 * r1) * cpr;
            hipLaunchKernelGGL((k_ompb_crop<T>), dim3((unsigned)((total + 255) / 256), (unsigned)n3g), dim3(256), 0, st, (const u64 *)(tab.dev() + tab.o_extra), (int64_t)pitch0, (int64_t)pitch1,
                               (int)r1, (int)r2, cpr, total);
            HIPCHK(hipGetLastError());
            ++S.packing;                                         // (counted where it is launched)
        }
        HIPCHK(hipEventRecord(ctx->ev[2], st));
        S.quant_kernel_launches += mixed ? ompb_sweep_mixed<T, false>(st, tab, sh, box_runs) : ompb_sweep_same<T, false>(st, tab, g, gv, 0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[3], st));
        S.quant_kernel = items[tab.list[OMPB_L_ENT][0]].quant_kernel;
        // 4. the boxes' histograms and every array's own: one launch, one read-back.  5. the books, the headers (hist_and_book of the single call, per array)
        if (mixed) {
            int gx = 1;
            for (int i : tab.list[OMPB_L_ENT]) gx = std::max(gx, ((int)sh[i].nb + tab.geo[i].per_wg - 1) / tab.geo[i].per_wg);
            hipLaunchKernelGGL(k_ompbs_hist_box, dim3((unsigned)gx, (unsigned)n_ent), dim3(256), hist_lds, st, tab.d_rec(), tab.d_geo(), tab.d_list(OMPB_L_ENT));
        } else {
            const size_t nb = (size_t)g.nb;
            const int hist_per_wg = omp_hist_per_wg(g.bel);
            hipLaunchKernelGGL(k_ompb_hist_box, dim3((unsigned)((nb + hist_per_wg - 1) / hist_per_wg), (unsigned)n_ent), dim3(256), hist_lds, st, g.bel, tab.d_rec(), tab.d_list(OMPB_L_ENT),
                               (int)nb, hist_per_wg);
        }
        HIPCHK(hipGetLastError());
        TRY(ensure_pinned(ctx, (size_t)count * 1024 * 4 + 64));
        HIPCHK(hipMemcpyAsync(ctx->pinned, d_hist(), (size_t)count * 1024 * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const double h0 = now_ms();
        const unsigned *h_hist = (const unsigned *)ctx->pinned;
        for (int i : tab.list[OMPB_L_ENT]) {
            std::vector<u64> tab_code; std::vector<uint8_t> tab_len; unsigned maxlen = 0;
            const unsigned *hh = h_hist + (size_t)i * 1024;
            E[i] = hh[0]; items[i].n_unpred = E[i];
            const huff_ptr hf = host_book(hh, iv[i], tab_code, tab_len, &maxlen);
            if (!hf) { state[i] = FAILED; items[i].rc = SZHIP_ERR_INTERNAL; snprintf(ctx->err, sizeof(ctx->err), "Huffman build failed"); continue; }
            const size_t tree_bytes = szhost_huff_tree_size(hf.get());
            total_bits[i] = hf->total_bits;
            const size_t nb = sh[i].nb;
            const omp_layout<T> L(meta_len, nb, E[i], tree_bytes, total_bits[i]);
            szh_ompb_rec &r = tab.rec[i];
            r.hdr_len = (unsigned)L.hdr_len; r.maxlen = (int)maxlen;
            r.off_ucount = L.off_ucount; r.off_first = L.off_first; r.off_unpred = L.off_unpred; r.off_sizes = L.off_sizes; r.off_pay = L.off_pay;
            off_pay[i] = L.off_pay; cap_len[i] = L.cap_len;
            const size_t lds3 = omp_fast_lds3(iv[i], maxlen);
            if (!omp_fast_packs(maxlen, lds3)) { state[i] = LATE; items[i].batched = 0; continue; }      // (pack_general: the single call, once the batch is through)
            lds3_max = std::max(lds3_max, lds3);
            hdr[i].assign(L.hdr_len, 0);
            omp_write_header<T>(hdr[i].data(), (const unsigned char *)items[i].meta, meta_len, nb, (T)items[i].eb, iv[i], hf.get(), tree_bytes);
            packed[i].resize(iv[i]);
            omp_packed_table(tab_code, tab_len, iv[i], packed[i].data());
            tab.list[OMPB_L_PACK].push_back(i);
            tab.list[gathered[i] ? OMPB_L_PACKG : OMPB_L_PACKD].push_back(i);      // (the encoder reads the verbatim values through the geometry)
        }
        host_ms += now_ms() - h0;
        return SZHIP_OK;
    }
    // ---- the blob: every stream at a multiple of 64, in item order.  A stream of the shared launches and one that is still to come take their bound (+ 64: the
    // packers' last words), a finished one its length
    int pack() {
        for (int i = 0; i < count; ++i) {
            items[i].offset = pos;
            const size_t slot = state[i] == EARLY ? fb[i].size() : state[i] == FAILED ? 0 : cap_len[i] + 64;
            pos = up64(pos + slot);
        }
        TRY(ensure(ctx, ctx->batch_blob, pos + 64));
        d_blob = (unsigned char *)ctx->batch_blob.p;
        n_pack = (int)tab.list[OMPB_L_PACK].size();
        if (n_pack == 0) { HIPCHK(hipStreamSynchronize(st)); return SZHIP_OK; }
        // 6. one upload: the table again, with every header and packed code table and the spans of the verbatim values behind it.  7. / 8. every box its size and place
        // inside its own stream; every stream's tables and payloads
        size_t un_bytes = 0, ex = 0;
        std::vector<size_t> o_un((size_t)count, 0), o_hdr((size_t)count, 0);
        int n_spans = 0;
        for (int i : tab.list[OMPB_L_PACK]) {
            o_un[i] = un_bytes; un_bytes += up16((size_t)E[i] * sizeof(T));
            o_hdr[i] = ex; ex += (hdr[i].size() + 7) / 8 * 8 + (size_t)iv[i] * 8;
            if (E[i] > 0) ++n_spans;
        }
        const size_t o_spans = ex;
        ex += (size_t)n_spans * 24;
        TRY(ensure(ctx, ctx->unpred, un_bytes + 16));
        TRY(tab.reserve(ex));
        fill_static();
        std::vector<unsigned char> extra(ex, 0);
        u64 *sp = (u64 *)(extra.data() + o_spans);
        for (int i : tab.list[OMPB_L_PACK]) {
            szh_ompb_rec &r = tab.rec[i];
            const size_t hdr_pad = (hdr[i].size() + 7) / 8 * 8;
            memcpy(extra.data() + o_hdr[i], hdr[i].data(), hdr[i].size());
            memcpy(extra.data() + o_hdr[i] + hdr_pad, packed[i].data(), (size_t)iv[i] * 8);
            r.hdr = tab.dev() + tab.o_extra + o_hdr[i]; r.packed = (const u64 *)(r.hdr + hdr_pad);
            r.stream = d_blob + items[i].offset;
            r.unpred = (char *)ctx->unpred.p + o_un[i];
            if (E[i] > 0) { *sp++ = (u64)(uintptr_t)r.unpred; *sp++ = (u64)(items[i].offset + r.off_unpred); *sp++ = (u64)E[i] * sizeof(T); }
        }
        TRY(tab.clear_totals());
        HIPCHK(hipMemsetAsync(d_blob, 0, pos + 64, st));
        TRY(tab.upload(2, extra));
        const int n_packd = (int)tab.list[OMPB_L_PACKD].size(), n_packg = (int)tab.list[OMPB_L_PACKG].size();
        if (mixed) {
            hipLaunchKernelGGL(k_ompbs_layout, dim3(1, (unsigned)n_pack), dim3(1024), 0, st, tab.d_rec(), tab.d_geo(), tab.d_list(OMPB_L_PACK));
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL((k_ompbs_encode_box3<T>), dim3((unsigned)ompb_most_boxes(tab.list[OMPB_L_PACKD], 0, n_packd, sh), (unsigned)n_packd), dim3(256), lds3_max, st, tab.d_rec(),
                               tab.d_geo(), tab.d_list(OMPB_L_PACKD));
        } else {
            const size_t nb = (size_t)g.nb;
            hipLaunchKernelGGL(k_ompb_layout, dim3(1, (unsigned)n_pack), dim3(1024), 0, st, (int)nb, tab.d_rec(), tab.d_list(OMPB_L_PACK));
            HIPCHK(hipGetLastError());
            if (n_packd) hipLaunchKernelGGL((k_ompb_encode_box3<T>), dim3((unsigned)nb, (unsigned)n_packd), dim3(256), lds3_max, st, gv, tab.d_rec(), tab.d_list(OMPB_L_PACKD));
            if (n_packg) hipLaunchKernelGGL((k_ompb_encode_box3<T>), dim3((unsigned)nb, (unsigned)n_packg), dim3(256), lds3_max, st, g, tab.d_rec(), tab.d_list(OMPB_L_PACKG));
        }
        HIPCHK(hipGetLastError());
        if (n_spans) {
            hipLaunchKernelGGL(k_ompb_fetch, dim3((unsigned)n_spans), dim3(256), 0, st, d_blob, (const u64 *)(tab.dev() + tab.o_extra + o_spans));
            HIPCHK(hipGetLastError());
        }
        // 9. the arrays' totals: the device's counts against the books' (check_and_deliver of the single call, per array)
        HIPCHK(hipEventRecord(ctx->ev[4], st));
        TRY(ensure_pinned(ctx, (size_t)count * 32));
        HIPCHK(hipMemcpyAsync(ctx->pinned, tab.dev(), (size_t)count * 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const u64 *h_tot = (const u64 *)ctx->pinned;
        float ms = 0;
        hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]); S.ms_quant = ms;
        hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]); S.ms_entropy = ms;
        for (int i : tab.list[OMPB_L_PACK]) {
            const u64 *t = h_tot + 4 * (size_t)i;
            // (the payloads against their bound: a failure with its own text in the single call, the same one here)
            if (!omp_totals_ok(t[1], t[2], t[0], E[i], total_bits[i], sh[i].nb) || off_pay[i] + (size_t)t[0] > cap_len[i]) {
                state[i] = FAILED; items[i].rc = SZHIP_ERR_INTERNAL;
                snprintf(ctx->err, sizeof(ctx->err), "OpenMP container: entropy stage mismatch in array %d of the batch", i);
                continue;
            }
            items[i].size = off_pay[i] + (size_t)t[0];
        }
        return SZHIP_OK;
    }
    // ---- the single calls that had to wait; the blob to the caller; the streams of the single calls into their places
    int deliver(unsigned char **blob, size_t *blob_size, szhip_stats *stats) {
        for (int i = 0; i < count; ++i) if (state[i] == LATE) single(i);
        unsigned char *h_blob = nullptr;
        if (!out_on_device) {
            h_blob = (unsigned char *)malloc(pos ? pos : 1);
            if (!h_blob) FAIL(SZHIP_ERR_INTERNAL, "out of host memory");
            if (n_pack > 0) { const int rc = staged_copy(ctx, h_blob, d_blob, pos, false); if (rc != SZHIP_OK) { free(h_blob); return rc; } }
        }
        bool copied = false;
        for (int i = 0; i < count; ++i) {
            if ((state[i] != EARLY && state[i] != LATE) || items[i].rc != SZHIP_OK) continue;
            if (state[i] == LATE && fb[i].size() > cap_len[i] + 64) { items[i].rc = SZHIP_ERR_INTERNAL; continue; }      // (the single call packs the same book: never)
            items[i].size = fb[i].size();
            if (h_blob) memcpy(h_blob + items[i].offset, fb[i].data(), fb[i].size());
            else { HIPCHK(hipMemcpyAsync(d_blob + items[i].offset, fb[i].data(), fb[i].size(), hipMemcpyHostToDevice, st)); copied = true; }
        }
        if (copied) HIPCHK(hipStreamSynchronize(st));
        *blob = h_blob ? h_blob : d_blob; *blob_size = pos;
        int rc_all = SZHIP_OK;                                  // the first failed item's code; the statistics
        for (int i = 0; i < count; ++i) {
            if (items[i].rc != SZHIP_OK) { items[i].size = 0; if (rc_all == SZHIP_OK) rc_all = items[i].rc; continue; }
            S.n_unpred += items[i].n_unpred; S.out_bytes += items[i].size;
        }
        S.ms_host = host_ms; S.ms_total = now_ms() - t_begin;
        if (stats) *stats = S;
        return rc_all;
    }
};

template <class T>
int compress_omp_batch_impl(szhip_ctx *ctx, szhip_batch_item *items, int count, int data_on_device, const szhip_batch_shape *shapes, size_t r0, size_t r1, size_t r2,
                            size_t pitch0, size_t pitch1, int thread_num, const szhip_params *prm, size_t meta_len, int out_on_device, unsigned char **blob, size_t *blob_size,
                            szhip_stats *stats)
{
    const bool mixed = shapes != nullptr;
    if (mixed) r0 = r1 = r2 = pitch0 = pitch1 = 0;
    ompb_enc<T> c{call_base(ctx), items, count, data_on_device, mixed, r0, r1, r2, pitch0, pitch1, thread_num, prm, meta_len, out_on_device};
    TRY(c.inputs(shapes));
    TRY(c.prepare());
    TRY(c.sort_items());
    TRY(c.sweep_and_books());
    TRY(c.pack());
    return c.deliver(blob, blob_size, stats);
}
// ---- the inverse.  What read_header of the single call finds in a stream is here per stream: omp_stream<T> (szhip_omprules.inc).
// Pieces of the callers' device streams to the host, one round for all streams of a batch: the spans go up, one k_ompb_fetch into the context's staging array, one copy
// down.  want[u]: bytes of stream u the host needs (0: none -- the stream has failed or left the batch); what it has already is not fetched again.
template <class T>
int batch_fetch(szhip_ctx *ctx, hipStream_t st, std::vector<omp_stream<T>> &ps, const std::vector<size_t> &want)
{
    std::vector<u64> spans;
    std::vector<size_t> at(ps.size(), 0);
    size_t bytes = 0;
    for (size_t u = 0; u < ps.size(); ++u) {
        if (want[u] <= ps[u].have) continue;
        at[u] = bytes;
        spans.push_back((u64)(uintptr_t)(ps[u].src + ps[u].have)); spans.push_back((u64)bytes); spans.push_back((u64)(want[u] - ps[u].have));
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
    for (size_t u = 0; u < ps.size(); ++u) {
        if (want[u] <= ps[u].have) continue;
        ps[u].hbuf.resize(want[u]);
        memcpy(ps[u].hbuf.data() + ps[u].have, (const unsigned char *)ctx->pinned + at[u], want[u] - ps[u].have);
        ps[u].have = want[u];
    }
    return SZHIP_OK;
}
// a stream of a decode call: in the shared launches, through the single call, refused
enum { OMPB_BATCH, OMPB_SINGLE, OMPB_FAILED };
// the grid of a stream's own thread_num on its own shape into `s`, if there is one
static bool ompb_own_grid(szhip_ctx *ctx, int thread_num, ompb_shape &s)
{
    szh_omp_geom gi;
    if (!(thread_num >= 1 && omp_box_grid(ctx, thread_num, s.r0, s.r1, s.r2, &gi) == SZHIP_OK && gi.nb == thread_num)) return false;
    s.g = gi; s.nb = (size_t)gi.nb; s.thread_num = thread_num;
    return true;
}
// Headers, trees and per-box tables of a batch's streams (after omp_stream::begin): three rounds of fetches at most, the steps of omp_stream per stream.  `grid(u)`: the
// call's rule for the box grid of stream u, whose fixed fields have been read -- it fills sh[u]; without a grid (sh[u].nb == 0) the stream goes to the single call, which
// says what is wrong with it.  `fail(u, why)`: the stream is refused.
template <class T, class GRID, class FAIL>
int batch_read_fronts(szhip_ctx *ctx, hipStream_t st, bool on_device, std::vector<omp_stream<T>> &ps, std::vector<ompb_shape> &sh, std::vector<int> &state, GRID &&grid, FAIL &&fail)
{
    const int count = (int)ps.size();
    auto fetch_round = [&](const std::vector<size_t> &want) { return on_device ? batch_fetch<T>(ctx, st, ps, want) : SZHIP_OK; };
    std::vector<size_t> want((size_t)count, 0);
    const char *why;
    for (int u = 0; u < count; ++u) if (state[u] == OMPB_BATCH) want[u] = ps[u].fixed;
    TRY(fetch_round(want));
    for (int u = 0; u < count; ++u) {
        want[u] = 0;
        if (state[u] != OMPB_BATCH) continue;
        omp_stream<T> &p = ps[u];
        if ((why = p.read_fixed(p.hs(on_device)))) { fail(u, why); continue; }
        grid(u);
        if (sh[u].nb == 0) { state[u] = OMPB_SINGLE; continue; }
        if ((why = p.place_tables(sh[u].g))) { fail(u, why); continue; }
        want[u] = p.off_unpred;
    }
    TRY(fetch_round(want));
    for (int u = 0; u < count; ++u) {
        want[u] = 0;
        if (state[u] != OMPB_BATCH) continue;
        if ((why = ps[u].read_tree_and_counts(ps[u].hs(on_device), sh[u].g))) { fail(u, why); continue; }
        want[u] = ps[u].off_pay;
    }
    if (on_device)                                             // (the third round wants the box sizes only: not the verbatim values in front of them)
        for (int u = 0; u < count; ++u) if (state[u] == OMPB_BATCH) { ps[u].hbuf.resize(ps[u].off_sizes); ps[u].have = ps[u].off_sizes; }
    TRY(fetch_round(want));
    for (int u = 0; u < count; ++u) {
        if (state[u] != OMPB_BATCH) continue;
        omp_stream<T> &p = ps[u];
        memcpy(p.size_table(sh[u].g), p.hs(on_device) + p.off_sizes, sh[u].nb * 8);
        if ((why = p.walk_sizes())) fail(u, why);
    }
    return SZHIP_OK;
}
// the error counts of a decode call's items to the host (*h_tot: 4 u64 per item), synchronised; the device times of the call
static int ompb_read_totals(call_base &c, const ompb_table &tab, const u64 **h_tot)
{
    szhip_ctx *const ctx = c.ctx;
    TRY(ensure_pinned(ctx, (size_t)tab.count * 32));
    HIPCHK(hipMemcpyAsync(ctx->pinned, tab.dev(), (size_t)tab.count * 32, hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipStreamSynchronize(c.st));
    *h_tot = (const u64 *)ctx->pinned;
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); c.S.ms_entropy = ms;
    hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]); c.S.ms_quant = ms;
    return SZHIP_OK;
}
// pitch0 / pitch1: the element pitches of the arrays the items' sub-boxes lie in (szhip_decompress_omp_batch_view; r1 * r2 and r2: contiguous arrays).  The mirror of the
// compress call: a device view is written where it lies through the pitched geometry, or (omp_view_packs) decoded contiguous in the context's output buffer and placed
// by ONE k_ompb_view_scatter launch for all such items -- those whose boxes all decoded.  A host view is decoded contiguous and its rows are copied out.
// (different shapes: a stream is batched when the grid of ITS thread_num divides ITS shape; one shape: the first such stream's box count is the batch's)
// One batch decode call: its state, and one member function per step (decompress_omp_batch_impl is their sequence).  What the steps rely on:
//  - Context buffers.  stream_buf holds every stream of the call from read_fronts on (the payloads are decoded out of it); seg_hist and the pinned block serve its fetch
//    rounds alone.  fill_table sizes out, batch_rec, codes_nat, unpred and chunk_bits ONCE, before the records that point into them are filled.  The single calls use
//    stream_buf, out, codes_nat and unpred themselves: they run in finish(), after launches() has read back what the shared launches left and scattered the gathered views.
//  - The table is reserved once; records are filled after that reserve, so no address in them moves (the compress call reserves twice and repeats fill_static()).
//  - `tab` is a member: its image[version] vectors, the pageable sources of the asynchronous uploads, outlive every upload; launches() ends synchronised.
template <class T>
struct ompb_dec : call_base {
    szhip_batch_item *const items; const int count, stream_on_device; const bool mixed; const size_t r0, r1, r2; const int out_on_device; const size_t pitch0, pitch1;
    const size_t n = r0 * r1 * r2; const bool any_view = pitch1 != r2 || pitch0 != r1 * r2, view = any_view && out_on_device;      // (`n`: one shape)
    std::vector<ompb_shape> sh; std::vector<int> state; std::vector<omp_stream<T>> ps;
    szh_omp_geom g, gv; bool have_g = false; int batch_threads = 0, fw = 0;      // one shape: the batch's grid (`gv`: of the items that are written where they lie), its flag words
    hdec_launch hl; unsigned char *d_streams = nullptr;
    ompb_table tab{ctx, count, mixed};
    // where item i's work arrays lie: its decoded copy (a host array, a gathered view), codes, first values, flag words -- behind those of the items before it, each
    // at the alignment the single call gives it (a stream of the single call in front takes its places too: an odd length there shifts nobody off a boundary)
    std::vector<size_t> o_out, o_code, o_first, o_flag, o_ex, o_un;
    std::vector<int> fws; std::vector<char> gathered; bool any_gathered = false, any_flags = false;
    size_t ex = 0, un_bytes = 0, sum_n = 0, first_bytes = 0, o_spans = 0, o_pairs = 0;
    int n_ent = 0, n_spans = 0; std::vector<unsigned char> extra;
    void fail(int i, const char *why) { state[i] = OMPB_FAILED; items[i].rc = SZHIP_ERR_STREAM; snprintf(ctx->err, sizeof(ctx->err), "stream %d of the batch: %s", i, why); }
    // ---- the streams into the context's buffer, each where its address modulo 16 puts it, 64 zero bytes behind each (the bit readers may look past an end)
    int read_fronts(const szhip_batch_shape *shapes) {
        sh.resize((size_t)count); state.assign((size_t)count, OMPB_BATCH); ps.resize((size_t)count);
        memset(&g, 0, sizeof(g));
        for (int i = 0; i < count; ++i) sh[i] = mixed ? ompb_shape_of(shapes[i].r0, shapes[i].r1, shapes[i].r2) : ompb_shape_of(r0, r1, r2);
        size_t total = 0;
        for (int i = 0; i < count; ++i) {
            total = up16(total) + ((uintptr_t)items[i].stream & 15u);
            ps[i].pos = total; total += items[i].stream_len + 64;
        }
        TRY(ensure(ctx, ctx->stream_buf, total + 64));
        d_streams = (unsigned char *)ctx->stream_buf.p;
        TRY(ensure(ctx, ctx->batch_rec, 64));
        HIPCHK(hipMemsetAsync(d_streams, 0, total + 64, st));
        if (stream_on_device) {
            std::vector<u64> all;
            for (int i = 0; i < count; ++i) { all.push_back((u64)(uintptr_t)items[i].stream); all.push_back((u64)ps[i].pos); all.push_back((u64)items[i].stream_len); }
            TRY(ensure(ctx, ctx->seg_zoff, all.size() * 8));
            HIPCHK(hipMemcpyAsync(ctx->seg_zoff.p, all.data(), all.size() * 8, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_ompb_fetch, dim3((unsigned)count), dim3(256), 0, st, d_streams, (const u64 *)ctx->seg_zoff.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));                        // (`all` is a pageable source)
        } else if (total <= ((size_t)64 << 20)) {
            TRY(ensure_pinned3(ctx, total + 64));
            memset(ctx->pinned3, 0, total);
            for (int i = 0; i < count; ++i) memcpy((unsigned char *)ctx->pinned3 + ps[i].pos, items[i].stream, items[i].stream_len);
            HIPCHK(hipMemcpyAsync(d_streams, ctx->pinned3, total, hipMemcpyHostToDevice, st));
        } else for (int i = 0; i < count; ++i) TRY(staged_copy(ctx, d_streams + ps[i].pos, items[i].stream, items[i].stream_len, true));
        HIPCHK(hipEventRecord(ctx->ev[0], st));
        // 1. / 2. headers, trees and per-box tables of all streams; who the look-up-table decoder takes
        const double h0 = now_ms();
        for (int i = 0; i < count; ++i) {
            ps[i].src = items[i].stream;
            if (const char *why = ps[i].begin(items[i].body_off, items[i].stream_len)) fail(i, why);
        }
        // different shapes: every stream's own grid; one shape: the first stream's that divides it, and every stream with that thread_num
        auto grid = [&](int i) {
            const int tn = ps[i].thread_num;
            if ((mixed || !have_g) && ompb_own_grid(ctx, tn, sh[i]) && !have_g) { g = sh[i].g; have_g = true; batch_threads = tn; }
            if (!mixed && have_g && tn == batch_threads) { sh[i].g = g; sh[i].nb = (size_t)g.nb; sh[i].thread_num = batch_threads; }
        };
        TRY(batch_read_fronts<T>(ctx, st, stream_on_device != 0, ps, sh, state, grid, [&](int i, const char *why) { fail(i, why); }));
        for (int i = 0; i < count; ++i) {
            if (state[i] != OMPB_BATCH) continue;
            const hdec_fit fit = hdec_lut_fit(ps[i].max_box, ps[i].D.n_nodes, ps[i].D.single_symbol, sh[i].g.bel);      // (for this stream alone)
            if (!fit.takes) { state[i] = OMPB_SINGLE; continue; }
            hl.add(fit);
        }
        hl.close();
        if (hl.lds_lut > HDEC_LDS_MAX) for (int i = 0; i < count; ++i) if (state[i] == OMPB_BATCH) state[i] = OMPB_SINGLE;
        host_ms += now_ms() - h0;
        return SZHIP_OK;
    }
    // ---- the arrays of the shared launches: their places, buffers and records
    int fill_table() {
        o_out.assign((size_t)count + 1, 0); o_code = o_out; o_first = o_out; o_flag = o_out;
        o_ex.assign((size_t)count, 0); o_un = o_ex; fws.assign((size_t)count, 0); gathered.assign((size_t)count, 0);
        for (int i = 0; i < count; ++i) {
            if (sh[i].nb) fws[i] = omp_flag_words<T>(sh[i].g);
            o_out[i + 1] = o_out[i] + up16(sh[i].n * sizeof(T)); o_code[i + 1] = o_code[i] + (sh[i].n + 7) / 8 * 8;
            o_first[i + 1] = o_first[i] + up16(sh[i].nb * sizeof(T)); o_flag[i + 1] = o_flag[i] + sh[i].nb * (size_t)fws[i];
        }
        gv = g;
        if (view && have_g) {
            omp_view_pitches(&gv, pitch0, pitch1, sizeof(T));
            for (int i = 0; i < count; ++i) if (state[i] == OMPB_BATCH && omp_view_packs(g, items[i].out, pitch0, pitch1, sizeof(T))) { gathered[i] = 1; any_gathered = true; }
        }
        if (!out_on_device || any_gathered) TRY(ensure(ctx, ctx->out, o_out[count]));
        size_t sum_nb = 0;                                      // (one shape: every stream counts with the batch's box count, as before)
        for (int i = 0; i < count; ++i) { sum_n += sh[i].n; sum_nb += mixed ? sh[i].nb : have_g ? (size_t)g.nb : 0; }
        fw = have_g && !mixed ? omp_flag_words<T>(g) : 0;
        if (have_g) TRY(ompb_limits(ctx, count, sum_nb, sum_n));
        first_bytes = o_first[count];
        for (int i = 0; i < count; ++i) {
            if (state[i] != OMPB_BATCH) continue;
            omp_stream<T> &p = ps[i];
            const size_t nb = sh[i].nb;
            tab.list[OMPB_L_ENT].push_back(i);
            o_ex[i] = ex;
            ex += up64(p.D.dtab.size() * 4) + SZH_LUT_BYTES + 64 + up16(nb * 8) * 2 + up16((nb + 1) * 8);
            o_un[i] = first_bytes + un_bytes; un_bytes += up16((size_t)p.E * sizeof(T));
            S.n_unpred += p.E; items[i].intervals = p.intervals; items[i].n_unpred = p.E; items[i].batched = 1;
            if (mixed) { tab.geo[i].g = sh[i].g; tab.geo[i].fw = fws[i]; }
        }
        n_ent = (int)tab.list[OMPB_L_ENT].size();
        S.n_elements = (uint64_t)sum_n; S.n_blocks = (uint64_t)sum_nb;
        if (n_ent == 0) return SZHIP_OK;
        // the buffers, every item's record and sweep form
        o_spans = ex;
        ex += (size_t)n_ent * 2 * 24;
        o_pairs = ex;                                           // (the pairs {view, contiguous copy} of the final scatter: uploaded when it is known which items decoded)
        if (any_gathered) ex += (size_t)count * 16;
        TRY(tab.reserve(ex));
        TRY(ensure(ctx, ctx->codes_nat, o_code[count] * 2 + 64));
        TRY(ensure(ctx, ctx->unpred, first_bytes + un_bytes + 16));
        if (o_flag[count] > 0) TRY(ensure(ctx, ctx->chunk_bits, o_flag[count] * 4));
        extra.assign(ex, 0);
        u64 *sp = (u64 *)(extra.data() + o_spans);
        unsigned char *d_un = (unsigned char *)ctx->unpred.p;
        for (int i : tab.list[OMPB_L_ENT]) {
            omp_stream<T> &p = ps[i];
            szh_ompb_rec &r = tab.rec[i];
            const size_t nb = sh[i].nb;
            unsigned char *dx = tab.dev() + tab.o_extra + o_ex[i], *hx = extra.data() + o_ex[i];
            size_t o = 0;
            memcpy(hx, p.D.dtab.data(), p.D.dtab.size() * 4); r.table = (const unsigned *)dx; o = up64(p.D.dtab.size() * 4);
            r.lut = (uint4 *)(dx + o); o += SZH_LUT_BYTES + 64;
            memcpy(hx + o, p.bbytes.data(), nb * 8); r.box_bytes = (u64 *)(dx + o); o += up16(nb * 8);
            memcpy(hx + o, p.boff.data(), nb * 8); r.box_off = (u64 *)(dx + o); o += up16(nb * 8);
            memcpy(hx + o, p.uoff.data(), (nb + 1) * 8); r.uoff = (u64 *)(dx + o);
            r.out = out_on_device && !gathered[i] ? items[i].out : (void *)((char *)ctx->out.p + o_out[i]);
            r.eb = (double)p.eb; r.recip = (double)(T)(1 / p.eb); r.intervals = p.intervals;
            r.codes = (uint16_t *)ctx->codes_nat.p + o_code[i];
            r.first = d_un + o_first[i]; r.unpred = d_un + o_un[i];
            r.totals = tab.totals(i);
            r.payload = d_streams + p.pos + p.off_pay; r.bytes_before = (unsigned)std::min<size_t>(p.pos + p.off_pay, 0x7fffffffu);
            r.n_nodes = p.D.n_nodes; r.tab_lds = hl.tab_lds(p.D.n_nodes);
            const size_t fp0 = view ? pitch0 : sh[i].r1 * sh[i].r2, fp1 = view ? pitch1 : sh[i].r2;      // (what omp_form looks at)
            const int form = gathered[i] ? 3 : omp_form(mixed ? sh[i].g : gv, r.out, sizeof(T), fp0, fp1);
            items[i].quant_kernel = form;
            tab.list[ompb_form_list(gathered[i] != 0, form)].push_back(i);
            if (form == 3 && p.E > 0) {
                tab.list[gathered[i] ? OMPB_L_PACKG : OMPB_L_PACKD].push_back(i);      // (here: the arrays k_omp_scatter runs for)
                if (fws[i] > 0) { r.vflags = (unsigned *)ctx->chunk_bits.p + o_flag[i]; any_flags = true; }
            }
            // the first values and the verbatim values to aligned addresses (omp_dec::decode_boxes copies them out of the stream one by one)
            *sp++ = (u64)(uintptr_t)(d_streams + p.pos + p.off_first); *sp++ = (u64)o_first[i]; *sp++ = (u64)(nb * sizeof(T)); ++n_spans;
            if (p.E > 0) { *sp++ = (u64)(uintptr_t)(d_streams + p.pos + p.off_unpred); *sp++ = (u64)o_un[i]; *sp++ = (u64)p.E * sizeof(T); ++n_spans; }
        }
        return SZHIP_OK;
    }
    // ---- 3. one upload; 4. / 5. the look-up tables, the Huffman decode; 6. the verbatim values of the column-form arrays to their places, one sweep launch per form
    int launches() {
        if (n_ent == 0) { HIPCHK(hipStreamSynchronize(st)); return SZHIP_OK; }
        TRY(tab.clear_totals());
        if (any_flags) HIPCHK(hipMemsetAsync(ctx->chunk_bits.p, 0, o_flag[count] * 4, st));
        std::vector<int> box_runs[2];                           // different shapes: where the runs of equal boxes end in the lists of forms 4 and 5
        if (mixed) { box_runs[0] = ompb_box_runs(tab.list[OMPB_L_F4], sh); box_runs[1] = ompb_box_runs(tab.list[OMPB_L_F5], sh); }
        TRY(tab.upload(0, extra));
        hipLaunchKernelGGL(k_ompb_fetch, dim3((unsigned)n_spans), dim3(256), 0, st, (unsigned char *)ctx->unpred.p, (const u64 *)(tab.dev() + tab.o_extra + o_spans));
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ompb_build_lut, dim3(SZH_LUT_SIZE / 256, (unsigned)n_ent), dim3(256), 0, st, tab.d_rec(), tab.d_list(OMPB_L_ENT));
        HIPCHK(hipGetLastError());
        const size_t nb = have_g ? (size_t)g.nb : 0;           // (one shape: the batch's box count)
        if (mixed) hipLaunchKernelGGL(k_ompbs_hdec_lut, dim3((unsigned)ompb_most_boxes(tab.list[OMPB_L_ENT], 0, n_ent, sh), (unsigned)n_ent), dim3(256), hl.lds_lut, st, tab.d_rec(), tab.d_geo(),
                                      tab.d_list(OMPB_L_ENT), (unsigned)hl.stage_max);
        else hipLaunchKernelGGL(k_ompb_hdec_lut, dim3((unsigned)nb, (unsigned)n_ent), dim3(256), hl.lds_lut, st, g.bel, tab.d_rec(), tab.d_list(OMPB_L_ENT), (unsigned)hl.stage_max);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[1], st));
        HIPCHK(hipEventRecord(ctx->ev[2], st));
        const int ns = (int)tab.list[OMPB_L_PACKD].size(), nsg = (int)tab.list[OMPB_L_PACKG].size();
        if (mixed) {
            if (ns) hipLaunchKernelGGL((k_ompbs_scatter<T>), dim3((unsigned)ompb_most_boxes(tab.list[OMPB_L_PACKD], 0, ns, sh), (unsigned)ns), dim3(256), 0, st, tab.d_rec(), tab.d_geo(),
                                       tab.d_list(OMPB_L_PACKD));
            S.quant_kernel_launches += ompb_sweep_mixed<T, true>(st, tab, sh, box_runs);
        } else {
            if (ns) hipLaunchKernelGGL((k_ompb_scatter<T>), dim3((unsigned)nb, (unsigned)ns), dim3(256), 0, st, gv, tab.d_rec(), tab.d_list(OMPB_L_PACKD), fw);
            if (nsg) hipLaunchKernelGGL((k_ompb_scatter<T>), dim3((unsigned)nb, (unsigned)nsg), dim3(256), 0, st, g, tab.d_rec(), tab.d_list(OMPB_L_PACKG), fw);
            S.quant_kernel_launches += ompb_sweep_same<T, true>(st, tab, g, gv, fw);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[3], st));
        S.quant_kernel = items[tab.list[OMPB_L_ENT][0]].quant_kernel;
        // 7. the arrays' error counts; the decoded arrays to the callers' host arrays; the gathered views to their places
        const u64 *h_tot = nullptr;
        TRY(ompb_read_totals(*this, tab, &h_tot));
        for (int i : tab.list[OMPB_L_ENT]) if ((unsigned)h_tot[4 * (size_t)i + 2] != 0) fail(i, "boxes whose payload or verbatim-value count does not fit their codes");
        if (!out_on_device) {                                 // one copy down, then those of the streams that decoded
            const host_view hv = {r1, r2 * sizeof(T), pitch0 * sizeof(T), pitch1 * sizeof(T)};
            std::vector<unsigned char> tmp(o_out[count]);
            TRY(staged_copy(ctx, tmp.data(), ctx->out.p, tmp.size(), false));
            for (int i : tab.list[OMPB_L_ENT]) {
                if (state[i] != OMPB_BATCH) continue;
                if (any_view) host_view_move(hv, (char *)items[i].out, (char *)tmp.data() + o_out[i], 0, n * sizeof(T), false);      // (the sub-box's rows alone)
                else memcpy(items[i].out, tmp.data() + o_out[i], sh[i].n * sizeof(T));
            }
        }
        std::vector<u64> pairs;                               // the gathered views that decoded: their contiguous copies into the callers' arrays, ONE scatter launch
        for (int i : tab.list[OMPB_L_F3G]) if (state[i] == OMPB_BATCH) { pairs.push_back((u64)(uintptr_t)items[i].out); pairs.push_back((u64)(uintptr_t)tab.rec[i].out); }
        if (!pairs.empty()) {
            const u64 *d_pairs = (const u64 *)(tab.dev() + tab.o_extra + o_pairs);
            HIPCHK(hipMemcpyAsync((void *)d_pairs, pairs.data(), pairs.size() * 8, hipMemcpyHostToDevice, st));
            const int ppr = 1 + (int)((r2 + 16 / sizeof(T) - 1) / (16 / sizeof(T)));
            const int64_t total = (int64_t)(r0 * r1) * ppr;
            hipLaunchKernelGGL((k_ompb_view_scatter<T>), dim3((unsigned)((total + 255) / 256), (unsigned)(pairs.size() / 2)), dim3(256), 0, st, d_pairs, (int64_t)pitch0, (int64_t)pitch1,
                               (int)r1, (int)r2, ppr, total);
            HIPCHK(hipGetLastError());
            ++S.packing;                                      // (counted where it is launched)
            HIPCHK(hipStreamSynchronize(st));                 // (`pairs` is a pageable source; the single calls use the output buffer)
        }
        return SZHIP_OK;
    }
    // ---- the streams the shared launches do not cover: the single call.  The first failed item's code; the statistics
    int finish(szhip_stats *stats) {
        for (int i = 0; i < count; ++i) {
            if (state[i] != OMPB_SINGLE) continue;
            szhip_stats s1; memset(&s1, 0, sizeof(s1));
            const int rc = decompress_omp_impl<T>(ctx, items[i].stream, stream_on_device, items[i].stream_len, items[i].body_off, sh[i].r0, sh[i].r1, sh[i].r2, items[i].out, out_on_device,
                                                   any_view ? pitch0 : 0, any_view ? pitch1 : 0, &s1);
            items[i].rc = rc; items[i].batched = 0;
            if (rc != SZHIP_OK) { hipStreamSynchronize(st); continue; }
            items[i].intervals = s1.intervals; items[i].n_unpred = s1.n_unpred; items[i].quant_kernel = s1.quant_kernel;
            S.n_unpred += s1.n_unpred;
        }
        int rc_all = SZHIP_OK;
        for (int i = 0; i < count; ++i) if (items[i].rc != SZHIP_OK && rc_all == SZHIP_OK) rc_all = items[i].rc;
        S.out_bytes = (uint64_t)sum_n * sizeof(T);
        S.ms_host = host_ms; S.ms_total = now_ms() - t_begin;
        if (stats) *stats = S;
        return rc_all;
    }
};

template <class T>
int decompress_omp_batch_impl(szhip_ctx *ctx, szhip_batch_item *items, int count, int stream_on_device, const szhip_batch_shape *shapes, size_t r0, size_t r1, size_t r2,
                              int out_on_device, size_t pitch0, size_t pitch1, szhip_stats *stats)
{
    const bool mixed = shapes != nullptr;
    if (mixed) r0 = r1 = r2 = pitch0 = pitch1 = 0;
    ompb_dec<T> c{call_base(ctx), items, count, stream_on_device, mixed, r0, r1, r2, out_on_device, pitch0, pitch1};
    TRY(c.read_fronts(shapes));
    TRY(c.fill_table());
    TRY(c.launches());
    return c.finish(stats);
}
