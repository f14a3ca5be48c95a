// szhip_quality.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace): an array against its decoded copy (szh_quality.h).

// where a HOST array of the pair is staged: the context's input buffer for `ori`, a second buffer for `dec` -- the other way round when the partner is a device array
// that lies in the buffer a host array would go to (what szhip_stage_input handed out)
static bool quality_lies_in(const DevBuf &b, const void *p) { return b.p && (const char *)p >= (const char *)b.p && (const char *)p < (const char *)b.p + b.cap; }

template <class T>
int quality_stage(szhip_ctx *ctx, DevBuf &buf, const void *host, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1, const T **d)
{
    const size_t bytes = r0 * r1 * r2 * sizeof(T);
    TRY(ensure(ctx, buf, bytes));
    if (pitch1 == r2 && pitch0 == r1 * r2) TRY(staged_copy(ctx, buf.p, host, bytes, true));
    else {                                                          // a view on the host: its rows alone go to the device, packed
        const host_view hv = {r1, r2 * sizeof(T), pitch0 * sizeof(T), pitch1 * sizeof(T)};
        TRY(staged_copy(ctx, buf.p, host, bytes, true, &hv));
    }
    *d = (const T *)buf.p;
    return SZHIP_OK;
}

// the slots of `grid` workgroups into one, on the host
static int quality_collect(szhip_ctx *ctx, u64 *d_slots, int grid, u64 (&res)[SZH_Q_WORDS])
{
    u64 *d_res = d_slots + (size_t)grid * SZH_Q_WORDS;
    hipLaunchKernelGGL(k_quality_final, dim3(1), dim3(256), 0, ctx->stream, (const unsigned long long *)d_slots, grid, (unsigned long long *)d_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(res, d_res, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SZHIP_OK;
}

static double quality_double(u64 bits) { double d; memcpy(&d, &bits, 8); return d; }

// pass 1's merged record `res` of n points into the report's counts, extremes and sums (everything else zero)
template <class T>
void quality_from_pass1(const u64 (&res)[SZH_Q_WORDS], size_t n, szhip_quality *out)
{
    szhip_quality q;
    memset(&q, 0, sizeof(q));
    q.n = n; q.n_excluded = res[SZH_Q_NEX]; q.n_excluded_diff = res[SZH_Q_NEXD]; q.n_zero_changed = res[SZH_Q_NZC];
    q.n_over_abs = res[SZH_Q_NOA]; q.n_over_pwr = res[SZH_Q_NOP]; q.n_over_both = res[SZH_Q_NOB];
    q.max_abs_idx = res[SZH_Q_EIDX]; q.first_over_idx = res[SZH_Q_FIRST];
    const bool any = res[SZH_Q_EKEY] != 0;                          // (no point took part: every one was excluded)
    q.vmin = any ? ord_dec<T>(res[SZH_Q_OMIN]) : NAN; q.vmax = any ? ord_dec<T>(res[SZH_Q_OMAX]) : NAN;
    q.max_abs_err = any ? quality_double(res[SZH_Q_EKEY] - 1) : 0.0;
    q.max_pw_rel_err = quality_double(res[SZH_Q_PW]);
    q.sum_ori = quality_double(res[SZH_Q_S0]); q.sum_dec = quality_double(res[SZH_Q_S1]);
    q.sum_dec_sq = quality_double(res[SZH_Q_S2]); q.sum_err_sq = quality_double(res[SZH_Q_S3]);
    *out = q;
}
// pass 2's merged record into the centred sums
static void quality_from_pass2(const u64 (&res)[SZH_Q_WORDS], szhip_quality *q)
{
    q->cov = quality_double(res[SZH_Q_S0]); q->var_ori = quality_double(res[SZH_Q_S1]); q->var_dec = quality_double(res[SZH_Q_S2]);
}
template <class T>
void quality_derive(szhip_quality *out, unsigned flags)
{
    szhip_quality q = *out;
    const double took_part = (double)(q.n - q.n_excluded);
    // the derived values, by the formulas of example/sz.c:600-611 (the range of float data is the FLOAT difference, as `float Max - Min` there)
    q.range = sizeof(T) == 4 ? (double)(float)((float)q.vmax - (float)q.vmin) : q.vmax - q.vmin;
    q.mse = q.sum_err_sq / took_part;
    q.psnr = 20 * log10(q.range) - 10 * log10(q.mse);
    q.nrmse = sqrt(q.mse) / q.range;
    q.norm_err = sqrt(q.sum_err_sq);
    q.ac_eff = (flags & SZHIP_Q_CORR) ? q.cov / took_part / sqrt(q.var_ori / took_part) / sqrt(q.var_dec / took_part) : NAN;
    *out = q;
}

template <class T>
int quality_impl(szhip_ctx *ctx, const void *ori, int ori_on_device, size_t o_pitch0, size_t o_pitch1, const void *dec, int dec_on_device, size_t d_pitch0, size_t d_pitch1,
                 size_t r0, size_t r1, size_t r2, double abs_bound, double pw_rel_bound, unsigned flags, szhip_quality *out)
{
    constexpr int VW = 16 / (int)sizeof(T);
    const size_t n = r0 * r1 * r2;
    const T *d_ori = (const T *)ori, *d_dec = (const T *)dec;
    if (!ori_on_device || !dec_on_device) {
        const bool swap = (ori_on_device && quality_lies_in(ctx->in2, ori)) || (dec_on_device && quality_lies_in(ctx->in, dec));
        DevBuf &b_ori = swap ? ctx->in2 : ctx->in, &b_dec = swap ? ctx->in : ctx->in2;
        if (!ori_on_device) { TRY(quality_stage<T>(ctx, b_ori, ori, r0, r1, r2, o_pitch0, o_pitch1, &d_ori)); o_pitch0 = r1 * r2; o_pitch1 = r2; }
        if (!dec_on_device) { TRY(quality_stage<T>(ctx, b_dec, dec, r0, r1, r2, d_pitch0, d_pitch1, &d_dec)); d_pitch0 = r1 * r2; d_pitch1 = r2; }
    }
    const szh_qview VO = {(int64_t)r1, (int64_t)r2, (int64_t)o_pitch0, (int64_t)o_pitch1, o_pitch1 == r2 && o_pitch0 == r1 * r2 ? 1 : 0};
    const szh_qview VD = {(int64_t)r1, (int64_t)r2, (int64_t)d_pitch0, (int64_t)d_pitch1, d_pitch1 == r2 && d_pitch0 == r1 * r2 ? 1 : 0};
    const int grid = szh_quality_grid(n, VW);
    TRY(ensure(ctx, ctx->quality, ((size_t)grid + 1) * SZH_Q_WORDS * 8));
    u64 *d_slots = (u64 *)ctx->quality.p;
    u64 res[SZH_Q_WORDS];
    hipLaunchKernelGGL((k_quality_pass1<T>), dim3(grid), dim3(256), 0, ctx->stream, d_ori, VO, d_dec, VD, (int64_t)n, abs_bound, pw_rel_bound, (unsigned long long *)d_slots);
    HIPCHK(hipGetLastError());
    TRY(quality_collect(ctx, d_slots, grid, res));

    szhip_quality q;
    quality_from_pass1<T>(res, n, &q);
    const double took_part = (double)(n - q.n_excluded);
    if (flags & SZHIP_Q_CORR) {
        hipLaunchKernelGGL((k_quality_pass2<T>), dim3(grid), dim3(256), 0, ctx->stream, d_ori, VO, d_dec, VD, (int64_t)n, q.sum_ori / took_part, q.sum_dec / took_part,
                           (unsigned long long *)d_slots);
        HIPCHK(hipGetLastError());
        TRY(quality_collect(ctx, d_slots, grid, res));
        quality_from_pass2(res, &q);
    }
    quality_derive<T>(&q, flags);
    *out = q;
    return SZHIP_OK;
}

// ---- many pairs of one length in one call (szhip_compare_batch): the steps above, each ONE launch with the pair as the grid's second dimension.  ctx->quality holds
// [count x grid slots][count records][the pairs' table]; the table goes up once, and once more with the means of pass 1 when the correlation is asked for.
// szhip_compare_batch_view: every `ori` a box of r0 x r1 x r2 values with the element pitches o_pitch0 / o_pitch1, every `dec` one with d_pitch0 / d_pitch1 (the
// contiguous call comes as 1 x 1 x n with pitches n); the view kernels run when either side is a view on the device, host views are staged packed.
template <class T>
int quality_batch_impl(szhip_ctx *ctx, const void *const *ori, size_t o_pitch0, size_t o_pitch1, const void *const *dec, size_t d_pitch0, size_t d_pitch1, int count, int on_device,
                       size_t r0, size_t r1, size_t r2, const double *abs_bound, const double *pw_rel_bound, unsigned flags, szhip_quality *out, szhip_stats *stats)
{
    constexpr int VW = 16 / (int)sizeof(T);
    call_base cb(ctx); szhip_stats &S = cb.S; const hipStream_t st = cb.st;
    const size_t n = r0 * r1 * r2;
    const bool o_view = o_pitch1 != r2 || o_pitch0 != r1 * r2, d_view = d_pitch1 != r2 || d_pitch0 != r1 * r2, view = (o_view || d_view) && on_device;
    TRY(batch_value_limits(ctx, o_view || d_view ? "szhip_compare_batch_view" : "szhip_compare_batch", count, n));
    S.n_elements = (uint64_t)count * n;
    std::vector<const void *> d_ori(ori, ori + count), d_dec(dec, dec + count);
    if (!on_device) {                                               // (both through the one pinned block: the first copy has left it before the second fills it)
        const host_view hvo = {r1, r2 * sizeof(T), o_pitch0 * sizeof(T), o_pitch1 * sizeof(T)}, hvd = {r1, r2 * sizeof(T), d_pitch0 * sizeof(T), d_pitch1 * sizeof(T)};
        TRY(batch_stage(ctx, ctx->in, count, n * sizeof(T), st, [&](int i) { return ori[i]; }, d_ori, o_view ? &hvo : nullptr));
        HIPCHK(hipStreamSynchronize(st));
        TRY(batch_stage(ctx, ctx->in2, count, n * sizeof(T), st, [&](int i) { return dec[i]; }, d_dec, d_view ? &hvd : nullptr));
    }
    const szh_qview VO = {(int64_t)r1, (int64_t)r2, (int64_t)o_pitch0, (int64_t)o_pitch1, o_view ? 0 : 1}, VD = {(int64_t)r1, (int64_t)r2, (int64_t)d_pitch0, (int64_t)d_pitch1, d_view ? 0 : 1};
    const int grid = szh_quality_grid(n, VW);
    const size_t rec_bytes = (size_t)SZH_Q_WORDS * 8, o_res = (size_t)count * grid * rec_bytes, o_tab = o_res + (size_t)count * rec_bytes;
    TRY(ensure(ctx, ctx->quality, o_tab + (size_t)count * sizeof(szh_qpair)));
    TRY(ensure_pinned(ctx, (size_t)count * rec_bytes));
    unsigned char *base = (unsigned char *)ctx->quality.p;
    unsigned long long *d_slots = (unsigned long long *)base, *d_res = (unsigned long long *)(base + o_res);
    const szh_qpair *d_tab = (const szh_qpair *)(base + o_tab);
    std::vector<szh_qpair> tab((size_t)count), tab2;               // (pageable sources of the uploads: they live until the synchronisation behind each)
    for (int i = 0; i < count; ++i) tab[i] = szh_qpair{d_ori[i], d_dec[i], abs_bound[i], pw_rel_bound ? pw_rel_bound[i] : -1.0, 0.0, 0.0};
    HIPCHK(hipMemcpyAsync(base + o_tab, tab.data(), (size_t)count * sizeof(szh_qpair), hipMemcpyHostToDevice, st));
    // the pairs' slots into their records, the records to the host: one launch, one read-back
    auto collect = [&]() -> int {
        hipLaunchKernelGGL(k_quality_final_batch, dim3(1, (unsigned)count), dim3(256), 0, st, (const unsigned long long *)d_slots, grid, d_res);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ctx->pinned, d_res, (size_t)count * rec_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return SZHIP_OK;
    };
    typedef const u64 (&rec_ref)[SZH_Q_WORDS];
    auto rec = [&](int i) -> rec_ref { return *(const u64 (*)[SZH_Q_WORDS])((const u64 *)ctx->pinned + (size_t)i * SZH_Q_WORDS); };
    if (view) hipLaunchKernelGGL((k_quality_pass1_batch_view<T>), dim3((unsigned)grid, (unsigned)count), dim3(256), 0, st, d_tab, VO, VD, (int64_t)n, d_slots);
    else hipLaunchKernelGGL((k_quality_pass1_batch<T>), dim3((unsigned)grid, (unsigned)count), dim3(256), 0, st, d_tab, (int64_t)n, d_slots);
    HIPCHK(hipGetLastError());
    S.quant_kernel_launches = 1;
    TRY(collect());
    std::vector<szhip_quality> q((size_t)count);
    for (int i = 0; i < count; ++i) quality_from_pass1<T>(rec(i), n, &q[i]);
    if (flags & SZHIP_Q_CORR) {
        tab2 = tab;
        for (int i = 0; i < count; ++i) {
            const double took_part = (double)(n - q[i].n_excluded);
            tab2[i].mean_ori = q[i].sum_ori / took_part; tab2[i].mean_dec = q[i].sum_dec / took_part;
        }
        HIPCHK(hipMemcpyAsync(base + o_tab, tab2.data(), (size_t)count * sizeof(szh_qpair), hipMemcpyHostToDevice, st));
        if (view) hipLaunchKernelGGL((k_quality_pass2_batch_view<T>), dim3((unsigned)grid, (unsigned)count), dim3(256), 0, st, d_tab, VO, VD, (int64_t)n, d_slots);
        else hipLaunchKernelGGL((k_quality_pass2_batch<T>), dim3((unsigned)grid, (unsigned)count), dim3(256), 0, st, d_tab, (int64_t)n, d_slots);
        HIPCHK(hipGetLastError());
        TRY(collect());
        for (int i = 0; i < count; ++i) quality_from_pass2(rec(i), &q[i]);
    }
    for (int i = 0; i < count; ++i) { quality_derive<T>(&q[i], flags); out[i] = q[i]; }
    S.ms_total = now_ms() - cb.t_begin;
    return cb.done(stats);
}
