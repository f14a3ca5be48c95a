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
    const double took_part = (double)(n - q.n_excluded);
    if (flags & SZHIP_Q_CORR) {
        hipLaunchKernelGGL((k_quality_pass2<T>), dim3(grid), dim3(256), 0, ctx->stream, d_ori, VO, d_dec, VD, (int64_t)n, q.sum_ori / took_part, q.sum_dec / took_part,
                           (unsigned long long *)d_slots);
        HIPCHK(hipGetLastError());
        TRY(quality_collect(ctx, d_slots, grid, res));
        q.cov = quality_double(res[SZH_Q_S0]); q.var_ori = quality_double(res[SZH_Q_S1]); q.var_dec = quality_double(res[SZH_Q_S2]);
    }
    // the derived values, by the formulas of example/sz.c:600-611 (the range of float data is the FLOAT difference, as `float Max - Min` there)
    q.range = sizeof(T) == 4 ? (double)(float)((float)q.vmax - (float)q.vmin) : q.vmax - q.vmin;
    q.mse = q.sum_err_sq / took_part;
    q.psnr = 20 * log10(q.range) - 10 * log10(q.mse);
    q.nrmse = sqrt(q.mse) / q.range;
    q.norm_err = sqrt(q.sum_err_sq);
    q.ac_eff = (flags & SZHIP_Q_CORR) ? q.cov / took_part / sqrt(q.var_ori / took_part) / sqrt(q.var_dec / took_part) : NAN;
    *out = q;
    return SZHIP_OK;
}
