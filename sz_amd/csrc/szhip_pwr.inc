// szhip_pwr.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace): point-wise relative bounds: the log-domain preparation passes.
// =====================================================================================================================
// Point-wise relative bounds, log-domain form (szh_pwr.h)
// =====================================================================================================================
template <class T>
int pwr_prepare_impl(szhip_ctx *ctx, const void *data, int data_on_device, size_t n, double vmin, double vmax, double ratio, void **d_log_out,
                     unsigned char *signs_host, int *positive, double *real_precision, double *value_range, double *median, double *min_log_value)
{
    hipStream_t st = ctx->stream;
    const T *d_in = nullptr;
    TRY(stage_input(ctx, data, data_on_device, n, &d_in));
    TRY(ensure(ctx, ctx->pwr_log, n * sizeof(T)));
    TRY(ensure(ctx, ctx->pwr_signs, n));
    TRY(ensure(ctx, ctx->pwr_small, PWR_RED * 8));
    T *d_log = (T *)ctx->pwr_log.p;
    u64 *red = (u64 *)ctx->pwr_small.p;
    const u64 init[PWR_RED] = {~0ull, 0ull, ~0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    HIPCHK(hipMemcpyAsync(red, init, sizeof(init), hipMemcpyHostToDevice, st));
    const int grid = (int)std::min<int64_t>(((int64_t)n + 255) / 256, 4096);
    hipLaunchKernelGGL((k_pwr_log<T>), dim3(grid), dim3(256), 0, st, d_in, (int64_t)n, d_log, (unsigned char *)ctx->pwr_signs.p, red);
    HIPCHK(hipGetLastError());
    u64 res[PWR_RED];
    HIPCHK(hipMemcpyAsync(res, red, sizeof(res), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // sz_float_pwr.c:1923-1947, in the data's type where the reference's variables have it
    const T tmin = (T)vmin, tmax = (T)vmax;
    T max_abs_log;
    if (tmin == 0) max_abs_log = (T)fabs(log2(fabs((double)tmax)));
    else if (tmax == 0) max_abs_log = (T)fabs(log2(fabs((double)tmin)));
    else max_abs_log = (T)(fabs(log2(fabs((double)tmin))) > fabs(log2(fabs((double)tmax))) ? fabs(log2(fabs((double)tmin))) : fabs(log2(fabs((double)tmax))));
    T min_log = max_abs_log;
    if (res[PWR_NONZERO]) {
        const T lo = (T)ord_dec<T>(res[PWR_MINLOG]), hi = (T)ord_dec<T>(res[PWR_MAXLOG]);
        if (hi > max_abs_log) max_abs_log = hi;
        if (lo < min_log) min_log = lo;
    }
    const T amin = (T)ord_dec<T>(res[PWR_MINALL]), amax = (T)ord_dec<T>(res[PWR_MAXALL]);     // computeRangeSize_float on the log array, zeros still 0
    const T range = amax - amin;
    *value_range = (double)range;
    *median = (double)(T)(amin + range / 2);
    if (fabs((double)min_log) > (double)max_abs_log) max_abs_log = (T)fabs((double)min_log);
    const double rp = log2(1.0 + ratio) - (double)max_abs_log * (sizeof(T) == 4 ? 1.2e-7 : 2.23e-16);
    *real_precision = rp;
    const T zval = (T)((double)min_log - 2.0001 * rp);
    *min_log_value = (double)(T)((double)min_log - 1.0001 * rp);
    hipLaunchKernelGGL((k_pwr_zero<T>), dim3(grid), dim3(256), 0, st, d_in, (int64_t)n, d_log, zval);
    HIPCHK(hipGetLastError());
    *positive = res[PWR_NEG] ? 0 : 1;
    if (res[PWR_NEG] && signs_host) HIPCHK(hipMemcpyAsync(signs_host, ctx->pwr_signs.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *d_log_out = d_log;
    return SZHIP_OK;
}


// computeRangeSize_float_MSST19 (dataCompression.c:121-166) and the zero replacement of the _MSST19 wrappers (sz_float_pwr.c:2053-2062), on a COPY
// (the reference overwrites the caller's zeros).  nearZero: the first value of least non-zero magnitude -- or 0 when element 0 is zero (the scan
// starts from it and nothing is smaller in magnitude than 0); signs: from element 1 on, as the reference's loop.
template <class T>
int msst_prepare_impl(szhip_ctx *ctx, const void *data, int data_on_device, size_t n, double vmax, double ratio, void **d_prep_out,
                      unsigned char *signs_host, int *positive, double *near_zero_out, double *median_log, double *min_log_value)
{
    hipStream_t st = ctx->stream;
    const T *d_in = nullptr;
    TRY(stage_input(ctx, data, data_on_device, n, &d_in));
    TRY(ensure(ctx, ctx->pwr_log, n * sizeof(T)));
    TRY(ensure(ctx, ctx->pwr_signs, n));
    TRY(ensure(ctx, ctx->pwr_small, PWR_RED * 8));
    T *d_prep = (T *)ctx->pwr_log.p;
    u64 *red = (u64 *)ctx->pwr_small.p;
    const u64 init[MS_RED] = {~0ull, ~0ull, 0ull, 0ull};
    HIPCHK(hipMemcpyAsync(red, init, sizeof(init), hipMemcpyHostToDevice, st));
    const int grid = (int)std::min<int64_t>(((int64_t)n + 255) / 256, 4096);
    hipLaunchKernelGGL((k_msst_scan<T>), dim3(grid), dim3(256), 0, st, d_in, (int64_t)n, (unsigned char *)ctx->pwr_signs.p, red);
    HIPCHK(hipGetLastError());
    u64 res[MS_RED]; T first = 0;
    HIPCHK(hipMemcpyAsync(res, red, sizeof(res), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&first, d_in, sizeof(T), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    T near_zero = 0;
    if (first != 0 && res[MS_MINMAG] != ~0ull) {
        hipLaunchKernelGGL((k_msst_minidx<T>), dim3(grid), dim3(256), 0, st, d_in, (int64_t)n, res[MS_MINMAG], red);
        HIPCHK(hipGetLastError());
        u64 idx = 0;
        HIPCHK(hipMemcpyAsync(&idx, red + MS_MINIDX, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (idx >= n) FAIL(SZHIP_ERR_INTERNAL, "nearZero position out of range");
        HIPCHK(hipMemcpyAsync(&near_zero, d_in + idx, sizeof(T), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    const T multiplier = (T)pow(1 + ratio, -3.0001);
    const T zval = (T)(near_zero * multiplier);
    hipLaunchKernelGGL((k_msst_fill<T>), dim3(grid), dim3(256), 0, st, d_in, (int64_t)n, d_prep, zval);
    HIPCHK(hipGetLastError());
    *near_zero_out = (double)near_zero;
    *median_log = (double)(T)sqrt(fabs((double)(T)(near_zero * (T)vmax)));
    *min_log_value = (double)(T)((double)near_zero / ((1 + ratio) * (1 + ratio)));
    *positive = res[MS_NEG] ? 0 : 1;
    if (res[MS_NEG] && signs_host) HIPCHK(hipMemcpyAsync(signs_host, ctx->pwr_signs.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *d_prep_out = d_prep;
    return SZHIP_OK;
}

template <class T>
int decompress14_pwr_impl(szhip_ctx *ctx, const unsigned char *stream, int stream_on_device, size_t stream_len, size_t body_off,
                          size_t r0, size_t r1, size_t r2, const unsigned char *signs_host, double threshold, bool msst, void *out, int out_on_device, szhip_stats *stats)
{
    const size_t n = (r0 ? r0 : 1) * (r1 ? r1 : 1) * r2;
    hipStream_t st = ctx->stream;
    TRY(ensure(ctx, ctx->pwr_log, n * sizeof(T)));
    T *d_log = (T *)ctx->pwr_log.p;
    TRY(decompress14_impl<T>(ctx, stream, stream_on_device, stream_len, body_off, msst ? 2 : 1, r0, r1, r2, d_log, 1, stats));
    const unsigned char *d_signs = nullptr;
    if (signs_host) {
        TRY(ensure(ctx, ctx->pwr_signs, n));
        HIPCHK(hipMemcpyAsync(ctx->pwr_signs.p, signs_host, n, hipMemcpyHostToDevice, st));
        d_signs = (const unsigned char *)ctx->pwr_signs.p;
    }
    T *d_out = nullptr;
    TRY(device_out(ctx, out, out_on_device, n, &d_out));
    const int grid = (int)std::min<int64_t>(((int64_t)n + 255) / 256, 4096);
    if (msst) hipLaunchKernelGGL((k_msst_post<T>), dim3(grid), dim3(256), 0, st, (const T *)d_log, (int64_t)n, (T)threshold, d_signs, d_out);
    else hipLaunchKernelGGL((k_pwr_exp<T>), dim3(grid), dim3(256), 0, st, (const T *)d_log, (int64_t)n, (T)threshold, d_signs, d_out);
    HIPCHK(hipGetLastError());
    TRY(return_out(ctx, out, out_on_device, d_out, n));
    HIPCHK(hipStreamSynchronize(st));
    return SZHIP_OK;
}
