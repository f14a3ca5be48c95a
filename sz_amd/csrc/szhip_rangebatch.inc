// szhip_rangebatch.inc -- part of szhip.hip (one translation unit; included inside its anonymous namespace, behind szhip_ompbatch.inc): the value range of many
// arrays of one length in one launch (include/szhip.h: szhip_minmax_batch; kernel: szh_rangebatch.h; DESIGN section 4.5.5).

// the limits of the batch calls over `count` arrays of n values (those of ompb_limits that do not speak of boxes)
static int batch_value_limits(szhip_ctx *ctx, const char *who, int count, size_t n)
{
    if (count > 65535 || n >= ((size_t)1 << 32) || (size_t)count * n >= ((size_t)1 << 32))
        FAIL(SZHIP_ERR_UNSUP, "%s: %d arrays of %zu values (at most 65535 arrays and 2^32 - 1 values in all)", who, count, n);
    return SZHIP_OK;
}

// The arrays are sub-boxes of r0 x r1 x r2 values (n in all) whose planes lie pitch0 and whose rows pitch1 elements apart (szhip_minmax_batch_view); the contiguous
// call comes as 1 x 1 x n with pitches n.  Sub-boxes on the host are staged packed and scanned as contiguous arrays.
// `lens` (or null): contiguous arrays of different lengths, array i of lens[i] values (szhip_minmax_batch_lens; r0 .. pitch1 come as 1 x 1 x the longest length).
template <class T>
int minmax_batch_impl(szhip_ctx *ctx, const void *const *data, int count, int on_dev, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1, const size_t *lens,
                      double *vmin, double *vmax, szhip_stats *stats)
{
    constexpr int VW = 16 / (int)sizeof(T);
    call_base cb(ctx); szhip_stats &S = cb.S; const hipStream_t st = cb.st;
    const size_t n = r0 * r1 * r2;
    const bool any_view = pitch1 != r2 || pitch0 != r1 * r2, view = any_view && on_dev;
    size_t sum_n = (size_t)count * n;
    if (lens) { sum_n = 0; for (int i = 0; i < count; ++i) sum_n += lens[i]; }
    if (lens) { if (count > 65535 || sum_n >= ((size_t)1 << 32)) FAIL(SZHIP_ERR_UNSUP, "szhip_minmax_batch_lens: %d arrays of %zu values in all (at most 65535 arrays and 2^32 - 1 values)", count, sum_n); }
    else TRY(batch_value_limits(ctx, any_view ? "szhip_minmax_batch_view" : "szhip_minmax_batch", count, n));
    S.n_elements = (uint64_t)sum_n;
    // ---- host arrays one behind the other into the context's input buffer; the table of base pointers, uploaded once
    std::vector<const void *> d_in(data, data + count);
    const host_view hv = {r1, r2 * sizeof(T), pitch0 * sizeof(T), pitch1 * sizeof(T)};
    std::vector<size_t> each;
    std::vector<int64_t> len64;
    if (lens) for (int i = 0; i < count; ++i) { each.push_back(lens[i] * sizeof(T)); len64.push_back((int64_t)lens[i]); }
    if (!on_dev) TRY(batch_stage(ctx, ctx->in, count, n * sizeof(T), st, [&](int i) { return data[i]; }, d_in, any_view ? &hv : nullptr, lens ? each.data() : nullptr));
    const size_t o_len = up64((size_t)count * sizeof(void *));                // (the lengths between the bases and the results, when there are any)
    const size_t o_res = o_len + (lens ? up64((size_t)count * 8) : 0);
    TRY(ensure(ctx, ctx->batch_rec, o_res + (size_t)count * 16));
    TRY(ensure_pinned(ctx, (size_t)count * 16));
    unsigned char *tab = (unsigned char *)ctx->batch_rec.p;
    HIPCHK(hipMemcpyAsync(tab, d_in.data(), (size_t)count * sizeof(void *), hipMemcpyHostToDevice, st));      // (`d_in` lives until the synchronisation below)
    if (lens) HIPCHK(hipMemcpyAsync(tab + o_len, len64.data(), (size_t)count * 8, hipMemcpyHostToDevice, st));      // (`len64` lives until the synchronisation below)
    HIPCHK(hipMemsetAsync(tab + o_res, 0, (size_t)count * 16, st));
    // ---- one launch, one read-back
    if (view) {                                                    // a group of lanes per row, sized to the row's 16-byte pieces
        int gs = 2 * VW;
        while (gs < 256 && (size_t)gs * VW < r2) gs *= 2;
        const size_t rows = r0 * r1, per_wg = 256 / (size_t)gs;
        const int grid = (int)std::min<size_t>((rows + per_wg - 1) / per_wg, (size_t)SZH_RB_MAX_GRID);
        hipLaunchKernelGGL((k_minmax_batch_view<T>), dim3((unsigned)grid, (unsigned)count), dim3(256), 0, st, (const T *const *)tab, (int64_t)pitch0, (int64_t)pitch1, (int64_t)rows,
                           (int)r1, (int)r2, gs, (u64 *)(tab + o_res));
    } else if (lens) {                                             // the grid of the longest array; the others' surplus workgroups return
        const int grid = szh_rangebatch_grid(n, VW);
        hipLaunchKernelGGL((k_minmax_batch_lens<T>), dim3((unsigned)grid, (unsigned)count), dim3(256), 0, st, (const T *const *)tab, (const int64_t *)(tab + o_len), (u64 *)(tab + o_res));
    } else {
        const int grid = szh_rangebatch_grid(n, VW);
        hipLaunchKernelGGL((k_minmax_batch<T>), dim3((unsigned)grid, (unsigned)count), dim3(256), 0, st, (const T *const *)tab, (int64_t)n, (u64 *)(tab + o_res));
    }
    HIPCHK(hipGetLastError());
    S.quant_kernel_launches = 1;
    HIPCHK(hipMemcpyAsync(ctx->pinned, tab + o_res, (size_t)count * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const u64 *res = (const u64 *)ctx->pinned;
    for (int i = 0; i < count; ++i) { vmin[i] = ord_dec<T>(~res[2 * (size_t)i]); vmax[i] = ord_dec<T>(res[2 * (size_t)i + 1]); }
    S.ms_total = now_ms() - cb.t_begin;
    return cb.done(stats);
}
