"""The error report for many pairs in one call: szhip_compare_batch (include/szhip.h) and HipContext.compare_batch.  Kernels: the batched wrappers of
sz_amd/csrc/szh_quality.h around the bodies the single call's kernels wrap.

Every case runs twice: on the device (-m gpu) and through the HIP-on-CPU shim (tests/sim).

The bar: record i of the batch equals, BYTE FOR BYTE, what szhip_compare returns for pair i alone -- without and with the correlation -- and its values meet
`reference()` of tests/test_quality.py (the reference's `sz -a` loop restated in numpy; sums within the bound that holds for any order of summation).

Sizes: those either side of the single call's grid rule (szh_quality_grid, stated in tests/test_quality.py): one sweep of a one-workgroup grid ends at 1024
float32 / 512 float64 points, a workgroup's share at 8192 / 4096; 70 001 float32 points take 9 workgroups per pair, whose slots the pair's final workgroup merges."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ptr_cases as P  # noqa: E402
from test_quality import assert_exact, assert_sums, pair, reference  # noqa: E402

f32, f64 = np.float32, np.float64
ERR_ARG, ERR_UNSUP = -2, -3
BACKENDS = [pytest.param("gpu", marks=pytest.mark.gpu, id="on_the_gpu"), pytest.param("shim", id="on_the_cpu_shim")]


@pytest.fixture(scope="module")
def gctx(built):
    import sz_amd
    c = sz_amd.HipContext(0)
    yield c
    c.close()


@pytest.fixture
def shim(built):
    import sim_lib
    from sz_amd import api
    old = api._lib
    api._lib = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    yield
    api._lib = old


@pytest.fixture
def sctx(shim):
    import sz_amd
    c = sz_amd.HipContext(0)
    yield c
    c.close()


@pytest.fixture(params=BACKENDS)
def env(request):
    if request.param == "gpu":
        return request.getfixturevalue("gctx"), True
    return request.getfixturevalue("sctx"), False


def place(dev, arrays, offs):
    return [P.carve(a.nbytes, o, device=dev).put(a) for a, o in zip(arrays, offs)]


def make_batch(n, dtype, count):
    """`count` pairs with bounds of their own: pair 0 is over its absolute bound at exactly one known point, pair 1 at none; a NaN pair and an inf pair (excluded and
    counted) in pair 2; the others as tests/test_quality.py's pair()"""
    oris, decs, abs_b, pwr_b = [], [], [], []
    for i in range(count):
        o, d = pair(n, dtype, 100 + i)
        ab, pb = 2e-3 * (i + 1), 1e-3 * (i + 1)
        if i == 0:
            d = o.copy()
            d[n // 3] = o[n // 3] + dtype(0.5)
            ab = 0.25
        if i == 1:
            ab = 10.0
        if i == 2 and n > 9:
            o[2], d[2] = np.nan, np.nan
            o[5] = np.nan
            o[n - 1], d[n - 1] = np.inf, np.inf
        oris.append(o), decs.append(d), abs_b.append(ab), pwr_b.append(pb)
    return oris, decs, abs_b, pwr_b


def check_batch(env, oris, decs, abs_b, pwr_b, corr, what):
    """the batch against the single call byte for byte and against the reference's loop; guards and inputs unchanged.  ori arrays 0, dec arrays 4 (float64: 8) bytes
    behind a 256-byte boundary, and the other way round for every second pair"""
    ctx, dev = env
    dtype, n, count = oris[0].dtype.type, oris[0].size, len(oris)
    step = np.dtype(dtype).itemsize
    ro = place(dev, oris, [0 if i % 2 == 0 else step for i in range(count)])
    rd = place(dev, decs, [step if i % 2 == 0 else 0 for i in range(count)])
    rc, got, st = ctx.compare_batch([r.ptr for r in ro], [r.ptr for r in rd], True, n, dtype, abs_b, pwr_b, corr=corr)
    assert rc == 0
    assert st.quant_kernel_launches == 1, f"{what}: {st.quant_kernel_launches} pass-1 launches for {count} pairs"
    for i in range(count):
        one = ctx.compare(ro[i].ptr, rd[i].ptr, True, n, dtype, abs_b[i], pwr_b[i], corr=corr)
        assert got[i].raw == one.raw, f"{what} pair {i}: the batch's record differs from the single call's\n{got[i]}\n{one}"
        r = reference(oris[i], decs[i], abs_b[i], pwr_b[i])
        assert_exact(got[i], r, f"{what} pair {i}")
        assert_sums(got[i], r, f"{what} pair {i}", corr=corr)
    for r, a in zip(ro + rd, oris + decs):
        r.check(what)
        assert np.array_equal(r.get(), a.reshape(-1).view(np.uint8)), f"{what}: an input was written"
    return got


SIZE_CASES = [(n, f32) for n in (1023, 1025, 8191, 8193, 70001)] + [(n, f64) for n in (511, 513, 4095, 4097)]


@pytest.mark.parametrize("corr", (False, True), ids=("plain", "corr"))
@pytest.mark.parametrize("n,dtype", SIZE_CASES, ids=[f"{t.__name__}-{n}" for n, t in SIZE_CASES])
def test_records_are_the_single_calls(env, n, dtype, corr):
    count = 4
    oris, decs, abs_b, pwr_b = make_batch(n, dtype, count)
    got = check_batch(env, oris, decs, abs_b, pwr_b, corr, f"{dtype.__name__} n = {n}")
    assert got[0].n_over_abs == 1 and got[0].first_over_idx == n // 3 and got[0].max_abs_idx == n // 3, f"pair 0: {got[0]}"
    assert got[1].n_over_abs == 0, f"pair 1: {got[1]}"
    assert got[2].n_excluded == 3 and got[2].n_excluded_diff == 1, f"pair 2: {got[2]}"
    assert got[3].n_excluded == 0


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("count", (1, 2, 6))
def test_counts_and_host_arrays(env, dtype, count):
    ctx, dev = env
    n = 16 * 16 * 16
    oris, decs, abs_b, pwr_b = make_batch(n, dtype, count)
    want = check_batch(env, oris, decs, abs_b, pwr_b, True, f"{count} pairs")
    rc, got, st = ctx.compare_batch([a.ctypes.data for a in oris], [a.ctypes.data for a in decs], False, n, dtype, abs_b, pwr_b, corr=True)
    assert rc == 0 and st.quant_kernel_launches == 1
    assert [g.raw for g in got] == [w.raw for w in want], "host arrays give other records than device arrays"
    rc, got, _ = ctx.compare_batch([a.ctypes.data for a in oris], [a.ctypes.data for a in decs], False, n, dtype, abs_b, None)
    assert rc == 0 and all(g.n_over_pwr == 0 and g.n_over_both == 0 for g in got), "pw_rel_bound == NULL is 'not asked'"


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
def test_a_pair_does_not_depend_on_its_neighbours(env, dtype):
    n = 8193
    oris, decs, abs_b, pwr_b = make_batch(n, dtype, 4)
    a = check_batch(env, oris, decs, abs_b, pwr_b, True, "first batch")
    o2, d2 = pair(n, dtype, 999)
    d2[7] = np.nan
    b = check_batch(env, [o2 * dtype(1e6), oris[3], d2], [d2, decs[3], o2], [1.0, abs_b[3], 0.0], [0.5, pwr_b[3], 0.0], True, "second batch")
    assert a[3].raw == b[1].raw, "a pair's record changed with its neighbours"


def test_refusals(env):
    ctx, dev = env
    o, d = pair(64, f32, 1)
    ro, rd = place(dev, [o, d], [0, 0])
    for what, op, dp, n, dtype, want in (("count < 1", [], [], 64, f32, ERR_ARG), ("n == 0", [ro.ptr], [rd.ptr], 0, f32, ERR_ARG),
                                         ("a null ori", [ro.ptr, None], [rd.ptr, rd.ptr], 64, f32, ERR_ARG), ("a null dec", [ro.ptr], [None], 64, f32, ERR_ARG),
                                         ("dec 2 bytes off", [ro.ptr], [rd.ptr + 2], 16, f32, ERR_ARG), ("ori 4 bytes off, float64", [ro.ptr + 4], [rd.ptr], 4, f64, ERR_ARG),
                                         ("count x n = 2^32", [ro.ptr] * 2, [rd.ptr] * 2, 2 ** 31, f32, ERR_UNSUP)):
        rc, _, _ = ctx.compare_batch(op, dp, True, n, dtype, [1.0] * max(len(op), 1), None, raise_on_error=False)
        print(f"{what}: rc = {rc}")
        assert rc == want, f"{what}: rc = {rc}, expected {want}"
    ro.check("refusals"), rd.check("refusals")
