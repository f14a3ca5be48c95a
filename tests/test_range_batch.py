"""The value range of many arrays in one launch: szhip_minmax_batch (include/szhip.h) and HipContext.minmax_batch.  Kernel: sz_amd/csrc/szh_rangebatch.h.

Every case runs twice: on the device (-m gpu, torch uint8 tensors) and through the HIP-on-CPU shim (tests/sim), where "device" memory is host memory.

Expected values: numpy nanmin / nanmax, compared BY VALUE (so the sign of a zero is not theirs to settle), and -- bit for bit -- szhip_minmax on each array
alone: that call is existing code and settles the zero's sign and what an array without a number gives.

The grid rule the sizes below are chosen for (szh_rangebatch_grid): an array is cut at the 16-byte boundaries of its own address into a head of fewer than
VW = 16 / itemsize values, 16-byte pieces of VW values, and a tail of fewer than VW values.  A lane takes one piece per load with 4 in flight, a workgroup has 256
lanes, so a workgroup's share is 256 * 4 * VW values (4096 float32, 2048 float64) and grid = clamp(ceil(n / share), 1, 128) workgroups per array.  One sweep of
the largest grid covers 128 * share values (524 288 float32, 262 144 float64); beyond it a lane goes round again (those two sizes run with one array, 4 / 8
bytes behind a boundary, to stay quick on the CPU shim; every other size with three arrays at three offsets)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ptr_cases as P  # noqa: E402

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


def bits(v, dtype):
    return np.array([v], dtype=dtype).view(np.uint32 if dtype == f32 else np.uint64)[0]


def check(env, arrays, offs=None, what=""):
    """the batch over `arrays` (placed offs[i] bytes behind a 256-byte boundary inside guarded allocations) against numpy by value and against the single call bit
    for bit; guards and inputs unchanged; returns the stats"""
    ctx, dev = env
    dtype, n = arrays[0].dtype.type, arrays[0].size
    offs = offs or [0] * len(arrays)
    regions = [P.carve(a.nbytes, o, device=dev).put(a) for a, o in zip(arrays, offs)]
    rc, got, st = ctx.minmax_batch([r.ptr for r in regions], True, n, dtype)
    assert rc == 0
    for i, (a, r) in enumerate(zip(arrays, regions)):
        lo, hi = got[i]
        one = ctx.minmax(r.ptr, True, n, dtype)
        print(f"{what} array {i} at +{offs[i]}: batch ({lo!r}, {hi!r}), alone {one!r}")
        assert bits(lo, f64) == bits(one[0], f64) and bits(hi, f64) == bits(one[1], f64), f"{what} array {i}: batch ({lo!r}, {hi!r}) is not the single call's {one!r}"
        if not np.all(np.isnan(a)):
            assert lo == float(np.nanmin(a)) and hi == float(np.nanmax(a)), f"{what} array {i}: ({lo!r}, {hi!r}), numpy gives ({np.nanmin(a)!r}, {np.nanmax(a)!r})"
        r.check(f"{what} array {i}")
        assert np.array_equal(r.get(), a.reshape(-1).view(np.uint8)), f"{what} array {i}: the input was written"
    return st


def ordinary(n, dtype, seed):
    return (np.random.default_rng(seed).standard_normal(n) * (1 + seed)).astype(dtype)


# ------------------------------------------------------------------------------------------------------------------ sizes

def _sizes(dtype):
    vw = 16 // np.dtype(dtype).itemsize
    share = 256 * 4 * vw
    return (1, vw - 1, vw + 1, share - 1, share + 1, 32768, 128 * share - 1, 128 * share + 1)


SIZE_CASES = [(n, t) for t in (f32, f64) for n in _sizes(t)]


@pytest.mark.parametrize("n,dtype", SIZE_CASES, ids=[f"{t.__name__}-{n}" for n, t in SIZE_CASES])
def test_every_size_at_three_offsets(env, n, dtype):
    """three arrays of one batch 0, 4 (8 for float64) and 8 bytes behind a 256-byte boundary: heads of 0, 3 and 2 float32 values (0, 1 and 1 float64), the
    extremes planted in the head, the tail and a piece"""
    step = np.dtype(dtype).itemsize
    offs = [0, step, 8]
    arrays = [ordinary(n, dtype, s) for s in range(3)]
    arrays[0][0], arrays[0][-1] = dtype(99), dtype(-99)
    arrays[1][-1], arrays[1][0] = dtype(77), dtype(-77)
    arrays[2][n // 2] = dtype(55)
    if n > 100000:
        arrays, offs = arrays[1:2], offs[1:2]
    check(env, arrays, offs, f"{dtype.__name__} n = {n}")


# ------------------------------------------------------------------------------------------------------------------ special arrays

@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
def test_special_arrays(env, dtype):
    n = 4099
    base = ordinary(n, dtype, 5)
    first_max, last_min = base.copy(), base.copy()
    first_max[0], last_min[-1] = dtype(1e6), dtype(-1e6)
    nan_first, nan_last = base.copy(), base.copy()
    nan_first[0], nan_first[1] = np.nan, dtype(1e6)                 # the extreme next to a NaN at the first ...
    nan_last[-1], nan_last[-2] = np.nan, dtype(-1e6)                # ... and at the last position
    infs = base.copy()
    infs[7], infs[n - 7] = np.inf, -np.inf
    zeros = np.zeros(n, dtype)                                      # -0.0 and +0.0 as the only extremes
    zeros[3] = dtype(-0.0)
    neg_zeros = np.full(n, dtype(-0.0), dtype)
    neg_zeros[n - 2] = dtype(0.0)
    all_nan = np.full(n, np.nan, dtype)
    arrays = [first_max, last_min, nan_first, all_nan, nan_last, infs, zeros, neg_zeros, base.copy()]
    step = np.dtype(dtype).itemsize
    check(env, arrays, [0, step, 8, 0, step, 8, 0, step, 8], f"{dtype.__name__} specials")
    ctx, dev = env
    rz = P.carve(zeros.nbytes, 0, device=dev).put(zeros)
    _, got, _ = ctx.minmax_batch([rz.ptr], True, n, dtype)
    assert bits(got[0][0], f64) == bits(-0.0, f64) and bits(got[0][1], f64) == bits(0.0, f64), f"zeros of both signs: {got[0]!r}"


# ------------------------------------------------------------------------------------------------------------------ host pointers, launches, refusals

@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("count", (1, 3, 6))
def test_host_arrays_and_one_launch(env, dtype, count):
    ctx, dev = env
    n = 8 * 64 * 64
    arrays = [ordinary(n, dtype, 10 + i) for i in range(count)]
    st = check(env, arrays, [(0, np.dtype(dtype).itemsize, 8)[i % 3] for i in range(count)], f"{count} arrays")
    assert st.quant_kernel_launches == 1, f"{count} arrays took {st.quant_kernel_launches} scan launches"
    keep = [a.copy() for a in arrays]
    rc, got, st = ctx.minmax_batch([a.ctypes.data for a in arrays], False, n, dtype)
    assert rc == 0 and st.quant_kernel_launches == 1
    for a, k, (lo, hi) in zip(arrays, keep, got):
        assert (lo, hi) == ctx.minmax(a.ctypes.data, False, n, dtype) == (float(a.min()), float(a.max()))
        assert np.array_equal(a.view(np.uint8), k.view(np.uint8)), "a host input was written"


def test_refusals(env):
    ctx, dev = env
    a = ordinary(64, f32, 1)
    r = P.carve(a.nbytes, 0, device=dev).put(a)
    for what, ptrs, n, dtype, want in (("count < 1", [], 64, f32, ERR_ARG), ("n == 0", [r.ptr], 0, f32, ERR_ARG), ("a null pointer", [r.ptr, None], 64, f32, ERR_ARG),
                                       ("a float32 pointer 2 bytes off", [r.ptr, r.ptr + 2], 16, f32, ERR_ARG),
                                       ("a float64 pointer 4 bytes off", [r.ptr + 4], 4, f64, ERR_ARG),
                                       ("count x n = 2^32", [r.ptr] * 2, 2 ** 31, f32, ERR_UNSUP), ("count > 65535", [r.ptr] * 65536, 1, f32, ERR_UNSUP)):
        rc, _, _ = ctx.minmax_batch(ptrs, True, n, dtype, raise_on_error=False)
        print(f"{what}: rc = {rc}")
        assert rc == want, f"{what}: rc = {rc}, expected {want}"
    r.check("refusals")
