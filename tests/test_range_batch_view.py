"""The value ranges of many same-shape sub-boxes in one launch: szhip_minmax_batch_view (include/szhip.h) and HipContext.minmax_batch_view.  Kernel:
k_minmax_batch_view of sz_amd/csrc/szh_rangebatch.h.

Every case runs twice: on the device (-m gpu) and through the HIP-on-CPU shim (tests/sim), where "device" memory is host memory.

Expected values: szhip_minmax on a contiguous copy of each sub-box alone, BIT FOR BIT (that call is existing code and settles the sign of a zero and what a sub-box
without a number gives), and numpy nanmin / nanmax by value.  The parents are the padded arrays of tests/test_omp_batch_view.py; their ghost cells hold garbage
-- NaNs, 1e30, larger and smaller than anything inside --, so a read outside a sub-box shows in the result.  Inputs and guard bytes are compared afterwards.

The mapping the shapes are chosen for: every ROW of a sub-box is cut at the 16-byte boundaries of its own address (a head, 16-byte pieces of VW = 16 / itemsize values,
a tail); a group of gs lanes takes a row, gs the power of two in [2 VW, 256] that covers the row's pieces; a sub-box has at most 128 workgroups of 256 / gs groups.
So: rows shorter than VW (head and tail only), rows of exactly the pieces of a group, rows a lane goes round for (beyond 256 x 4 pieces), more rows than one sweep
of the grid takes (128 x 256 / gs), and ghost widths that put the rows at every offset from a boundary."""
import ctypes

import numpy as np
import pytest

import ptr_cases as P
from test_omp_batch_view import _garbage, _layout

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
def sctx(built):
    import sim_lib
    import sz_amd
    from sz_amd import api
    old = api._lib
    api._lib = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    c = sz_amd.HipContext(0)
    yield c
    c.close()
    api._lib = old


@pytest.fixture(params=BACKENDS)
def env(request):
    if request.param == "gpu":
        return request.getfixturevalue("gctx"), True
    return request.getfixturevalue("sctx"), False


def bits(v):
    return np.array([v], dtype=f64).view(np.uint64)[0]


def interior(shape, dtype, seed):
    return (np.random.default_rng(seed).standard_normal(shape) * (1 + seed)).astype(dtype)


def check(env, boxes, ghosts, offs=None, extra0=0, far_ghost=True, on_device=True, what=""):
    """the batch over the sub-boxes `boxes` (each the interior of its own padded parent, offs[i] bytes behind a 256-byte boundary) against the single call on a
    contiguous copy, bit for bit, and against numpy by value; parents and guards unchanged; returns the stats"""
    ctx, dev = env
    dtype, shape = boxes[0].dtype.type, boxes[0].shape
    esz = np.dtype(dtype).itemsize
    lay = _layout(shape, ghosts, extra0, far_ghost)
    offs = offs or [0] * len(boxes)
    parents = []
    for i, b in enumerate(boxes):
        p = _garbage(lay.total, dtype, 70 + i)
        p[np.nonzero(lay.outside)[0][::7]] = -np.inf                    # (next to the garbage's own 1e30 and NaNs)
        p[lay.idx] = b.reshape(-1)
        parents.append(p)
    regs = [P.carve(p.nbytes, o, pad=256, device=dev and on_device).put(p) for p, o in zip(parents, offs)]
    rc, got, st = ctx.minmax_batch_view([r.ptr + lay.lead * esz for r in regs], on_device, shape, lay.pitches, dtype)
    assert rc == 0
    assert st.quant_kernel_launches == 1, f"{what}: {st.quant_kernel_launches} scan launches for {len(boxes)} sub-boxes"
    for i, (b, r) in enumerate(zip(boxes, regs)):
        lo, hi = got[i]
        c = P.carve(b.nbytes, 0, device=dev).put(b)
        one = ctx.minmax(c.ptr, True, b.size, dtype)
        print(f"{what} sub-box {i} at +{offs[i]}: batch ({lo!r}, {hi!r}), contiguous copy alone {one!r}")
        assert bits(lo) == bits(one[0]) and bits(hi) == bits(one[1]), f"{what} sub-box {i}: batch ({lo!r}, {hi!r}) is not the single call's {one!r}"
        if not np.all(np.isnan(b)):
            assert lo == float(np.nanmin(b)) and hi == float(np.nanmax(b)), f"{what} sub-box {i}: ({lo!r}, {hi!r}), numpy gives ({np.nanmin(b)!r}, {np.nanmax(b)!r})"
        r.check(f"{what} sub-box {i}")
        assert np.array_equal(r.get(), parents[i].view(np.uint8)), f"{what} sub-box {i}: the parent was written"
    return st


SHAPES = [(8, 64, 64), (16, 16, 16), (3, 5, 7), (4, 3, 1), (2, 3, 2), (1, 2, 4200), (70, 64, 8), (5, 1, 33)]
PADS = [((1, 1, 1), 0), ((0, 0, 2), 0), ((2, 3, 4), 0), ((2, 3, 4), 5), ((2, 2, 2), 0)]


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_every_shape_and_ghost_width(env, shape, dtype):
    """three sub-boxes per call, their parents 0, 4 (8 for float64) and 8 bytes behind a boundary; the extremes planted at a row's first value, its last, and inside"""
    step = np.dtype(dtype).itemsize
    for ghosts, extra0 in PADS:
        boxes = [interior(shape, dtype, s) for s in range(3)]
        boxes[0][0, 0, 0], boxes[0][-1, -1, -1] = dtype(99), dtype(-99)
        boxes[1][-1, 0, -1], boxes[1][0, -1, 0] = dtype(77), dtype(-77)
        boxes[2][shape[0] // 2, shape[1] // 2, shape[2] // 2] = dtype(55)
        check(env, boxes, ghosts, [0, step, 8], extra0, what=f"{dtype.__name__} {shape} ghosts {ghosts} + {extra0}")


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
def test_special_values_and_the_far_end(env, dtype):
    shape = (4, 6, 19)
    base = interior(shape, dtype, 5)
    nan_first, nan_last, infs = base.copy(), base.copy(), base.copy()
    nan_first[0, 0, 0], nan_first[0, 0, 1] = np.nan, dtype(1e6)
    nan_last[-1, -1, -1], nan_last[-1, -1, -2] = np.nan, dtype(-1e6)
    infs[1, 2, 3], infs[2, 5, 18] = np.inf, -np.inf
    zeros = np.zeros(shape, dtype)
    zeros[1, 1, 3] = dtype(-0.0)
    neg_zeros = np.full(shape, dtype(-0.0), dtype)
    neg_zeros[3, 5, 17] = dtype(0.0)
    all_nan = np.full(shape, np.nan, dtype)
    boxes = [nan_first, all_nan, nan_last, infs, zeros, neg_zeros, base.copy()]
    step = np.dtype(dtype).itemsize
    offs = [0, step, 8, 0, step, 8, 0]
    for far_ghost in (True, False):                                      # (False: the last row ends at the parent's last byte)
        check(env, boxes, (1, 1, 1), offs, far_ghost=far_ghost, what=f"{dtype.__name__} specials")
        check(env, boxes, (2, 3, 4), offs, far_ghost=far_ghost, what=f"{dtype.__name__} specials, aligned")


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("count", (1, 3, 6))
def test_counts_host_parents_and_the_contiguous_call(env, dtype, count):
    ctx, dev = env
    shape = (8, 64, 64)
    boxes = [interior(shape, dtype, 10 + i) for i in range(count)]
    offs = [(0, np.dtype(dtype).itemsize, 8)[i % 3] for i in range(count)]
    check(env, boxes, (1, 1, 1), offs, what=f"{count} sub-boxes")
    check(env, boxes, (1, 1, 1), offs, on_device=False, what=f"{count} sub-boxes on the host")
    # pitch1 == r2 with pitch0 == r1 r2: the contiguous batch call
    regs = [P.carve(b.nbytes, o, device=dev).put(b) for b, o in zip(boxes, offs)]
    rc1, want, st1 = ctx.minmax_batch([r.ptr for r in regs], True, boxes[0].size, dtype)
    rc2, got, st2 = ctx.minmax_batch_view([r.ptr for r in regs], True, shape, (shape[1] * shape[2], shape[2]), dtype)
    assert rc1 == 0 and rc2 == 0 and st2.quant_kernel_launches == 1
    assert [(bits(a), bits(b)) for a, b in got] == [(bits(a), bits(b)) for a, b in want]


def test_refusals(env):
    ctx, dev = env
    shape = (4, 6, 8)
    lay = _layout(shape, (1, 1, 1))
    p = _garbage(lay.total, f32, 1)
    r = P.carve(p.nbytes, 0, device=dev).put(p)
    base = r.ptr + lay.lead * 4
    ok = lay.pitches
    for what, ptrs, shp, pitches, dtype, want in (("count < 1", [], shape, ok, f32, ERR_ARG), ("an empty box", [base], (4, 0, 8), ok, f32, ERR_ARG),
                                                  ("a null pointer", [base, None], shape, ok, f32, ERR_ARG),
                                                  ("a float32 pointer 2 bytes off", [base, base + 2], shape, ok, f32, ERR_ARG),
                                                  ("a float64 pointer 4 bytes off", [r.ptr + 4], (1, 1, 2), (2, 2), f64, ERR_ARG),
                                                  ("pitch1 < r2", [base], shape, (ok[0], 7), f32, ERR_ARG),
                                                  ("pitch0 < r1 pitch1", [base], shape, (6 * ok[1] - 1, ok[1]), f32, ERR_ARG),
                                                  ("count x n = 2^32", [base] * 2, (2 ** 11, 2 ** 10, 2 ** 10), (2 ** 20, 2 ** 10), f32, ERR_UNSUP)):
        rc, got, _ = ctx.minmax_batch_view(ptrs, True, shp, pitches, dtype, raise_on_error=False)
        print(f"{what}: rc = {rc}")
        assert rc == want, f"{what}: rc = {rc}, expected {want}"
        assert all(lo == 0.0 and hi == 0.0 for lo, hi in got), f"{what}: a refused call wrote its outputs"
    r.check("refusals")
    assert np.array_equal(r.get(), p.view(np.uint8))
