"""The error report for many pairs of same-shape sub-boxes in one call: szhip_compare_batch_view (include/szhip.h) and HipContext.compare_batch_view.  Kernels:
k_quality_pass1_batch_view / k_quality_pass2_batch_view of sz_amd/csrc/szh_quality.h, around the bodies the single call's kernels wrap.

Every case runs twice: on the device (-m gpu) and through the HIP-on-CPU shim (tests/sim).

The bar: record i of the batch equals, BYTE FOR BYTE, what szhip_compare returns for contiguous copies of pair i alone -- without and with the correlation; that
call is existing code -- and what szhip_compare_view returns for the pair where it lies; its exact fields meet `reference()` of tests/test_quality.py.  The parents
are the padded arrays of tests/test_omp_batch_view.py with garbage (NaNs, 1e30) in the ghost cells: a read outside a box shows in the record.  The originals and
the decoded copies have DIFFERENT ghost widths, so the two sides take different pitches and alignments.  Inputs and guard bytes are compared afterwards.

Sizes: boxes either side of the grid rule of the single call (szh_quality_grid, tests/test_quality.py): one workgroup's share is 8192 float32 / 4096 float64 points
-- 16^3 fits one workgroup, 8 x 64 x 64 takes four (float32) --, rows that are no multiple of a 16-byte piece so that pieces cross row ends, rows shorter than a piece."""
import ctypes

import numpy as np
import pytest

import ptr_cases as P
from test_omp_batch_view import _garbage, _layout
from test_quality import assert_exact, pair, reference

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


def make_batch(shape, dtype, count):
    """`count` pairs with bounds of their own (as tests/test_quality_batch.py): pair 0 over its absolute bound at exactly one known point, pair 1 at none, NaN and inf
    points in pair 2"""
    n = int(np.prod(shape))
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
        oris.append(o.reshape(shape)), decs.append(d.reshape(shape)), abs_b.append(ab), pwr_b.append(pb)
    return oris, decs, abs_b, pwr_b


def put_parents(dev, boxes, lay, offs, seed):
    parents = []
    for i, b in enumerate(boxes):
        p = _garbage(lay.total, b.dtype.type, seed + i)
        p[lay.idx] = b.reshape(-1)
        parents.append(p)
    return parents, [P.carve(p.nbytes, o, pad=256, device=dev).put(p) for p, o in zip(parents, offs)]


def check_batch(env, oris, decs, abs_b, pwr_b, corr, o_pad, d_pad, what, on_device=True, far_ghost=True):
    """the batch against the single calls byte for byte and against the reference's loop; parents and guards unchanged"""
    ctx, dev = env
    dtype, shape, count = oris[0].dtype.type, oris[0].shape, len(oris)
    step = np.dtype(dtype).itemsize
    lo, ld = _layout(shape, o_pad[0], o_pad[1], far_ghost), _layout(shape, d_pad[0], d_pad[1], far_ghost)
    po, ro = put_parents(dev and on_device, oris, lo, [(0, step, 8)[i % 3] for i in range(count)], 200)
    pd, rd = put_parents(dev and on_device, decs, ld, [(8, 0, step)[i % 3] for i in range(count)], 300)
    bo, bd = [r.ptr + lo.lead * step for r in ro], [r.ptr + ld.lead * step for r in rd]
    rc, got, st = ctx.compare_batch_view(bo, lo.pitches, bd, ld.pitches, on_device, shape, dtype, abs_b, pwr_b, corr=corr)
    assert rc == 0
    assert st.quant_kernel_launches == 1, f"{what}: {st.quant_kernel_launches} pass-1 launches for {count} pairs"
    for i in range(count):
        co, cd = P.carve(oris[i].nbytes, 0, device=dev).put(oris[i]), P.carve(decs[i].nbytes, 0, device=dev).put(decs[i])
        one = ctx.compare(co.ptr, cd.ptr, True, oris[i].size, dtype, abs_b[i], pwr_b[i] if pwr_b is not None else -1.0, corr=corr)
        assert got[i].raw == one.raw, f"{what} pair {i}: the batch's record differs from szhip_compare's on the contiguous copies\n{got[i]}\n{one}"
        view = ctx.compare_view(bo[i], lo.pitches, bd[i], ld.pitches, on_device, shape, dtype, abs_b[i], pwr_b[i] if pwr_b is not None else -1.0, corr=corr)
        assert got[i].raw == view.raw, f"{what} pair {i}: the batch's record differs from szhip_compare_view's"
        assert_exact(got[i], reference(oris[i], decs[i], abs_b[i], pwr_b[i] if pwr_b is not None else -1.0), f"{what} pair {i}")
    for r, p in zip(ro + rd, po + pd):
        r.check(what)
        assert np.array_equal(r.get(), p.view(np.uint8)), f"{what}: a parent was written"
    return got


SHAPES = [(8, 64, 64), (16, 16, 16), (12, 10, 14), (3, 5, 7), (4, 3, 1), (2, 3, 1030)]
PADS = [(((1, 1, 1), 0), ((2, 3, 4), 0)), (((2, 3, 4), 5), ((0, 0, 2), 0)), (((2, 2, 2), 0), ((0, 0, 0), 0))]


@pytest.mark.parametrize("corr", (False, True), ids=("plain", "corr"))
@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_records_are_the_single_calls(env, shape, dtype, corr):
    n = int(np.prod(shape))
    oris, decs, abs_b, pwr_b = make_batch(shape, dtype, 4)
    for o_pad, d_pad in PADS:
        got = check_batch(env, oris, decs, abs_b, pwr_b, corr, o_pad, d_pad, f"{dtype.__name__} {shape} ghosts {o_pad} / {d_pad}")
        assert got[0].n_over_abs == 1 and got[0].first_over_idx == n // 3 and got[0].max_abs_idx == n // 3, f"pair 0: {got[0]}"
        assert got[1].n_over_abs == 0, f"pair 1: {got[1]}"
        assert got[2].n_excluded == (3 if n > 9 else 0), f"pair 2: {got[2]}"


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("count", (1, 2, 5))
def test_counts_host_parents_the_far_end_and_the_contiguous_call(env, dtype, count):
    ctx, dev = env
    shape = (16, 16, 16)
    oris, decs, abs_b, pwr_b = make_batch(shape, dtype, count)
    pads = (((1, 1, 1), 0), ((2, 3, 4), 0))
    want = check_batch(env, oris, decs, abs_b, pwr_b, True, *pads, f"{count} pairs")
    far = check_batch(env, oris, decs, abs_b, pwr_b, True, *pads, f"{count} pairs, no ghost behind", far_ghost=False)
    host = check_batch(env, oris, decs, abs_b, pwr_b, True, *pads, f"{count} pairs on the host", on_device=False)
    assert [g.raw for g in far] == [w.raw for w in want] and [g.raw for g in host] == [w.raw for w in want]
    none = check_batch(env, oris, decs, abs_b, None, False, *pads, f"{count} pairs, no point-wise bound")
    assert all(g.n_over_pwr == 0 and g.n_over_both == 0 for g in none), "pw_rel_bound == NULL is 'not asked'"
    # contiguous pitches on both sides: the contiguous batch call
    ro = [P.carve(a.nbytes, 0, device=dev).put(a) for a in oris]
    rd = [P.carve(a.nbytes, np.dtype(dtype).itemsize, device=dev).put(a) for a in decs]
    flat = (shape[1] * shape[2], shape[2])
    rc1, a, _ = ctx.compare_batch([r.ptr for r in ro], [r.ptr for r in rd], True, oris[0].size, dtype, abs_b, pwr_b, corr=True)
    rc2, b, st = ctx.compare_batch_view([r.ptr for r in ro], flat, [r.ptr for r in rd], flat, True, shape, dtype, abs_b, pwr_b, corr=True)
    assert rc1 == 0 and rc2 == 0 and st.quant_kernel_launches == 1
    assert [g.raw for g in a] == [g.raw for g in b] == [w.raw for w in want]


def test_refusals(env):
    ctx, dev = env
    shape = (4, 6, 8)
    lay = _layout(shape, ((1, 1, 1)))
    p = _garbage(lay.total, f32, 1)
    ro, rd = P.carve(p.nbytes, 0, device=dev).put(p), P.carve(p.nbytes, 0, device=dev).put(p)
    bo, bd = ro.ptr + lay.lead * 4, rd.ptr + lay.lead * 4
    ok = lay.pitches
    for what, op, dp, shp, opitch, dpitch, dtype, want in (
            ("count < 1", [], [], shape, ok, ok, f32, ERR_ARG), ("an empty box", [bo], [bd], (4, 6, 0), ok, ok, f32, ERR_ARG),
            ("a null ori", [bo, None], [bd, bd], shape, ok, ok, f32, ERR_ARG), ("a null dec", [bo], [None], shape, ok, ok, f32, ERR_ARG),
            ("dec 2 bytes off", [bo], [bd + 2], shape, ok, ok, f32, ERR_ARG), ("ori 4 bytes off, float64", [ro.ptr + 4], [rd.ptr], (1, 1, 2), (2, 2), (2, 2), f64, ERR_ARG),
            ("ori pitch1 < r2", [bo], [bd], shape, (ok[0], 7), ok, f32, ERR_ARG), ("dec pitch0 < r1 pitch1", [bo], [bd], shape, ok, (6 * ok[1] - 1, ok[1]), f32, ERR_ARG),
            ("count x n = 2^32", [bo] * 2, [bd] * 2, (2 ** 11, 2 ** 10, 2 ** 10), (2 ** 20, 2 ** 10), (2 ** 20, 2 ** 10), f32, ERR_UNSUP)):
        rc, got, _ = ctx.compare_batch_view(op, opitch, dp, dpitch, True, shp, dtype, [1.0] * max(len(op), 1), None, raise_on_error=False)
        print(f"{what}: rc = {rc}")
        assert rc == want, f"{what}: rc = {rc}, expected {want}"
        assert all(g.raw == bytes(len(g.raw)) for g in got), f"{what}: a refused call wrote its records"
    for r in (ro, rd):
        r.check("refusals")
        assert np.array_equal(r.get(), p.view(np.uint8))
