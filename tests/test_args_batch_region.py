"""SZ_compress_args over one box common to many padded parents: SZ_hip_compress_args_batch_region, SZ_hip_decompress_batch_into_region,
SZ_hip_compare_batch_region (include/sz.h) and their Python mirror.  Every case runs on the CPU shim (tests/sim) and, marked gpu, on the device, where the parents sit
at guarded device pointers.

The checker is code the region calls do not change: SZ_hip_compress_args_batch / SZ_hip_decompress_batch on contiguous copies of the sub-boxes, and SZ_hip_compare on
contiguous copies of each pair (tests/test_args_batch.py pins those against the single calls and the oracle).  streams[i] must equal the contiguous call's stream byte
for byte and batched[i] its flag; the decode must write the interior bit for bit and no other byte of a parent; record i must equal SZ_hip_compare's byte for byte.

The parents: the arrays of tests/test_args_batch.py (scaled S-fields, noise, 1e30 and a NaN, a constant array) as the interiors of parents with ghosts (1, 1, 1) --
the float32 column shape is gathered, the float64 box shape runs value by value in place -- whose ghost cells hold garbage larger and smaller than anything inside
(NaNs among it), so a ghost cell that reaches a range, a stream or a record shows."""
import numpy as np
import pytest

import ptr_cases as P
from test_args_batch import ABS, ABS_OR_REL, BOX, COL, PSNR, REL, arrays, dev, f32, f64, gpu, init, shim  # noqa: F401  (dev, gpu, shim: fixtures)
from test_omp_batch import SENTINEL, _bits
from test_omp_batch_view import _garbage, _layout

GHOSTS = (1, 1, 1)
SZ_NSCS = -1


def parents_of(dev, arrs, fill=None):
    """every array as the interior of its own parent; returns (layout, parent shape, lo, hi, numpy parents, regions)"""
    shape = arrs[0].shape
    lay = _layout(shape, GHOSTS)
    pshape = tuple(n + 2 * g for n, g in zip(shape, GHOSTS))
    ps = []
    for i, a in enumerate(arrs):
        if fill is None:
            p = _garbage(lay.total, a.dtype.type, 90 + i)
        else:
            p = np.empty(lay.total, dtype=a.dtype)
            p.view(np.uint32 if a.itemsize == 4 else np.uint64)[:] = fill
        if a is not None and fill is None:
            p[lay.idx] = a.reshape(-1)
        ps.append(p)
    step = arrs[0].itemsize
    regs = [P.carve(p.nbytes, (0, step, 8)[i % 3], pad=256, device=dev).put(p) for i, p in enumerate(ps)]
    return lay, pshape, GHOSTS, tuple(g + n for g, n in zip(GHOSTS, shape)), ps, regs


def contiguous(dev, arrs):
    return [P.carve(a.nbytes, 0, device=dev).put(a) for a in arrs]


def five(shape, dtype):
    named = arrays(shape, dtype)[:5]
    return [k for k, _ in named], [a for _, a in named]


@pytest.mark.parametrize("mode,abs_b,rel", [(ABS, 1e-3, 0.0), (REL, 0.0, 1e-4), (ABS_OR_REL, 1e-3, 1e-4), (PSNR, 0.0, 0.0)], ids=["ABS", "REL", "ABS_OR_REL", "PSNR"])
@pytest.mark.parametrize("shape,dtype", [(COL, f32), (BOX, f64)], ids=["col-f32", "box-f64"])
def test_streams_are_the_contiguous_calls(dev, shape, dtype, mode, abs_b, rel):
    import sz_amd
    names, arrs = five(shape, dtype)
    lay, pshape, lo, hi, ps, regs = parents_of(dev, arrs)
    flat = contiguous(dev, arrs)
    init()
    rc, want, want_batched = sz_amd.SZ_hip_compress_args_batch([r.ptr for r in flat], True, shape, dtype, mode, abs_b, rel)
    assert rc == 0
    sz_amd.SZ_Finalize(); init()
    rc, got, batched = sz_amd.SZ_hip_compress_args_batch_region([r.ptr for r in regs], True, pshape, dtype, lo, hi, mode, abs_b, rel)
    launches = sz_amd.SZ_hip_last_stats().quant_kernel_launches
    assert rc == 0
    for i, k in enumerate(names):
        print(f"item {i} ({k}): {len(got[i])} bytes, batched {batched[i]}")
        assert got[i] == want[i], f"item {i} ({k}): the region call's stream ({len(got[i])} bytes) is not the contiguous call's ({len(want[i])} bytes)"
    assert batched == want_batched and sum(batched) >= 3
    assert 1 <= launches <= 2, launches                                      # (one sweep launch per form and addressing, whatever the count)
    for r, p in zip(regs, ps):
        r.check("input parent")
        assert np.array_equal(r.get(), p.view(np.uint8)), "an input parent was written"
    # host parents: the same streams
    sz_amd.SZ_Finalize(); init()
    rc, host, hb = sz_amd.SZ_hip_compress_args_batch_region([p.ctypes.data for p in ps], False, pshape, dtype, lo, hi, mode, abs_b, rel)
    assert rc == 0 and host == want and hb == want_batched


@pytest.mark.parametrize("shape,dtype", [(COL, f32), (BOX, f64)], ids=["col-f32", "box-f64"])
def test_constant_interior_round_trip_and_report(dev, shape, dtype):
    """ABS 1e-3 over five patches and a constant one: the constant interior (non-constant ghosts) gets the constant stream; everything decodes into the interiors
    only; the report over the round trip equals SZ_hip_compare's of the contiguous copies and finds no point over the bound"""
    import sz_amd
    named = arrays(shape, dtype)[:6]
    names, arrs = [k for k, _ in named], [a for _, a in named]
    assert names[5] == "constant"
    lay, pshape, lo, hi, ps, regs = parents_of(dev, arrs)
    flat = contiguous(dev, arrs)
    init()
    rc, want, want_batched = sz_amd.SZ_hip_compress_args_batch([r.ptr for r in flat], True, shape, dtype, ABS, 1e-3, 0.0)
    rc2, got, batched = sz_amd.SZ_hip_compress_args_batch_region([r.ptr for r in regs], True, pshape, dtype, lo, hi, ABS, 1e-3, 0.0)
    assert rc == 0 and rc2 == 0 and got == want and batched == want_batched
    assert batched[5] == 0 and len(got[5]) == (44 if dtype is f32 else 56) and got[5][3] & 0x01, "the constant interior did not get the constant stream"
    # ---- the decode: contiguous (the checker) and into the interiors of sentinel-filled parents
    esz = np.dtype(dtype).itemsize
    outs = [P.carve(a.nbytes, 0, device=dev) for a in arrs]
    assert sz_amd.SZ_hip_decompress_batch(want, [r.ptr for r in outs], True, shape, dtype) == 0
    dec = [r.get().view(dtype).reshape(shape) for r in outs]
    for on_device in (True, False):
        _, _, _, _, before, tregs = parents_of(dev and on_device, arrs, fill=SENTINEL[esz])
        assert sz_amd.SZ_hip_decompress_batch_into_region(got, [r.ptr for r in tregs], on_device, pshape, dtype, lo, hi) == 0
        for i, r in enumerate(tregs):
            r.check(f"decode {i}")
            now = r.get().view(dtype)
            assert np.array_equal(_bits(now[lay.idx]), _bits(dec[i])), f"item {i} ({names[i]}), on_device {on_device}: the interior differs from the contiguous decode"
            assert np.array_equal(_bits(now[lay.outside]), _bits(before[i][lay.outside])), f"item {i} ({names[i]}), on_device {on_device}: bytes outside the interior were written"
    # ---- the report: originals (garbage ghosts) against decoded parents (sentinel ghosts)
    _, _, _, _, before, tregs = parents_of(dev, arrs, fill=SENTINEL[esz])
    assert sz_amd.SZ_hip_decompress_batch_into_region(got, [r.ptr for r in tregs], True, pshape, dtype, lo, hi) == 0
    recs = sz_amd.SZ_hip_compare_batch_region([r.ptr for r in regs], [r.ptr for r in tregs], True, pshape, dtype, lo, hi, [1e-3] * 6, None, corr=True)
    for i, q in enumerate(recs):
        one = sz_amd.SZ_hip_compare(arrs[i], dec[i], 1e-3, -1.0, corr=True)
        assert q.raw == one.raw, f"pair {i} ({names[i]}): the region report differs from SZ_hip_compare's of the contiguous copies\n{q}\n{one}"
        assert q.n_over_abs == 0 and q.n == arrs[i].size, q
    # a damaged stream: SZ_NSCS, its parent untouched, the others decoded
    _, _, _, _, before, tregs = parents_of(dev, arrs, fill=SENTINEL[esz])
    bad = list(got); bad[1] = bad[1][:-5]
    assert sz_amd.SZ_hip_decompress_batch_into_region(bad, [r.ptr for r in tregs], True, pshape, dtype, lo, hi, raise_on_error=False) == SZ_NSCS
    assert np.array_equal(tregs[1].get(), before[1].view(np.uint8)), "a damaged stream reached its parent"
    assert np.array_equal(_bits(tregs[0].get().view(dtype)[lay.idx]), _bits(dec[0])) and np.array_equal(_bits(tregs[2].get().view(dtype)[lay.idx]), _bits(dec[2]))


def test_a_bound_that_is_not_positive_goes_the_contiguous_calls_way(dev):
    """ABS 0: no item is batched; each goes through SZ_compress_args' ordinary path from a packed copy and ends as it ends in the contiguous call -- the same return
    code, the same streams (today that path refuses a zero bound: both calls return SZ_NSCS and no stream)"""
    import sz_amd
    names, arrs = five(BOX, f32)
    lay, pshape, lo, hi, ps, regs = parents_of(dev, arrs[:2])
    flat = contiguous(dev, arrs[:2])
    init()
    rc, want, wb = sz_amd.SZ_hip_compress_args_batch([r.ptr for r in flat], True, BOX, f32, ABS, 0.0, 0.0, raise_on_error=False)
    rc2, got, gb = sz_amd.SZ_hip_compress_args_batch_region([r.ptr for r in regs], True, pshape, f32, lo, hi, ABS, 0.0, 0.0, raise_on_error=False)
    assert rc2 == rc and got == want and gb == wb == [0, 0]
    rc3, host, hb = sz_amd.SZ_hip_compress_args_batch_region([p.ctypes.data for p in ps], False, pshape, f32, lo, hi, ABS, 0.0, 0.0, raise_on_error=False)
    assert rc3 == rc and host == want and hb == wb
    for r, p in zip(regs, ps):
        r.check("input parent")
        assert np.array_equal(r.get(), p.view(np.uint8)), "an input parent was written"


def test_refusals(dev):
    import sz_amd
    names, arrs = five(BOX, f32)
    lay, pshape, lo, hi, ps, regs = parents_of(dev, arrs[:2])
    init()
    _, streams, _ = sz_amd.SZ_hip_compress_args_batch_region([r.ptr for r in regs], True, pshape, f32, lo, hi, ABS, 1e-3, 0.0)
    ptrs = [r.ptr for r in regs]
    cases = (("an empty box", ptrs, pshape, lo, (hi[0], lo[1], hi[2])), ("a box beyond the extent", ptrs, pshape, lo, (hi[0], hi[1], pshape[2] + 1)),
             ("a parent that is not 3-D", ptrs, (0, pshape[1], pshape[2]), lo, hi), ("a null parent", [ptrs[0], None], pshape, lo, hi), ("count < 1", [], pshape, lo, hi))
    for what, pp, shp, a, b in cases:
        rc, got, batched = sz_amd.SZ_hip_compress_args_batch_region(pp, True, shp, f32, a, b, ABS, 1e-3, 0.0, raise_on_error=False)
        assert rc == SZ_NSCS and all(s is None for s in got) and not any(batched), what
        if pp:
            assert sz_amd.SZ_hip_decompress_batch_into_region(streams[:len(pp)], pp, True, shp, f32, a, b, raise_on_error=False) == SZ_NSCS, what
            with pytest.raises(sz_amd.api.SZError):
                sz_amd.SZ_hip_compare_batch_region(pp, pp, True, shp, f32, a, b, [1.0] * len(pp))
    for r, p in zip(regs, ps):
        r.check("refusals")
        assert np.array_equal(r.get(), p.view(np.uint8)), "a refused call wrote"
