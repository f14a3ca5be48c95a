"""SZ_compress_args over arrays of DIFFERENT shapes in one call: SZ_hip_compress_args_batch_shapes, SZ_hip_decompress_batch_shapes (include/sz.h) and their Python
mirror.  As tests/test_args_batch.py: every case runs on the CPU shim (tests/sim) and, marked gpu, on the device, where the arrays sit at guarded device pointers.

streams[i] is compared with SZ_compress_args of this library under SZ_HIP_MODE=omp for array i alone, as the first call after the same SZ_Init -- the path that
tests/golden/ref_recorded_omp.json pins --, and a container item also with the oracle, independent of the code under test: oracle.omp_compress at the bound the
reference's rule gives for the array's own range, with the box count SZ_HIP_MODE=omp applies to the item's OWN shape.  batched[i] is asserted: 1 exactly for the items
the container takes and whose range exceeds their bound.  The decode is compared bit for bit with SZ_decompress of each stream.

The items: four shapes the container takes (boxes with 32 x 32 faces, 8^3, 4 x 12 x 8, 6^3 under a forced box count of 8; the grids picked from the shapes without one),
a constant array, an array of 20 values and an array no grid divides -- the last two take SZ_compress_args' ordinary path from inside the call."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ptr_cases as P  # noqa: E402
from test_args_batch import ABS_OR_REL, BACKENDS, MARK, PW_REL, REL, bound_of, gpu, init, shim, single  # noqa: E402,F401
from test_omp_batch import _field  # noqa: E402

f32, f64 = np.float32, np.float64
SHAPES = [(8, 64, 64), (16, 16, 16), (2, 2, 5), (8, 24, 16), (16, 16, 16), (3, 5, 7), (12, 12, 12), (8, 24, 16)]      # (the fifth is the constant array)
CONSTANT, TWENTY, NO_GRID = 4, 2, 5
_ARR = {}


@pytest.fixture(params=BACKENDS)
def dev(request, monkeypatch):
    monkeypatch.delenv("SZ_HIP_MODE", raising=False)
    monkeypatch.delenv("SZ_HIP_OMP_THREADS", raising=False)
    request.getfixturevalue("gpu" if request.param == "gpu" else "shim")
    return request.param == "gpu"


def arrays(dtype):
    key = np.dtype(dtype).name
    if key not in _ARR:
        from sz_amd.fields import s_field
        out = []
        for i, shape in enumerate(SHAPES):
            a = np.full(shape, 1.5, dtype=dtype) if i == CONSTANT else (s_field(*shape, np.dtype(dtype).type, z0=3 * i) * dtype((1.0, 1e3, 1e-3)[i % 3])).astype(dtype)
            a = np.ascontiguousarray(a); a.setflags(write=False)
            out.append(a)
        _ARR[key] = out
    return _ARR[key]


def picked_threads(shape, forced):
    """the box count SZ_HIP_MODE=omp applies to a shape (sz_api.c: omp_pick_threads): the forced count where its grid divides the shape, else the first power of two
    whose boxes have faces of at most 1024 rows and at most 32 768 points; 0: no grid.  At most 20 values or an extent below 2: the container does not take it"""
    from test_omp_batch_shapes import grid
    if min(shape) < 2 or int(np.prod(shape)) <= 20:
        return 0
    if forced:
        return forced if grid(shape, forced) else 0
    for o in range(31):
        g = grid(shape, 1 << o)
        n = (1 << o)
        order = n.bit_length() - 1
        bb = order // 3
        nx, ny = [(1 << bb, 1 << bb), (1 << (bb + 1), 1 << bb), (1 << (bb + 1), 1 << (bb + 1))][order % 3]
        if nx > shape[0] or ny > shape[1] or n // (nx * ny) > shape[2]:
            break
        if g and g[1][0] * g[1][1] <= 1024 and g[1][0] * g[1][1] * g[1][2] <= 32768:
            return n
    return 0


@pytest.mark.parametrize("forced", (8, 0), ids=("eight_boxes", "boxes_from_the_shape"))
@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("name,mode,abs_b,rel", [("REL", REL, 0.0, 1e-3), ("ABS_OR_REL", ABS_OR_REL, 1e-3, 1e-3)], ids=("REL", "ABS_OR_REL"))
def test_streams_and_round_trip(dev, oracle, monkeypatch, name, mode, abs_b, rel, dtype, forced):
    import sz_amd
    if forced:
        monkeypatch.setenv("SZ_HIP_OMP_THREADS", str(forced))
    arrs = arrays(dtype)
    esz = np.dtype(dtype).itemsize
    on_device = dtype is f32                                                   # (float64: host arrays, staged one behind the other at their own lengths)
    regs = [P.carve(a.nbytes, (0, esz, 8)[i % 3], device=dev).put(a) for i, a in enumerate(arrs)] if on_device else None
    ptrs = [r.ptr for r in regs] if on_device else [a.ctypes.data for a in arrs]
    init()
    rc, streams, batched = sz_amd.SZ_hip_compress_args_batch_shapes(ptrs, on_device, SHAPES, dtype, mode, abs_b, rel)
    assert rc == 0
    if regs:
        for r, a in zip(regs, arrs):
            r.check("input")
            assert np.array_equal(r.get(), a.reshape(-1).view(np.uint8)), "an input was written"
    want_batched = []
    for i, a in enumerate(arrs):
        what = f"{name} {np.dtype(dtype).name} item {i} {a.shape}"
        threads = picked_threads(a.shape, forced)
        rng, eb = bound_of(a, mode, abs_b, rel)
        container = threads > 0 and rng > eb
        want_batched.append(1 if container else 0)
        print(f"{what}: {threads} boxes, range {rng!r}, bound {eb!r}, batched {batched[i]}, {len(streams[i])} bytes")
        one = single(a, mode, abs_b, rel, monkeypatch)
        assert streams[i] == one, f"{what}: the batch's stream ({len(streams[i])} bytes) is not SZ_compress_args' ({len(one)} bytes)"
        if container:
            assert streams[i][19] == MARK
            assert int.from_bytes(streams[i][32:36], "big") == threads, what
            assert streams[i] == oracle.omp_compress(a, eb, threads, streams[i][:32]), f"{what}: not the oracle's container at the bound {eb!r}"
        elif threads > 0:
            assert streams[i] == oracle.compress(a, mode, abs_b, rel)[0], f"{what}: not the oracle's constant stream"
    # (3, 5, 7): a forced count of 8 finds no grid; picked from the shape it is one box of 105 points, which the container takes -- through its single call
    assert want_batched[CONSTANT] == 0 and want_batched[TWENTY] == 0 and (want_batched[NO_GRID] == 0 or not forced) and sum(want_batched) >= len(SHAPES) - 3
    assert list(batched) == want_batched, f"batched = {list(batched)}, the container's items with range > bound are {want_batched}"
    # the inverse: bit for bit SZ_decompress of each stream, nothing else written
    outs = [P.carve(a.nbytes, (8, 0, esz)[i % 3], device=dev).put(np.zeros(a.shape, dtype)) for i, a in enumerate(arrs)]
    init()
    assert sz_amd.SZ_hip_decompress_batch_shapes(streams, [r.ptr for r in outs], True, SHAPES, dtype) == 0
    for i, (a, s, r) in enumerate(zip(arrs, streams, outs)):
        r.check(f"output {i}")
        init()
        ref = sz_amd.SZ_decompress(s, a.shape, dtype)
        assert np.array_equal(P.bits(r.get().view(dtype)), P.bits(ref)), f"item {i}: the batched decode differs from SZ_decompress"
    damaged = list(streams)
    damaged[3] = damaged[3][:len(damaged[3]) // 2]
    outs = [P.carve(a.nbytes, 0, device=dev).put(np.zeros(a.shape, dtype)) for a in arrs]
    init()
    assert sz_amd.SZ_hip_decompress_batch_shapes(damaged, [r.ptr for r in outs], True, SHAPES, dtype, raise_on_error=False) == sz_amd.SZ_NSCS
    for i, (a, s, r) in enumerate(zip(arrs, streams, outs)):
        r.check(f"output {i} beside a damaged stream")
        if i != 3:
            init()
            assert np.array_equal(P.bits(r.get().view(dtype)), P.bits(sz_amd.SZ_decompress(s, a.shape, dtype))), f"stream {i} did not decode beside the damaged one"


def test_refusals(dev):
    import sz_amd
    a = arrays(f32)[1]
    r = P.carve(a.nbytes, 0, device=dev).put(a)
    init()
    for what, shapes, mode in (("a PW_REL mode", [a.shape], PW_REL), ("an extent of 0", [(16, 0, 16)], REL)):
        rc, streams, _ = sz_amd.SZ_hip_compress_args_batch_shapes([r.ptr], True, shapes, f32, mode, 1e-3, 1e-3, raise_on_error=False)
        assert rc == sz_amd.SZ_NSCS and streams == [None], what
    r.check("refused calls")
