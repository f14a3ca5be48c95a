"""Sub-boxes of many streams in one call from C: SZ_hip_decompress_batch_regions (include/sz.h) and its Python mirror.  As tests/test_args_batch_shapes.py: every case
runs on the CPU shim (tests/sim) and, marked gpu, on the device, where the destinations sit at guarded device pointers.

The bar is bit for bit, no tolerance: every destination sub-box holds SZ_decompress(stream)[start:end] of this library -- which the other test files pin to the
oracle --, for streams from SZ_hip_compress_args_batch_shapes (three containers and the constant stream it writes for a constant array), and every other byte of every
destination keeps its fill.  An SZ 2.1 stream among the items is refused alone."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ptr_cases as P  # noqa: E402
from test_args_batch import BACKENDS, REL, gpu, init, shim  # noqa: E402,F401
from test_omp_batch_region import Item  # noqa: E402

f32, f64 = np.float32, np.float64
SHAPES = [(8, 64, 64), (16, 16, 16), (16, 16, 16), (8, 24, 16)]           # (the third is the constant array)
CONSTANT = 2
_MADE = {}


@pytest.fixture(params=BACKENDS)
def dev(request, monkeypatch):
    monkeypatch.delenv("SZ_HIP_MODE", raising=False)
    monkeypatch.delenv("SZ_HIP_OMP_THREADS", raising=False)
    request.getfixturevalue("gpu" if request.param == "gpu" else "shim")
    return request.param == "gpu"


def made(dev, dtype):
    """(streams, what SZ_decompress returns for each): the streams of SZ_hip_compress_args_batch_shapes, once per backend and type"""
    import sz_amd
    key = (dev, np.dtype(dtype).name)
    if key not in _MADE:
        from sz_amd.fields import s_field
        arrs = [np.ascontiguousarray(np.full(s, 1.5, dtype=dtype) if i == CONSTANT else s_field(*s, np.dtype(dtype).type, z0=3 * i)) for i, s in enumerate(SHAPES)]
        init()
        rc, streams, batched = sz_amd.SZ_hip_compress_args_batch_shapes([a.ctypes.data for a in arrs], False, SHAPES, dtype, REL, 0.0, 1e-3)
        assert rc == 0 and list(batched) == [1, 1, 0, 1]
        decs = []
        for s, a in zip(streams, arrs):
            init()
            dec = sz_amd.SZ_decompress(s, a.shape, dtype)
            dec.setflags(write=False)
            decs.append(dec)
        init()
        sz21 = sz_amd.SZ_compress_args(arrs[1], sz_amd.ABS, 1e-3)                    # (SZ_HIP_MODE is not set: an SZ 2.1 stream)
        assert sz21[19] != streams[1][19]
        _MADE[key] = (streams, decs, sz21)
    return _MADE[key]


def regions_of(k):
    """items over stream k: a face, an inner box across box boundaries, one value; contiguous and with pitches that are and are not multiples of 16 bytes"""
    n = SHAPES[k]
    inner = ((1, 2, 3), (n[0] - 1, n[1] - 2, n[2] - 4))
    e = [h - l for l, h in zip(*inner)]
    return [Item(k, (0, 0, 0), (n[0], n[1], 2), (n[1] * 8 + 4, 8), 0), Item(k, *inner), Item(k, *inner, ((e[2] + 3) * e[1] + 5, e[2] + 3), 8),
            Item(k, (n[0] - 1, n[1] - 1, n[2] - 1), n)]


def check(dest, it, dec, what, dtype):
    got = dest.get().view(dtype)
    m = it.mask()
    crop = np.ascontiguousarray(dec[it.lo[0]:it.hi[0], it.lo[1]:it.hi[1], it.lo[2]:it.hi[2]])
    assert np.array_equal(P.bits(got[m]), P.bits(crop)), f"{what}: not the crop of SZ_decompress"
    assert (got[~m].view(np.uint8) == P.FILL).all(), f"{what}: bytes between the rows or planes of the sub-box were written"
    dest.check(what)


@pytest.mark.parametrize("out_on_device", (True, False), ids=("device_destinations", "host_destinations"))
@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
def test_crops_of_sz_decompress(dev, dtype, out_on_device):
    import sz_amd
    streams, decs, sz21 = made(dev, dtype)
    esz = np.dtype(dtype).itemsize
    items = [it for k in range(len(SHAPES)) for it in regions_of(k)]
    dests = [P.carve(it.span() * esz, it.off, pad=64, device=dev and out_on_device) for it in items]
    pitches = [(it.p0, it.p1) for it in items]
    init()
    rc = sz_amd.SZ_hip_decompress_batch_regions([streams[it.name] for it in items], [SHAPES[it.name] for it in items], [it.lo for it in items], [it.hi for it in items],
                                                [d.ptr for d in dests], out_on_device, dtype, pitches)
    assert rc == 0
    for i, (it, d) in enumerate(zip(items, dests)):
        check(d, it, decs[it.name], f"item {i} (stream {it.name} {it.lo}-{it.hi} pitches {it.pitches})", dtype)
    st = sz_amd.SZ_hip_last_stats()
    assert st.packing == 1 and st.n_elements == sum(int(np.prod(it.ext)) for it in items if it.name != CONSTANT)
    # contiguous destinations: out_pitches = NULL
    items = [it for it in items if it.pitches is None]
    dests = [P.carve(it.span() * esz, it.off, pad=64, device=dev and out_on_device) for it in items]
    init()
    assert sz_amd.SZ_hip_decompress_batch_regions([streams[it.name] for it in items], [SHAPES[it.name] for it in items], [it.lo for it in items], [it.hi for it in items],
                                                  [d.ptr for d in dests], out_on_device, dtype) == 0
    for i, (it, d) in enumerate(zip(items, dests)):
        check(d, it, decs[it.name], f"contiguous item {i} (stream {it.name} {it.lo}-{it.hi})", dtype)


def test_an_sz21_stream_is_refused_alone(dev):
    import sz_amd
    streams, decs, sz21 = made(dev, f32)
    items = [Item(0, (1, 2, 3), (7, 40, 50)), Item(1, (1, 2, 3), (9, 9, 9)), Item(1, (0, 0, 0), (16, 16, 3), (16 * 4 + 1, 4), 4)]
    given = [streams[0], sz21, streams[1]]
    dests = [P.carve(it.span() * 4, it.off, pad=64, device=dev) for it in items]
    init()
    rc = sz_amd.SZ_hip_decompress_batch_regions(given, [SHAPES[it.name] for it in items], [it.lo for it in items], [it.hi for it in items], [d.ptr for d in dests], True,
                                                f32, [(it.p0, it.p1) for it in items], raise_on_error=False)
    assert rc == sz_amd.SZ_NSCS
    assert (dests[1].get() == P.FILL).all(), "the destination of the refused item was written"
    dests[1].check("refused item")
    for i in (0, 2):
        check(dests[i], items[i], decs[items[i].name], f"beside the refused stream: item {i}", f32)


def test_refusals_of_the_whole_call(dev):
    import sz_amd
    streams, decs, sz21 = made(dev, f32)
    good = Item(1, (1, 2, 3), (9, 9, 9))
    dests = [P.carve(good.span() * 4, 0, pad=64, device=dev) for _ in range(2)]
    ptrs = [d.ptr for d in dests]

    def refused(what, los=None, his=None, out_ptrs=None, pitches=None):
        init()
        rc = sz_amd.SZ_hip_decompress_batch_regions([streams[1]] * 2, [SHAPES[1]] * 2, los or [good.lo] * 2, his or [good.hi] * 2, out_ptrs or ptrs, True, f32, pitches,
                                                    raise_on_error=False)
        assert rc == sz_amd.SZ_NSCS, what
        for d in dests:
            assert (d.get() == P.FILL).all(), f"{what}: a destination was written"
            d.check(what)

    refused("a null destination", out_ptrs=[ptrs[0], None])
    refused("an empty box", los=[good.lo, (2, 2, 2)], his=[good.hi, (2, 5, 5)])
    refused("a box beyond the extent", his=[good.hi, (17, 9, 9)])
    refused("a row pitch below the row", pitches=[(42, 6), (42, 5)])
    refused("a plane pitch below the plane", pitches=[(42, 6), (41, 6)])
