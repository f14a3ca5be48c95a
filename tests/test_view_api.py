"""The view calls of the drop-in API (include/sz.h): SZ_hip_compress_region compresses a sub-box of a larger host array where it lies, SZ_hip_decompress_into_region
decodes into one.  The bar: the bytes are those SZ_compress_args returns for np.ascontiguousarray(parent[lo:hi]) under the same configuration -- SZ 2.1, SZ 1.4
(withLinearRegression = NO) and SZ_HIP_MODE=omp, bare and behind the zstd stage, ABS and REL (the range is the sub-box's: the parent's halo holds 1e30) --; the decode
writes bit for bit what SZ_decompress returns into the sub-box of a parent pre-filled with a NaN pattern, and nothing else.  CPU shim (tests/sim) and, marked gpu,
the built library."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT, LO, HI = (20, 36, 70), (2, 3, 5), (18, 35, 69)
SENTINEL = {4: 0x7FC0DEAD, 8: 0x7FF8DEAD0000BEEF}


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _crop(a, lo=LO, hi=HI):
    return a[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]


def _parent_of(sub, fill=1e30):
    p = np.full(PARENT, fill, dtype=sub.dtype)
    _crop(p)[...] = sub
    return p


def _sentinel_parent(dtype):
    p = np.empty(PARENT, dtype=dtype)
    p.view(np.uint32 if p.itemsize == 4 else np.uint64)[...] = SENTINEL[p.itemsize]
    return p


def _round_trip(sz, parent, mode, what, **bounds):
    """compress the sub-box where it lies, compare with the contiguous call; decode it into a sentinel parent, compare with SZ_decompress"""
    sub = np.ascontiguousarray(_crop(parent))
    before = parent.copy()
    want = sz.SZ_compress_args(sub, mode, **bounds)
    got = sz.SZ_hip_compress_region(parent, LO, HI, mode, **bounds)
    assert got == want, f"{what}: {len(got)} / {len(want)} bytes"
    assert np.array_equal(_bits(parent), _bits(before)), f"{what}: the parent was written"
    dec = sz.SZ_decompress(want, sub.shape, sub.dtype)
    into = _sentinel_parent(sub.dtype)
    expect = into.copy(); _crop(expect)[...] = dec
    sz.SZ_hip_decompress_into_region(want, into, LO, HI)
    assert np.array_equal(_bits(_crop(into)), _bits(dec)), f"{what}: the decoded sub-box differs from SZ_decompress"
    assert np.array_equal(_bits(into), _bits(expect)), f"{what}: the parent was written outside the sub-box"
    return got


def _view_calls(sz, monkeypatch):
    from sz_amd.fields import s_field
    for config in ("sz_speed.config", None):                                  # SZ_BEST_SPEED: the bare stream; the default configuration wraps it with zstd
        for kind in ("sz21", "omp", "sz14"):
            assert sz.SZ_Init(os.path.join(ROOT, "tests", "golden", config) if config else None) == 0
            try:
                monkeypatch.delenv("SZ_HIP_MODE", raising=False); monkeypatch.delenv("SZ_HIP_OMP_THREADS", raising=False)
                if kind == "omp":
                    monkeypatch.setenv("SZ_HIP_MODE", "omp"); monkeypatch.setenv("SZ_HIP_OMP_THREADS", "8")
                sz.conf_params().withRegression = 0 if kind == "sz14" else 1
                for sub, eb in ((s_field(16, 32, 64), 1e-4), (s_field(16, 32, 64, np.float64), 1e-6)):
                    parent = _parent_of(sub)
                    what = f"{config} {kind} {sub.dtype}"
                    got = _round_trip(sz, parent, sz.ABS, what + " ABS", absErrBound=eb)
                    assert (got[:4] == b"\x28\xb5\x2f\xfd") == (config is None), what
                    if config is not None:
                        assert (got[19] == 0x4F) == (kind == "omp") and bool(got[3] & 0x80) == (kind != "sz14"), what
                    rel = _round_trip(sz, parent, sz.REL, what + " REL", relBoundRatio=1e-3)
                    assert rel != got
            finally:
                sz.SZ_Finalize()


def _constant_and_refusals(sz):
    assert sz.SZ_Init(os.path.join(ROOT, "tests", "golden", "sz_speed.config")) == 0
    try:
        for dtype in (np.float32, np.float64):
            from sz_amd.fields import s_field
            parent = s_field(*PARENT, dtype)                                  # a constant sub-box inside a parent that is not: the constant stream
            _crop(parent)[...] = 1.5
            got = _round_trip(sz, parent, sz.ABS, f"constant {np.dtype(dtype).name}", absErrBound=1e-4)
            assert got[3] & 0x01 and len(got) == 4 + (28 if dtype == np.float32 else 36) + 8 + np.dtype(dtype).itemsize
            sub = s_field(16, 32, 64, dtype)
            stream = sz.SZ_compress_args(sub, sz.ABS, 1e-4)
            L = sz.lib()
            n = ctypes.c_size_t(0)
            buf = ctypes.create_string_buffer(stream, len(stream))
            dt = 0 if dtype == np.float32 else 1
            box = lambda lo, hi: ((ctypes.c_size_t * 3)(*lo), (ctypes.c_size_t * 3)(*hi))      # noqa: E731
            for dims, lo, hi in (((0, 0, 0, 36, 70), (0, 0, 0), (1, 4, 4)),                     # a 2-D parent
                                 ((0, 0) + PARENT, (2, 3, 5), (2, 35, 69)),                    # an empty box
                                 ((0, 0) + PARENT, (2, 3, 5), (18, 35, 71)),                   # beyond the parent
                                 ((0, 0) + PARENT, (5, 3, 5), (21, 35, 69))):
                parent = _sentinel_parent(dtype)
                before = parent.copy()
                assert not L.SZ_hip_compress_region(dt, parent.ctypes.data, ctypes.byref(n), sz.ABS, 1e-4, 0.0, 0.0, *dims, *box(lo, hi)), (dims, lo, hi)
                assert L.SZ_hip_decompress_into_region(dt, buf, len(stream), parent.ctypes.data, *dims, *box(lo, hi)) == sz.SZ_NSCS, (dims, lo, hi)
                assert np.array_equal(_bits(parent), _bits(before)), (dims, lo, hi)
            parent = _sentinel_parent(dtype)                                  # a stream that does not decode: nothing written
            before = parent.copy()
            with pytest.raises(sz.SZError):
                sz.SZ_hip_decompress_into_region(stream[:len(stream) // 2], parent, LO, HI)
            assert np.array_equal(_bits(parent), _bits(before))
    finally:
        sz.SZ_Finalize()


@pytest.fixture()
def shim_sz(built):
    import sim_lib
    import sz_amd
    from sz_amd import api
    saved = api._lib
    api._lib = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    yield sz_amd
    api._lib = saved


def test_view_calls_on_cpu_shim(shim_sz, monkeypatch):
    _view_calls(shim_sz, monkeypatch)


def test_view_constant_and_refusals_on_cpu_shim(shim_sz):
    _constant_and_refusals(shim_sz)


@pytest.mark.gpu
def test_hip_view_calls(built, monkeypatch):
    import sz_amd
    _view_calls(sz_amd, monkeypatch)


@pytest.mark.gpu
def test_hip_view_constant_and_refusals(built):
    import sz_amd
    _constant_and_refusals(sz_amd)
