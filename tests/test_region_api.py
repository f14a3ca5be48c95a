"""The region calls of the drop-in API: SZ_hip_decompress_region (include/sz.h) on the streams SZ_compress_args writes under SZ_HIP_MODE=omp, bare and behind
the zstd stage, and sz_slab_decompress_region (include/sz_slab_region.h) on slab containers of OpenMP and of SZ 2.1 sub-streams.  The bar: bit for bit the crop of what
this library's SZ_decompress / sz_slab_decompress returns for the same bytes.  CPU shim (tests/sim) and, marked gpu, the built library."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIONS = [((1, 2, 3), (5, 7, 6)), ((0, 0, 0), (16, 32, 64)), ((3, 9, 17), (14, 25, 50)), ((8, 16, 32), (16, 32, 64)), ((15, 31, 63), (16, 32, 64)), ((0, 5, 0), (16, 6, 64))]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _crop(a, lo, hi):
    return a[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]


def _region_call(sz, monkeypatch):
    from sz_amd.fields import s_field
    for config in ("sz_speed.config", None):                                  # SZ_BEST_SPEED: the bare stream; the default configuration wraps it with zstd
        assert sz.SZ_Init(os.path.join(ROOT, "tests", "golden", config) if config else None) == 0
        try:
            for d, eb in ((s_field(16, 32, 64), 1e-4), (s_field(16, 32, 64, np.float64), 1e-6)):
                monkeypatch.setenv("SZ_HIP_MODE", "omp")
                monkeypatch.setenv("SZ_HIP_OMP_THREADS", "8")
                got = sz.SZ_compress_args(d, sz.ABS, eb)
                assert (got[19] == 0x4F) == (config is not None) and (got[:4] == b"\x28\xb5\x2f\xfd") == (config is None)
                whole = sz.SZ_decompress(got, d.shape, d.dtype)
                for lo, hi in REGIONS:
                    part = sz.SZ_hip_decompress_region(got, d.shape, d.dtype, lo, hi)
                    assert part.shape == tuple(h - l for l, h in zip(lo, hi))
                    assert np.array_equal(_bits(part), _bits(_crop(whole, lo, hi))), (config, d.dtype, lo, hi)
                assert sz.SZ_hip_last_stats().n_blocks == 4                    # (the last region: one row of the 2 x 2 x 2 grid in dim 1)
                for lo, hi in (((2, 2, 2), (2, 5, 5)), ((0, 0, 0), (17, 32, 64))):
                    with pytest.raises(sz.SZError):
                        sz.SZ_hip_decompress_region(got, d.shape, d.dtype, lo, hi)
                # the same array without the variable: an SZ 2.1 stream, refused; a 2-D array, refused
                monkeypatch.delenv("SZ_HIP_MODE")
                plain = sz.SZ_compress_args(d, sz.ABS, eb)
                assert plain != got and sz.SZ_decompress(plain, d.shape, d.dtype).shape == d.shape
                with pytest.raises(sz.SZError):
                    sz.SZ_hip_decompress_region(plain, d.shape, d.dtype, (1, 2, 3), (5, 7, 6))
                flat = np.ascontiguousarray(d[0])
                got2 = sz.SZ_compress_args(flat, sz.ABS, eb)
                L = sz.lib()
                buf = ctypes.create_string_buffer(got2, len(got2))
                lo3, hi3 = (ctypes.c_size_t * 3)(0, 0, 0), (ctypes.c_size_t * 3)(1, 4, 4)
                assert not L.SZ_hip_decompress_region(0 if d.dtype == np.float32 else 1, buf, len(got2), 0, 0, 0, 32, 64, lo3, hi3)
        finally:
            sz.SZ_Finalize()


def _refusal_names_the_mode(sz, capfd):
    from sz_amd.fields import s_field
    assert sz.SZ_Init(os.path.join(ROOT, "tests", "golden", "sz_speed.config")) == 0
    try:
        d = s_field(16, 32, 64)
        plain = sz.SZ_compress_args(d, sz.ABS, 1e-4)
        capfd.readouterr()
        with pytest.raises(sz.SZError):
            sz.SZ_hip_decompress_region(plain, d.shape, d.dtype, (1, 2, 3), (5, 7, 6))
        ctypes.CDLL(None).fflush(None)                                        # (the C library's printf)
        assert "SZ_HIP_MODE=omp" in capfd.readouterr().out
    finally:
        sz.SZ_Finalize()


def _slab_region(sz, monkeypatch):
    from sz_amd.fields import s_field
    assert sz.SZ_Init(os.path.join(ROOT, "tests", "golden", "sz_speed.config")) == 0
    try:
        d = s_field(36, 32, 32)
        regions = [((2, 3, 4), (9, 20, 30)), ((13, 0, 0), (24, 32, 32)), ((5, 7, 9), (31, 25, 32)), ((11, 0, 16), (25, 16, 32)), ((35, 31, 31), (36, 32, 32)), ((0, 0, 0), (36, 32, 32))]
        for omp in (True, False):
            if omp:
                monkeypatch.setenv("SZ_HIP_MODE", "omp")
                monkeypatch.setenv("SZ_HIP_OMP_THREADS", "4")               # a 2 x 2 x 1 grid divides the slabs of 12 planes
            else:
                monkeypatch.delenv("SZ_HIP_MODE", raising=False); monkeypatch.delenv("SZ_HIP_OMP_THREADS", raising=False)
            blob = sz.sz_slab_compress(d, 3, sz.ABS, 1e-4)
            n = int.from_bytes(blob[8:12], "little")
            off = 40 + 24 * n
            marks = []
            for r in range(n):
                z0, z1, nb = (int.from_bytes(blob[40 + 24 * r + 8 * k:48 + 24 * r + 8 * k], "little") for k in range(3))
                marks.append(blob[off + 19] == 0x4F and bool(blob[off + 3] & 0x80)); off += nb
            assert n == 3 and marks == [omp] * 3
            whole = sz.sz_slab_decompress(blob)
            assert whole.shape == d.shape and float(np.abs(whole.astype(np.float64) - d).max()) <= 1e-4
            for lo, hi in regions:
                part = sz.sz_slab_decompress_region(blob, lo, hi)
                assert np.array_equal(_bits(part), _bits(_crop(whole, lo, hi))), (omp, lo, hi)
            if omp:
                sz.sz_slab_decompress_region(blob, (13, 1, 1), (14, 5, 5))
                assert sz.SZ_hip_last_stats().n_blocks == 1                  # one slab, one box of it
            for lo, hi in (((4, 0, 0), (4, 8, 8)), ((0, 0, 0), (37, 32, 32))):
                with pytest.raises(sz.SZError):
                    sz.sz_slab_decompress_region(blob, lo, hi)
            with pytest.raises(sz.SZError):                                  # the container checks of sz_slab_decompress
                sz.sz_slab_decompress_region(blob[:50], (0, 0, 0), (1, 1, 1))
            bad = bytearray(blob); bad[40 + 24:40 + 32] = (13).to_bytes(8, "little")        # a gap between the first two slabs
            with pytest.raises(sz.SZError):
                sz.sz_slab_decompress_region(bytes(bad), (0, 0, 0), (1, 1, 1))
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


def test_region_call_on_cpu_shim(shim_sz, monkeypatch):
    _region_call(shim_sz, monkeypatch)


def test_region_refusal_names_the_mode_on_cpu_shim(shim_sz, capfd):
    _refusal_names_the_mode(shim_sz, capfd)


def test_slab_region_on_cpu_shim(shim_sz, monkeypatch):
    _slab_region(shim_sz, monkeypatch)


@pytest.mark.gpu
def test_hip_region_call(built, monkeypatch):
    import sz_amd
    _region_call(sz_amd, monkeypatch)


@pytest.mark.gpu
def test_hip_region_refusal_names_the_mode(built, capfd):
    import sz_amd
    _refusal_names_the_mode(sz_amd, capfd)


@pytest.mark.gpu
def test_hip_slab_region(built, monkeypatch):
    import sz_amd
    _slab_region(sz_amd, monkeypatch)
