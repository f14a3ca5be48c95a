"""A sub-box of an OpenMP-container stream: szhip_decompress_omp_region (include/szhip.h) decodes only the boxes that meet the region.

The bar: the values are bit for bit oracle.omp_decompress(stream)[lo0:hi0, lo1:hi1, lo2:hi2] -- NaN payloads and signed zeros included --, for
streams made by oracle.omp_compress.  No tolerance.  The same groups of cases run on the CPU shim (tests/sim) and, under -m gpu, through the
built library; one group of larger arrays runs on the GPU only."""
import ctypes

import numpy as np
import pytest

import ptr_cases

META = bytes(range(1, 33))
_STREAMS = {}        # name -> (array, stream, the oracle's decoded array): computed once, never changed


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _special(shape, dtype):
    """zeros of both signs, a NaN, an infinity, values far outside the quantiser's range, a constant stretch (as tests/test_zz_omp_hip.py)"""
    from sz_amd.fields import s_field
    d = s_field(*shape, np.dtype(dtype).type)
    f = d.ravel()
    f[3] = 0.0; f[4] = -0.0; f[5] = 1e30; f[6] = -1e30; f[40:90] = -0.0; f[100:400] = 0.25
    f[f.size // 2] = np.nan; f[f.size // 2 + 7] = np.inf
    return d


def _array(name):
    from sz_amd.fields import m_field, s_field
    rng = np.random.default_rng
    if name == "noisy":              # col-one-noisy-box-t16 of tests/test_zz_omp_hip.py: a 4 x 2 x 2 grid of boxes 2 x 32 x 64; boxes (*, 0, 0) hold the noise
        mix = s_field(8, 64, 128); mix[:, :32, 32:64] = (rng(8).standard_normal((8, 32, 32)) * 3).astype(np.float32)
        return mix, 1e-4, 16, 0
    return {"box": lambda: (s_field(16, 16, 16), 1e-3, 8, 0),                                  # 2 x 2 x 2 boxes of 8^3: k_omp_box
            "f64-rows7": lambda: (s_field(12, 10, 14, np.float64), 1e-3, 8, 0),                # boxes 6 x 5 x 7: scalar rows
            "rows18": lambda: (s_field(8, 8, 18), 1e-3, 4, 0),                                 # unaligned code rows
            "col": lambda: (s_field(8, 64, 64), 1e-3, 8, 0),                                   # boxes 4 x 32 x 32: k_omp_col
            "col-f64": lambda: (s_field(8, 64, 64, np.float64), 1e-5, 8, 0),
            "m32": lambda: (np.ascontiguousarray(m_field(32)), 1e-6, 8, 0),                    # most values verbatim
            "col-m": lambda: (np.ascontiguousarray(m_field(64)[:8]), 1e-6, 8, 0),
            "special-f32": lambda: (_special((16, 16, 32), np.float32), 1e-3, 8, 0),
            "special-f64": lambda: (_special((16, 16, 32), np.float64), 1e-3, 8, 64),
            "col-special-f32": lambda: (_special((8, 64, 64), np.float32), 1e-3, 8, 0),
            "col-special-f64": lambda: (_special((8, 64, 64), np.float64), 1e-3, 8, 64),
            "constant": lambda: (np.full((16, 16, 16), 1.5, dtype=np.float32), 1e-3, 8, 0),    # one-symbol book, empty payloads
            "wide-codes": lambda: ((rng(5).standard_normal((16, 16, 32)) * 50).astype(np.float32), 1e-3, 8, 65536),
            "wide-codes-one-box": lambda: ((rng(6).standard_normal((32, 32, 32)) * 50).astype(np.float32), 1e-3, 1, 65536),
            "s128": lambda: (s_field(128, 128, 128), 1e-4, 64, 0)}[name]()                      # GPU only: 64 boxes of 32^3


def _stream(oracle, name):
    if name not in _STREAMS:
        d, eb, threads, iv = _array(name)
        p = oracle.default_params(); p.quantization_intervals = iv
        s = oracle.omp_compress(d, eb, threads, META, p)
        want = oracle.omp_decompress(s, len(META), d.shape, d.dtype)
        want.setflags(write=False)
        _STREAMS[name] = (d, s, want)
    return _STREAMS[name]


def _region(ctx, stream, shape, dtype, lo, hi):
    """the call with everything on the host -> (array, stats)"""
    out = np.empty(tuple(h - l for l, h in zip(lo, hi)), dtype=dtype)
    buf = ctypes.create_string_buffer(stream, len(stream))
    st = ctx.decompress_omp_region(ctypes.addressof(buf), False, len(stream), len(META), shape, dtype, lo, hi, out.ctypes.data, False)
    return out, st


def _crop(want, lo, hi):
    return want[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]


def _grid(thread_num):
    """the box grid of thread_num (sz/src/sz_omp.c:88-117)"""
    order = thread_num.bit_length() - 1
    bb = order // 3
    nx, ny = [(1 << bb, 1 << bb), (2 << bb, 1 << bb), (2 << bb, 2 << bb)][order % 3]
    return nx, ny, thread_num // (nx * ny)


def _covered(shape, nb, lo, hi):
    """the numbers of the boxes that meet [lo, hi), in the order of the stream's tables"""
    grid = _grid(nb)
    c = [n // g for n, g in zip(shape, grid)]
    rng = [range(l // k, (h - 1) // k + 1) for l, h, k in zip(lo, hi, c)]
    return [(bi * grid[1] + bj) * grid[2] + bk for bi in rng[0] for bj in rng[1] for bk in rng[2]]


def _check(ctx, oracle, name, lo, hi):
    d, s, want = _stream(oracle, name)
    out, st = _region(ctx, s, d.shape, d.dtype, lo, hi)
    assert np.array_equal(_bits(out), _bits(_crop(want, lo, hi))), (name, lo, hi)
    nb, ucount, _, _ = _tables(s, d.dtype)
    boxes = _covered(d.shape, nb, lo, hi)
    assert st.n_elements == out.size and st.n_blocks == len(boxes) and st.n_unpred == int(ucount[boxes].sum()), (name, lo, hi)
    return st


def _tables(stream, dtype):
    """(nb, ucount[nb], offset of the payload-size table, offset of the payloads) of a stream behind META"""
    nb = int.from_bytes(stream[len(META):len(META) + 4], "big")
    esz = np.dtype(dtype).itemsize
    tree_bytes = int.from_bytes(stream[len(META) + 8 + esz:len(META) + 12 + esz], "big")
    at = len(META) + 16 + esz + tree_bytes
    ucount = np.frombuffer(stream, dtype=np.uint32, count=nb, offset=at)
    off_sizes = at + nb * 4 + nb * esz + int(ucount.sum()) * esz
    return nb, ucount, off_sizes, off_sizes + nb * 8


# ------------------------------------------------------------------------------------------------------------------ the groups of cases
def g_box_form(ctx, oracle):
    for lo, hi in [((1, 2, 3), (5, 7, 6)), ((3, 3, 3), (13, 13, 13)), ((0, 0, 0), (16, 16, 16)), ((15, 15, 15), (16, 16, 16)),
                   ((0, 7, 8), (16, 9, 9)), ((7, 0, 0), (8, 16, 16)), ((0, 0, 15), (16, 16, 16))]:
        _check(ctx, oracle, "box", lo, hi)
    st = _check(ctx, oracle, "box", (8, 0, 8), (16, 8, 16))                   # box-aligned: the direct form
    assert st.n_blocks == 1
    assert _check(ctx, oracle, "box", (1, 2, 3), (5, 7, 6)).n_blocks == 1
    assert _check(ctx, oracle, "box", (3, 3, 3), (13, 13, 13)).n_blocks == 8


def g_scalar_rows_f64(ctx, oracle):
    _check(ctx, oracle, "f64-rows7", (5, 4, 6), (7, 6, 8))
    _check(ctx, oracle, "f64-rows7", (0, 0, 3), (12, 10, 14))


def g_unaligned_code_rows(ctx, oracle):
    _check(ctx, oracle, "rows18", (1, 0, 5), (8, 5, 18))


def g_column_form(ctx, oracle):
    for name in ("col", "col-f64"):
        assert _check(ctx, oracle, name, (0, 0, 20), (4, 32, 40)).n_blocks == 2        # an even count
        assert _check(ctx, oracle, name, (1, 5, 2), (3, 30, 31)).n_blocks == 1         # an odd count: k_omp_box
        assert _check(ctx, oracle, name, (2, 10, 10), (7, 50, 50)).n_blocks == 8


def g_verbatim_values(ctx, oracle):
    _check(ctx, oracle, "m32", (9, 9, 9), (23, 23, 23))
    _check(ctx, oracle, "col-m", (3, 30, 0), (8, 34, 64))
    d, s, want = _stream(oracle, "noisy")
    nb, ucount, _, _ = _tables(s, d.dtype)
    noisy = [0, 4, 8, 12]
    assert nb == 16 and (ucount[noisy] > 1000).all() and ucount.sum() < ucount[noisy].sum() + 100
    st = _check(ctx, oracle, "noisy", (1, 3, 20), (5, 60, 70))                # with noisy boxes: (0..2, 0..1, 0..1)
    assert st.n_blocks == 12 and st.n_unpred == int(ucount[_covered(d.shape, nb, (1, 3, 20), (5, 60, 70))].sum()) > 3000
    st = _check(ctx, oracle, "noisy", (2, 0, 64), (6, 64, 128))               # box-aligned, beside the noise: (1..2, 0..1, 1)
    assert st.n_blocks == 4 and st.n_unpred == int(ucount[[5, 7, 9, 11]].sum())
    st = _check(ctx, oracle, "noisy", (1, 33, 1), (8, 64, 100))               # below the noise: (0..3, 1, 0..1)
    assert st.n_blocks == 8 and st.n_unpred == int(ucount[[2, 3, 6, 7, 10, 11, 14, 15]].sum())


def g_special_values(ctx, oracle):
    for name, lo, hi in [("special-f32", (0, 0, 0), (9, 3, 31)), ("special-f64", (0, 0, 0), (9, 3, 31)),       # the +-0 stretch and the NaN at (8, 0, 0)
                         ("col-special-f32", (0, 0, 0), (5, 7, 64)), ("col-special-f64", (0, 0, 0), (5, 7, 64))]:
        d, s, want = _stream(oracle, name)
        crop = _crop(want, lo, hi)
        src = _crop(d, lo, hi)                                                    # (the array's NaN comes back as it is; its -0 stretch within the bound)
        assert np.isnan(crop).any() and (np.signbit(src) & (src == 0)).sum() >= 50, name
        _check(ctx, oracle, name, lo, hi)


def g_degenerate_and_large_books(ctx, oracle):
    _check(ctx, oracle, "constant", (2, 3, 4), (15, 9, 13))
    _check(ctx, oracle, "wide-codes", (3, 2, 9), (14, 16, 30))
    _check(ctx, oracle, "wide-codes-one-box", (5, 6, 7), (30, 29, 28))        # a payload too large for the decoder's LDS staging


def g_fuzz(ctx, oracle):
    rng = np.random.default_rng(11)
    names = ("box", "col", "m32")
    for k in range(40):
        name = names[k % 3]
        shape = _stream(oracle, name)[0].shape
        lo = [int(rng.integers(0, n)) for n in shape]
        hi = [int(rng.integers(l + 1, n + 1)) for l, n in zip(lo, shape)]
        _check(ctx, oracle, name, lo, hi)


def g_output_placement(ctx, oracle, device):
    """out / the stream on the "device" (the shim's device memory is host memory) and on the host; out one element behind a 16-byte aligned address, with guard bytes"""
    for name, lo, hi in (("box", (3, 3, 3), (13, 13, 13)), ("col", (0, 0, 20), (4, 32, 40)), ("col-f64", (4, 32, 0), (8, 64, 32)), ("box", (8, 0, 8), (16, 8, 16))):
        d, s, want = _stream(oracle, name)
        crop = np.ascontiguousarray(_crop(want, lo, hi))
        esz = d.dtype.itemsize
        for stream_dev in (False, True):
            for out_dev in (False, True):
                for off in (0, esz):
                    sr = ptr_cases.carve(len(s), 0, device=device and stream_dev).put(s)
                    o = ptr_cases.carve(crop.nbytes, off, pad=64, device=device and out_dev)
                    ctx.decompress_omp_region(sr.ptr, stream_dev, len(s), len(META), d.shape, d.dtype, lo, hi, o.ptr, out_dev)
                    got = o.get().view(d.dtype).reshape(crop.shape)
                    assert np.array_equal(_bits(got), _bits(crop)), (name, stream_dev, out_dev, off)
                    o.check(f"{name} stream_dev={stream_dev} out_dev={out_dev} off={off}")


def g_locality(ctx, oracle):
    import sz_amd
    d, s, want = _stream(oracle, "box")
    nb, ucount, off_sizes, off_pay = _tables(s, d.dtype)
    sizes = np.frombuffer(s, dtype=np.uint64, count=nb, offset=off_sizes)
    starts = off_pay + np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    lo, hi = (1, 2, 3), (5, 7, 6)                                             # inside box 0
    bad = bytearray(s)
    bad[int(starts[5]):int(starts[5] + sizes[5])] = b"\xff" * int(sizes[5])   # a box the region does not touch
    out, _ = _region(ctx, bytes(bad), d.shape, d.dtype, lo, hi)
    assert np.array_equal(_bits(out), _bits(_crop(want, lo, hi)))
    with pytest.raises(sz_amd.SZError):                                       # (the full decode does see it)
        full = np.empty_like(d)
        buf = ctypes.create_string_buffer(bytes(bad), len(bad))
        ctx.decompress_omp(ctypes.addressof(buf), False, len(bad), len(META), d.shape, d.dtype, full.ctypes.data, False)
    cut = bytearray(s)                                                        # the payload of a covered box truncated: its size entry re-written
    cut[off_sizes:off_sizes + 8] = int(sizes[0] // 2).to_bytes(8, "little")
    with pytest.raises(sz_amd.SZError):
        _region(ctx, bytes(cut), d.shape, d.dtype, lo, hi)


def g_refusals(ctx, oracle):
    import sz_amd
    d, s, want = _stream(oracle, "box")
    for lo, hi in (((2, 2, 2), (2, 5, 5)), ((0, 4, 0), (16, 4, 16)), ((0, 0, 9), (1, 1, 9)), ((0, 0, 0), (17, 16, 16)), ((0, 0, 3), (16, 16, 17)), ((5, 0, 0), (4, 16, 16))):
        out = np.full(16, 7.0, dtype=d.dtype)
        buf = ctypes.create_string_buffer(s, len(s))
        with pytest.raises(sz_amd.SZError, match="region"):
            ctx.decompress_omp_region(ctypes.addressof(buf), False, len(s), len(META), d.shape, d.dtype, lo, hi, out.ctypes.data, False)
        assert (out == 7.0).all()
    bad = bytearray(s); bad[len(META):len(META) + 4] = (7).to_bytes(4, "big")         # a thread_num that is not this array's grid
    with pytest.raises(sz_amd.SZError):
        _region(ctx, bytes(bad), d.shape, d.dtype, (0, 0, 0), (4, 4, 4))
    with pytest.raises(sz_amd.SZError):
        _region(ctx, s[:len(s) // 2], d.shape, d.dtype, (0, 0, 0), (4, 4, 4))


GROUPS = [g_box_form, g_scalar_rows_f64, g_unaligned_code_rows, g_column_form, g_verbatim_values, g_special_values, g_degenerate_and_large_books, g_fuzz,
          g_locality, g_refusals]
IDS = [g.__name__[2:] for g in GROUPS]


@pytest.fixture()
def shim_ctx(built):
    import sim_lib
    import sz_amd
    from sz_amd import api
    saved = api._lib
    api._lib = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    ctx = sz_amd.HipContext(0)
    yield ctx
    ctx.close()
    api._lib = saved


@pytest.fixture()
def hip_ctx(built):
    import sz_amd
    ctx = sz_amd.HipContext(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_region_on_cpu_shim(oracle, shim_ctx, group):
    group(shim_ctx, oracle)


def test_region_output_placement_on_cpu_shim(oracle, shim_ctx):
    g_output_placement(shim_ctx, oracle, device=False)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_hip_region(oracle, hip_ctx, group):
    group(hip_ctx, oracle)


@pytest.mark.gpu
def test_hip_region_output_placement(oracle, hip_ctx):
    g_output_placement(hip_ctx, oracle, device=True)


@pytest.mark.gpu
def test_hip_region_of_128_cubed(oracle, hip_ctx):
    """64 boxes of 32^3, the column form: a region over eight boxes (staging + crop) and a box-aligned one (the direct form)"""
    st = _check(hip_ctx, oracle, "s128", (40, 40, 40), (80, 80, 80))
    assert st.n_blocks == 8 and st.quant_kernel == 3
    st = _check(hip_ctx, oracle, "s128", (32, 0, 64), (96, 32, 128))
    assert st.n_blocks == 4 and st.quant_kernel == 3
