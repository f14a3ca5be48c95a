"""Unpredictable values (quantisation code 0, the value itself in a list behind the Huffman payload) at every density, at exact counts per block column and at
chosen places, through every path of the entropy stage -- and the opposite extreme, a code book of one symbol.

What handles the zero codes is data dependent: k_permute notes up to SZH_ZCAP = 128 zero places per (block column, segment) and k_unpred orders them if the column has
at most SZH_ZMAX = 1024 and no segment overflowed, else it scans the column (szhip_kernels.h); k_col_encode carries bit count and zero count in one sum and
`zeros_done` across rounds and segments; k_col_zeros / k_col_zscan / k_col_unpack rank the zeros again on the way back, bounded by `ucap` (szh_segenc.h).  The arrays of
the other test files, under the interval optimiser, leave a handful of zeros per column; tests/unpred_fields.py builds the arrays that do not, under 32 fixed
intervals, and asserts from the oracle's stages what each of them is built for.

Every case compares with the oracle (oracle/: pinned against the reference's recorded outputs): the stream byte for byte, the decoded values bit for bit with the
oracle decoder's output of the oracle's stream, stats.n_unpred with the oracle's count; and the stat that proves the path ran (packing, quant_kernel, book_on_device).
Every GPU test has a twin through the HIP-on-CPU shim; the twins of the density cases use the smaller shapes.  The counts of the exact-count arrays, per column and
per segment, which of k_unpred's routes each takes, and the times are in profiles/r11_unpredictable.txt.  k_unpred's two routes write the same list: moving SZH_ZCAP or
SZH_ZMAX changes no output, so no case here can notice it; the cases pin each route on its own side of each threshold."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ptr_cases as P  # noqa: E402
import unpred_fields as U  # noqa: E402

f32, f64 = np.float32, np.float64
A, B, C4, LONG = (24, 32, 48), (20, 30, 42), (20, 30, 44), (12, 12, 512)      # rows of 8 k (k_beam, vw 8) | odd rows (k_pencil, vw 1) | rows of 4 k only | several segments
WIDE, WIDE_SHORT = (12, 12, 1584), (7, 7, 1560)                                # nine segments of k_permute along the row (GPU) and the CPU twin, one block column
SHORT = (7, 12, 256)                                                          # the CPU twin of LONG: two block columns, two segments (blocks 0 - 31 and 32 - 41 of the row)
SIGMAS = (3e-3, 8e-3, 2e-2, 1e-1)
SZHIP_ERR_STREAM = -4


# ------------------------------------------------------------------------------------------------------------------ the arrays, by name

def _exact(K, shape=A, dtype=f32):
    if shape in (LONG, SHORT):        # every zero inside the second of the column's segments
        return lambda o: U.exact_count_case(o, shape, (0, 1), K, dtype, krange=U.perm_segments(shape)[1])
    if shape in (WIDE, WIDE_SHORT):   # the zeros spread over all nine segments, at most 128 in any: K alone decides k_unpred's route
        return lambda o: U.spread_count_case(o, shape, (0, 1) if shape == WIDE else (0, 0), K, dtype)
    assert shape == A, shape          # one segment: from 129 zeros on the segment's note overflows and k_unpred scans, whatever K is
    return lambda o: U.exact_count_case(o, A, (1, 2), K, dtype)


EXACT = {f"K{K}": _exact(K) for K in (127, 128, 129, 1023, 1024, 1025)}
EXACT.update({f"long-K{K}": _exact(K, LONG) for K in (127, 128, 129)})
EXACT["K1025-f64"] = _exact(1025, A, f64)
EXACT.update({f"spread-K{K}": _exact(K, WIDE) for K in (1023, 1024, 1025)})
EXACT_SHIM = {f"short-K{K}": _exact(K, SHORT) for K in (127, 128, 129)}
EXACT_SHIM.update({f"spread-short-K{K}": _exact(K, WIDE_SHORT) for K in (1024, 1025)})

# C4 has blocks 7 wide along the row (44 = 2 x 7 + 5 x 6) and along the slowest axis
PLACES = [(0, 0, 0), (-1, -1, -1),                   # the array's first and last element
          (9, 8, 0), (9, 14, -1),                    # the first and the last element of a row
          (3, 20, 6), (15, 3, 13),                   # the 7th code of a 7-wide block (k = 6 and k = 13)
          (6, 5, 40), (19, 29, 20), (13, 29, 43)]    # the last row of a block at the end of a column; the array's last row; the last run of the second-last block row
# outliers three values into a block on the middle axis: no point the block selection samples is touched (the oracle keeps every block a Lorenzo block: asserted)
LORENZO_PLACES = [(6, 16, 4), (12, 2, 22), (18, 9, 40), (0, 28, 10), (-1, -1, -1)]
POSITION = {"places": lambda o: U.position_case(o, C4, PLACES, "places"),
            "places-f64": lambda o: U.position_case(o, C4, PLACES, "places-f64", f64),
            # a column that is entirely zero (the array's last: nothing lies in front of it) beside empty ones; every round and segment of it ends on a zero
            "full-column": lambda o: U.position_case(o, A, [], "full-column", full_column=(3, 4)),
            "full-column-long": lambda o: U.position_case(o, LONG, [(0, 0, 0)], "full-column-long", full_column=(1, 1)),
            "full-column-short": lambda o: U.position_case(o, SHORT, [], "full-column-short", full_column=(0, 1)),
            "lorenzo-only": lambda o: U.position_case(o, A, LORENZO_PLACES, "lorenzo-only")}
DENSE = {f"{'x'.join(map(str, s))}-{np.dtype(t).name}-{g:g}": (lambda o, s=s, g=g, t=t: U.density_case(o, s, g, t))
         for s, t, gs in ((A, f32, SIGMAS), (A, f64, (8e-3, 1e-1)), (B, f32, SIGMAS), (B, f64, (3e-3, 1e-1)), (C4, f32, (8e-3, 1e-1))) for g in gs}


def _noise2d(amp, dtype):
    return np.ascontiguousarray((amp * (2 * np.random.default_rng(5).random((30, 36)) - 1)).astype(dtype))


def _bumps(shape, dtype):
    x = U.plane(shape, dtype).copy()
    x[5::7, 3::5, 2::9] += np.dtype(dtype).type(2e-3)
    return x


BOOKS = {"plane-beam-f32": (lambda: U.plane(A, f32), 1), "plane-beam-f64": (lambda: U.plane(A, f64), 1),
         "plane-pencil-f32": (lambda: U.plane(B, f32), 1), "plane-pencil-f64": (lambda: U.plane(B, f64), 1),
         "2d-30x36-f32": (lambda: _noise2d(0.8e-3, f32), 1), "2d-30x36-f64": (lambda: _noise2d(0.8e-3, f64), 1),       # noise below the bound, a range above it
         "two-symbols-f32": (lambda: _bumps(A, f32), 2), "two-symbols-pencil-f64": (lambda: _bumps(B, f64), 2), "two-symbols-2d": (lambda: _noise2d(0.95e-3, f32), 2)}
BOOK = {k: (lambda o, k=k: U.book_case(o, k, BOOKS[k][0](), BOOKS[k][1])) for k in BOOKS}
ARRAYS = {**EXACT, **EXACT_SHIM, **POSITION, **DENSE, **BOOK}


def _case(oracle, name):
    c = ARRAYS[name](oracle)
    if name == "lorenzo-only":
        assert c["reg_count"] == 0 and c["total_unpred"] >= 8 * 4 + 1, (name, c["reg_count"], c["total_unpred"])
    if name.startswith("full-column"):
        cz, x = c["column_zeros"], c["x"]
        codes_in_column = int(np.prod([U.axis(n)[1][-1] for n in x.shape[:2]])) * x.shape[2]
        assert cz[-1, -1] == codes_in_column and cz[-1, -2] == 0 and (cz.shape[0] == 1 or cz[-2, -1] == 0), (name, cz.tolist())
    if name.startswith("spread"):
        # the precondition of the SZH_ZMAX cases: no segment's note overflows and at least eight segments hold zeros, so 1023 and 1024 keys (of several segments, one
        # behind the other) are ordered by rank and 1025 zeros are found by the scan
        assert max(c["per_segment"]) <= U.SZH_ZCAP and sum(1 for q in c["per_segment"] if q) >= 8 and sum(c["per_segment"]) == int(name.split("K")[1]), (name, c["per_segment"])
    if name.startswith(("long-K", "short-K")):
        K = int(name.split("K")[1])
        assert c["per_segment"] == ([0, K, 0] if name.startswith("long") else [0, K]), (name, c["per_segment"])
    return c


# ------------------------------------------------------------------------------------------------------------------ fixtures

@pytest.fixture(scope="module")
def cfg(tmp_path_factory):
    """tests/golden/sz_speed.config with 32 fixed intervals; cfg[0]: SZ 2.1, cfg[1]: withLinearRegression = NO"""
    import ref_cases
    d = tmp_path_factory.mktemp("unpredictable")
    base = {"quantization_intervals": U.INTERVALS, "max_quant_intervals": U.INTERVALS, "absErrBound": U.BOUND}
    paths = []
    for nm, extra in (("sz21", {}), ("sz14", {"withLinearRegression": "NO"})):
        paths.append(str(d / f"{nm}_32.config"))
        ref_cases.write_config(paths[-1], {**base, **extra})
    return paths


@pytest.fixture
def shim(built):
    import sim_lib
    from sz_amd import api
    old = api._lib
    api._lib = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    yield
    api._lib = old


def _setenv(monkeypatch, switch):
    for kv in filter(None, switch.split(";")):
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)


def _params():
    import sz_amd
    return sz_amd.api.szhip_params(100, 0.99, U.INTERVALS, U.INTERVALS)


# ------------------------------------------------------------------------------------------------------------------ checks

def _same(got, want, what):
    assert len(got) == len(want), (what, "stream of", len(got), "bytes, the oracle's has", len(want))
    if got != want:
        d = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
        raise AssertionError(f"{what}: {d.size} bytes differ from the oracle's stream, the first at {int(d[0])} of {len(want)}")


def _same_values(dec, want, what):
    d = np.flatnonzero(U.bits(dec) != U.bits(want))
    assert d.size == 0, f"{what}: {d.size} decoded values differ from the oracle decoder's, the first at {int(d[0])}"


def _compress(monkeypatch, cfg, c, name, switch, want=None, sz14=False):
    """SZ_compress_args under the switch: the oracle's stream, its count of unpredictable values, and the stats in `want`"""
    import sz_amd
    _setenv(monkeypatch, switch)
    assert sz_amd.SZ_Init(cfg[1 if sz14 else 0]) == 0
    try:
        x = c["x"]
        got = sz_amd.SZ_compress_args(x, sz_amd.ABS, U.BOUND)
        st = sz_amd.SZ_hip_last_stats()
        n_unpred = c["total_unpred"] if "total_unpred" in c else c["n_unpred"]
        what = f"{name} [{switch or 'default'}]"
        print(f"{what}: {len(got)} bytes, n_unpred {int(st.n_unpred)} (oracle {n_unpred}), packing {int(st.packing)}, quant_kernel {int(st.quant_kernel)}, "
              f"book_on_device {int(st.book_on_device)}")
        _same(got, c["ref"], what)
        assert int(st.n_unpred) == n_unpred, (what, int(st.n_unpred), n_unpred)
        for k, v in (want or {}).items():
            assert int(getattr(st, k)) == v, (what, k, int(getattr(st, k)), "expected", v)
    finally:
        sz_amd.SZ_Finalize()


def _decode(monkeypatch, cfg, c, name, switch, sz14=False):
    """SZ_decompress of the ORACLE's stream under the switch: the oracle decoder's values, bit for bit"""
    import sz_amd
    _setenv(monkeypatch, switch)
    assert sz_amd.SZ_Init(cfg[1 if sz14 else 0]) == 0
    try:
        x = c["x"]
        dec = sz_amd.SZ_decompress(c["ref"], x.shape, x.dtype)
        _same_values(dec, c["dec"], f"{name} [decode, {switch or 'default'}]")
    finally:
        sz_amd.SZ_Finalize()


def _beam(c):
    return P.beam_eligible(c["x"])


def _want(c, switch):
    """the stats that prove which kernels a compress call of a 3-D array ran"""
    w = {"packing": 0 if "SZ_HIP_SEGENC=0" in switch else 1, "quant_kernel": 2 if _beam(c) and "SZ_HIP_BEAM=0" not in switch else 0}
    if "SZ_HIP_DEV_BOOK=1" in switch:
        w["book_on_device"] = 1
    return w


COMPRESS = ["", "SZ_HIP_SEGHIST=0", "SZ_HIP_SEG_SCAN1=0", "SZ_HIP_SEG_SEGB=1", "SZ_HIP_SEG_TILE_KB=4",
            "SZ_HIP_SEGENC=0",                             # k_permute + k_unpred, in slices beside the beam where it runs (four by default)
            "SZ_HIP_SEGENC=0;SZ_HIP_ENC32=0", "SZ_HIP_SEGENC=0;SZ_HIP_SLICES=1", "SZ_HIP_SEGENC=0;SZ_HIP_SLICES=3", "SZ_HIP_BEAM=0"]
DECODE = ["", "SZ_HIP_COL_UNPACK=0", "SZ_HIP_UNPACK_TILE_KB=4", "SZ_HIP_SEG_SCAN1=0", "SZ_HIP_DEC_CHECKS_LAST=0", "SZ_HIP_TEST_HDEC_FALLBACK=1"]
ALL_SWITCH_ARRAYS = [k for k in list(EXACT) + list(POSITION) if k != "full-column-short"]
EXACT_ON_SHIM = [k for k in EXACT if not k.startswith(("long", "spread"))] + [k for k in EXACT_SHIM if k.startswith("short")]
# (nine segments need a row of 1542 values or more: 76 000 values, 15 s a call on the shim -- so the list's last K and the scan's first, through k_permute / k_unpred only, both ways)
SPREAD_ON_SHIM = ["spread-short-K1024", "spread-short-K1025"]
# the CPU twins: the thresholds matter to k_permute / k_unpred (SZ_HIP_SEGENC=0 and SZ_HIP_COL_UNPACK=0), every exact-count array goes through those and the default;
# the position arrays go through every switch
SHIM_COMPRESS = [(a, s) for a in EXACT_ON_SHIM for s in ("", "SZ_HIP_SEGENC=0")] + [(a, s) for a in ("places", "full-column") for s in COMPRESS] + \
                [(a, s) for a in ("K128", "K129", "K1025", "short-K129") for s in COMPRESS[1:5] + COMPRESS[6:]] + [(a, "SZ_HIP_SEGENC=0") for a in SPREAD_ON_SHIM] + [(a, s) for a in ("full-column-short", "places-f64", "lorenzo-only") for s in ("", "SZ_HIP_SEGENC=0")]
SHIM_DECODE = [(a, s) for a in EXACT_ON_SHIM for s in ("", "SZ_HIP_COL_UNPACK=0")] + [(a, s) for a in ("places", "K128", "K129", "K1025", "short-K129") for s in DECODE[2:]] + [(a, "SZ_HIP_COL_UNPACK=0") for a in SPREAD_ON_SHIM] + \
              [(a, s) for a in ("places", "full-column", "places-f64", "full-column-short", "lorenzo-only") for s in DECODE[:2]]
DENSE_SHIM = [k for k in DENSE if k.startswith("20x30x42")] + ["24x32x48-float32-0.1", "20x30x44-float32-0.008"]


# ------------------------------------------------------------------------------------------------------------------ CPU: the arrays

def test_every_array_is_what_it_is_built_for(oracle):
    """the builders assert their own preconditions; this prints what the oracle reported (profiles/r11_unpredictable.txt is this output)"""
    for name in ARRAYS:
        c = _case(oracle, name)
        print(name + ": " + c["report"])
    for K in (127, 128, 129, 1023, 1024, 1025):
        cz = _case(oracle, f"K{K}")["column_zeros"]
        assert cz[1, 2] == K and cz.sum() == K
    assert len(U.perm_segments(WIDE)) == 9 and len(U.perm_segments(WIDE_SHORT)) == 9
    assert U.SZH_ZCAP == 128 and U.SZH_ZMAX == 1024
    src = open(os.path.join(ROOT, "sz_amd", "csrc", "szhip_kernels.h")).read()
    assert "#define SZH_ZCAP 128" in src and "#define SZH_ZMAX 1024" in src          # (the thresholds the counts are built around)
    assert U.perm_segments(LONG) == [(0, 194), (194, 386), (386, 512)] and U.perm_segments(A) == [(0, 48)] and U.perm_segments(SHORT) == [(0, 196), (196, 256)]


# ------------------------------------------------------------------------------------------------------------------ SZ 2.1, 3-D: compress

@pytest.mark.parametrize("name,switch", SHIM_COMPRESS)
def test_compress_switches_on_the_cpu_shim(oracle, shim, monkeypatch, cfg, name, switch):
    c = _case(oracle, name)
    _compress(monkeypatch, cfg, c, name, switch, _want(c, switch))


@pytest.mark.gpu
@pytest.mark.parametrize("switch", COMPRESS)
@pytest.mark.parametrize("name", ALL_SWITCH_ARRAYS)
def test_compress_switches_on_the_gpu(oracle, monkeypatch, cfg, name, switch):
    c = _case(oracle, name)
    _compress(monkeypatch, cfg, c, name, switch, _want(c, switch))


@pytest.mark.parametrize("switch", ["", "SZ_HIP_SEGENC=0"])
@pytest.mark.parametrize("name", DENSE_SHIM)
def test_compress_densities_on_the_cpu_shim(oracle, shim, monkeypatch, cfg, name, switch):
    c = _case(oracle, name)
    _compress(monkeypatch, cfg, c, name, switch, _want(c, switch))


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["", "SZ_HIP_SEGENC=0"])
@pytest.mark.parametrize("name", list(DENSE))
def test_compress_densities_on_the_gpu(oracle, monkeypatch, cfg, name, switch):
    c = _case(oracle, name)
    _compress(monkeypatch, cfg, c, name, switch, _want(c, switch))


BOOK_ON_DEVICE = ["lorenzo-only"]


@pytest.mark.parametrize("name", BOOK_ON_DEVICE)
def test_device_book_on_the_cpu_shim(oracle, shim, monkeypatch, cfg, name):
    c = _case(oracle, name)
    assert c["reg_count"] == 0
    _compress(monkeypatch, cfg, c, name, "SZ_HIP_DEV_BOOK=1", _want(c, "SZ_HIP_DEV_BOOK=1"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOOK_ON_DEVICE)
def test_device_book_on_the_gpu(oracle, monkeypatch, cfg, name):
    c = _case(oracle, name)
    assert c["reg_count"] == 0
    _compress(monkeypatch, cfg, c, name, "SZ_HIP_DEV_BOOK=1", _want(c, "SZ_HIP_DEV_BOOK=1"))


# ------------------------------------------------------------------------------------------------------------------ SZ 2.1, 3-D: decompress

@pytest.mark.parametrize("name,switch", SHIM_DECODE)
def test_decode_switches_on_the_cpu_shim(oracle, shim, monkeypatch, cfg, name, switch):
    _decode(monkeypatch, cfg, _case(oracle, name), name, switch)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", DECODE)
@pytest.mark.parametrize("name", ALL_SWITCH_ARRAYS)
def test_decode_switches_on_the_gpu(oracle, monkeypatch, cfg, name, switch):
    _decode(monkeypatch, cfg, _case(oracle, name), name, switch)


@pytest.mark.parametrize("switch", ["", "SZ_HIP_COL_UNPACK=0"])
@pytest.mark.parametrize("name", DENSE_SHIM)
def test_decode_densities_on_the_cpu_shim(oracle, shim, monkeypatch, cfg, name, switch):
    _decode(monkeypatch, cfg, _case(oracle, name), name, switch)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["", "SZ_HIP_COL_UNPACK=0"])
@pytest.mark.parametrize("name", list(DENSE))
def test_decode_densities_on_the_gpu(oracle, monkeypatch, cfg, name, switch):
    _decode(monkeypatch, cfg, _case(oracle, name), name, switch)


def _ctx_decode(ctx, dev, c, name, prefill=None):
    """szhip_decompress of the oracle's stream into the caller's array (pre-filled with random bits if asked): values, n_unpred, and the guard bytes round the array"""
    x = c["x"]
    strm, dst = P.carve(len(c["ref"]), 0, device=dev).put(c["ref"]), P.carve(x.nbytes, 0, device=dev)
    if prefill is not None:
        dst.put(np.random.default_rng(prefill).integers(0, 256, x.nbytes, dtype=np.uint8))
    st = ctx.decompress(strm.ptr, True, len(c["ref"]), P.meta_len(x) + 8, P.shape3(x), x.dtype, dst.ptr, True)
    _same_values(dst.get().view(x.dtype), c["dec"], name)
    dst.check(name + " (output)")
    assert int(st.n_unpred) == (c["total_unpred"] if "total_unpred" in c else c["n_unpred"]), (name, int(st.n_unpred))
    return st


PREFILLED = ["K128", "K1025", "spread-K1024", "spread-K1025", "long-K129", "places", "full-column", "24x32x48-float32-0.1", "20x30x42-float32-0.008", "plane-beam-f32"]
PREFILLED_SHIM = ["K129", "places", "20x30x42-float32-0.1", "plane-pencil-f32"]


def _prefilled(oracle, monkeypatch, dev, name, switch):
    import sz_amd
    _setenv(monkeypatch, switch)
    ctx = sz_amd.HipContext(0)
    try:
        _ctx_decode(ctx, dev, _case(oracle, name), name, prefill=3)
    finally:
        ctx.close()


@pytest.mark.parametrize("switch", ["", "SZ_HIP_COL_UNPACK=0"])
@pytest.mark.parametrize("name", PREFILLED_SHIM)
def test_decode_into_an_array_of_random_bits_on_the_cpu_shim(oracle, shim, monkeypatch, name, switch):
    _prefilled(oracle, monkeypatch, False, name, switch)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["", "SZ_HIP_COL_UNPACK=0"])
@pytest.mark.parametrize("name", PREFILLED)
def test_decode_into_an_array_of_random_bits_on_the_gpu(oracle, monkeypatch, name, switch):
    _prefilled(oracle, monkeypatch, True, name, switch)


# ------------------------------------------------------------------------------------------------------------------ one- and two-symbol code books

BOOK_PATHS = [("", ""), ("SZ_HIP_SEGENC=0", "SZ_HIP_COL_UNPACK=0"), ("SZ_HIP_SEG_SEGB=1", "SZ_HIP_TEST_HDEC_FALLBACK=1")]


def _book(oracle, monkeypatch, cfg, name, enc, dec):
    c = _case(oracle, name)
    assert len(c["distinct"]) == BOOKS[name][1] and (BOOKS[name][1] > 1 or c["huff_bytes"] == 0)
    _compress(monkeypatch, cfg, c, name, enc, _want(c, enc) if c["x"].ndim == 3 else None)
    _decode(monkeypatch, cfg, c, name, dec)


@pytest.mark.parametrize("enc,dec", BOOK_PATHS)
@pytest.mark.parametrize("name", ["plane-pencil-f32", "plane-pencil-f64", "plane-beam-f32", "2d-30x36-f32", "2d-30x36-f64", "two-symbols-pencil-f64", "two-symbols-2d"])
def test_books_of_one_and_two_symbols_on_the_cpu_shim(oracle, shim, monkeypatch, cfg, name, enc, dec):
    _book(oracle, monkeypatch, cfg, name, enc, dec)


@pytest.mark.gpu
@pytest.mark.parametrize("enc,dec", BOOK_PATHS)
@pytest.mark.parametrize("name", list(BOOKS))
def test_books_of_one_and_two_symbols_on_the_gpu(oracle, monkeypatch, cfg, name, enc, dec):
    _book(oracle, monkeypatch, cfg, name, enc, dec)


# ------------------------------------------------------------------------------------------------------------------ a pool lane, beside an S-field

def _pool(oracle, dev, lanes, orders):
    import sz_amd
    from sz_amd.fields import s_field
    s = s_field(14, 20, 36)
    s_ref, s_st = oracle.compress(s, oracle.ABS, 1e-4, want_stages=True)
    work = [(c["x"], U.BOUND, c["ref"], _params(), c["total_unpred"]) for c in (_case(oracle, "24x32x48-float32-0.1"), _case(oracle, "K1025"))]
    work.append((s, 1e-4, s_ref, None, int(s_st["total_unpred"])))
    srcs = [P.carve(w[0].nbytes, 0, device=dev).put(w[0]) for w in work]
    outs = [P.carve(len(w[2]) + (1 << 16), 0, device=dev) for w in work]
    metas = [w[2][:P.meta_len(w[0])] for w in work]
    pool = sz_amd.HipPool(0, lanes)
    try:
        for order in orders:                                         # the lanes see the arrays in several orders, the S-field between and beside them
            tks = [(i, pool.submit(srcs[i].ptr, True, work[i][0].shape, work[i][0].dtype, work[i][1], metas[i], work[i][3], outs[i].ptr, outs[i].nbytes)) for i in order]
            for i, tk in tks:
                n, st = pool.wait(tk)
                what = f"pool, order {order}, array {i}"
                _same(bytes(outs[i].get(n)), work[i][2], what)
                assert int(st.n_unpred) == work[i][4] and int(st.packing) == 1, (what, int(st.n_unpred), int(st.packing))
                outs[i].check(what)
    finally:
        pool.close()


def test_pool_lane_beside_an_s_field_on_the_cpu_shim(oracle, shim):
    _pool(oracle, False, 1, ((0, 2, 1), (1, 0, 2)))          # (the shim runs one workgroup at a time on the calling thread: one lane)


@pytest.mark.gpu
def test_pool_lanes_beside_an_s_field_on_the_gpu(oracle):
    _pool(oracle, True, 2, ((0, 2, 1), (2, 1, 0), (1, 0, 2), (0, 2, 1)))


# ------------------------------------------------------------------------------------------------------------------ the other formats

FORMAT_CASES = [(f, which) for f in U.FORMATS for which in ("low", "high", "places")]


def _format(oracle, monkeypatch, cfg, fmt, which, dtype):
    import sz_amd
    c = U.format_position_case(oracle, fmt, dtype) if which == "places" else U.format_density_case(oracle, fmt, which == "high", dtype)
    name = f"{fmt}-{which}-{np.dtype(dtype).name}"
    x = c["x"]
    if c["kind"] != "omp":
        _compress(monkeypatch, cfg, c, name, "", None, sz14=c["kind"] == "sz14")
        _decode(monkeypatch, cfg, c, name, "", sz14=c["kind"] == "sz14")
        return
    ctx = sz_amd.HipContext(0)
    try:
        got, n, st = ctx.compress_omp(x.ctypes.data, False, x.shape, x.dtype, U.BOUND, U.OMP_THREADS, U.OMP_META, sz_amd.api.szhip_params(100, 0.99, 65536, U.INTERVALS))
        print(f"{name}: {n} bytes, n_unpred {int(st.n_unpred)} (oracle {c['n_unpred']})")
        _same(got, c["ref"], name)
        assert int(st.n_unpred) == c["n_unpred"], (name, int(st.n_unpred))
        out = np.full(x.shape, np.nan, dtype=x.dtype)
        buf = ctypes.create_string_buffer(c["ref"], len(c["ref"]))
        st = ctx.decompress_omp(ctypes.addressof(buf), False, len(c["ref"]), len(U.OMP_META), x.shape, x.dtype, out.ctypes.data, False)
        _same_values(out, c["dec"], name)
        assert int(st.n_unpred) == c["n_unpred"], (name, int(st.n_unpred))
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt,which", FORMAT_CASES)
def test_other_formats_on_the_cpu_shim(oracle, shim, monkeypatch, cfg, fmt, which):
    _format(oracle, monkeypatch, cfg, fmt, which, f64 if which == "high" else f32)       # (float64 once a format, at the 75 % density)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [f32, f64], ids=["f32", "f64"])
@pytest.mark.parametrize("fmt,which", FORMAT_CASES)
def test_other_formats_on_the_gpu(oracle, monkeypatch, cfg, fmt, which, dtype):
    _format(oracle, monkeypatch, cfg, fmt, which, dtype)


# ------------------------------------------------------------------------------------------------------------------ one context, alternating inputs

def _alternate(oracle, dev, shape, rounds):
    """75 % unpredictable, then 0.3 %, then the one-symbol plane, through ONE context, compress and decompress: a count, an offset or a list left over from the call
    before would show in the stream, in n_unpred or in the values"""
    import sz_amd
    cases = [("75 %", U.density_case(oracle, shape, 1e-1)), ("0.3 %", U.density_case(oracle, shape, 3e-3)),
             ("one symbol", U.book_case(oracle, "plane-beam-f32" if shape == A else "plane-pencil-f32", U.plane(shape, f32), 1))]
    ctx = sz_amd.HipContext(0)
    try:
        for r in range(rounds):
            for nm, c in cases:
                x, what = c["x"], f"round {r}, {nm}"
                src = P.carve(x.nbytes, 0, device=dev).put(x)
                got, n, st = ctx.compress(src.ptr, True, x.shape, x.dtype, U.BOUND, c["ref"][:P.meta_len(x)], _params())
                _same(got, c["ref"], what)
                assert int(st.n_unpred) == c["total_unpred"] and int(st.packing) == 1, (what, int(st.n_unpred), int(st.packing))
                _ctx_decode(ctx, dev, c, what, prefill=r)
    finally:
        ctx.close()


def test_one_context_with_alternating_densities_on_the_cpu_shim(oracle, shim):
    _alternate(oracle, False, B, 2)


@pytest.mark.gpu
def test_one_context_with_alternating_densities_on_the_gpu(oracle):
    _alternate(oracle, True, A, 3)
    _alternate(oracle, True, B, 2)


# ------------------------------------------------------------------------------------------------------------------ CPU only: a header that lies about the count

def _tampered(c, delta):
    """The oracle's stream with the header's count of unpredictable values changed by `delta` and the list made to fit (its last value dropped, or one more appended), so
    that the Huffman payload stays where the header says it is: only the comparison of the count with the codes' zeros can refuse the stream."""
    x, ref = c["x"], c["ref"]
    K, w = c["total_unpred"], x.dtype.itemsize
    # the count is the 8 bytes in front of the list; the list holds the values in block order: found by its content
    vals = np.ascontiguousarray(x.reshape(-1)[U.block_order(x.shape)][c["codes"] == 0])
    at = ref.find(vals.tobytes())
    assert at >= 8 and int.from_bytes(ref[at - 8:at], sys.byteorder) == K and ref.find(vals.tobytes(), at + 1) < 0, "the list of unpredictable values was not found"
    head, lst, tail = ref[:at - 8], ref[at:at + K * w], ref[at + K * w:]
    lst = lst[:-w] if delta < 0 else lst + np.asarray([12345.0], dtype=x.dtype).tobytes()
    return head + int(K + delta).to_bytes(8, sys.byteorder) + lst + tail


@pytest.mark.parametrize("switch", ["", "SZ_HIP_DEC_CHECKS_LAST=0", "SZ_HIP_COL_UNPACK=0"])
@pytest.mark.parametrize("delta", [-1, 1])
@pytest.mark.parametrize("name", ["places", "K129", "20x30x42-float32-0.1"])
def test_a_count_that_differs_from_the_codes_zeros_is_refused(oracle, shim, monkeypatch, capfd, name, delta, switch):
    import sz_amd
    from sz_amd import api
    _setenv(monkeypatch, switch)
    c = _case(oracle, name)
    x = c["x"]
    bad = _tampered(c, delta)
    ctx = sz_amd.HipContext(0)
    try:
        _ctx_decode(ctx, False, c, name + " (before)")
        strm, dst = P.carve(len(bad), 0).put(bad), P.carve(x.nbytes, 0)
        st = api.szhip_stats()
        rc = api.lib().szhip_decompress(ctx._h, 0 if x.dtype == np.float32 else 1, strm.ptr, 1, len(bad), P.meta_len(x) + 8, *P.shape3(x), dst.ptr, 1, ctypes.byref(st))
        assert rc == SZHIP_ERR_STREAM, (name, delta, switch, rc)
        assert "unpredictable values, codes need" in capfd.readouterr().err
        dst.check(f"{name}, count {delta:+d} [{switch or 'default'}] (output)")
        strm.check(f"{name}, count {delta:+d} (stream)")
        _ctx_decode(ctx, False, c, name + " (after)", prefill=1)                     # the same context takes the valid stream afterwards
    finally:
        ctx.close()
