"""The geometry of k_col_encode's rounds (sz_amd/csrc/szh_segenc.h): a round is 256 threads x nr runs, nr chosen per segment and column so that the runs
spread evenly over as few rounds as the bit window allows; segments are of equal size (no short one at the end); the packing pass reads the codes from LDS a
second time.  The cases here are the ones that can go wrong with that and that tests/test_colenc.py does not reach.  Every case: the stream must be the
oracle's, byte for byte, and the decoded values the oracle decoder's, bit for bit (oracle/: pinned against the reference's recorded outputs)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _slow(nz, ny, nx, span, dtype=np.float32):
    """A slowly varying array whose range is `span`: with a bound of span / 4 nearly every code is the same one (one-bit code words)."""
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.ascontiguousarray((span * (0.5 * x / max(nx - 1, 1) + 0.3 * y / max(ny - 1, 1) + 0.2 * z / max(nz - 1, 1))).astype(dtype))


def _noisy(shape, sigma, seed, dtype=np.float32):
    from sz_amd.fields import s_field
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((s_field(*shape, np.float64) + sigma * rng.standard_normal(shape)).astype(dtype))


# name, array, error bound, switches, the alphabet (number of quantisation intervals) the case is meant to have: (lo, hi) or None
def _cases():
    from sz_amd.fields import s_field
    return [
        # 85 blocks along the row (2 of 7, 83 of 6: the 512^3 geometry): the column's runs are no whole number of rounds, three equal segments
        ("row512", s_field(12, 12, 512), 1e-4, "", None),
        # segments of three blocks: 3 x 36 runs a round, and a last segment of one block (85 = 28 x 3 + 1)
        ("row512-segb3", s_field(12, 12, 512), 1e-4, "SZ_HIP_SEG_SEGB=3", None),
        # a long row in a small tile: many segments, rounds of few runs per thread
        ("row1000-tile4", s_field(7, 13, 1000), 1e-4, "SZ_HIP_SEG_TILE_KB=4", None),
        # columns of 49 rows (7 x 7 blocks) beside columns of 36: more rounds in some columns than in others
        ("rows49", s_field(13, 13, 300), 1e-4, "", None),
        # one-bit code words, one block a segment: rounds of 36 runs (a few words each), the partial last word carried from round to round across segments.
        # (A column's first round cannot end inside its leading partial word: the host logic sends only arrays whose blocks hold 32 codes or more here, and the
        # first round holds a whole block at least -- so the kernel's test "is this word shared with the column before", made by the word's position, cannot be
        # told from a test made by progress with any input the library accepts.)
        ("one-bit-6x6x40", _slow(6, 6, 40, 4e-3), 1e-3, "SZ_HIP_SEG_SEGB=1", None),
        ("one-bit-12x12x40", _slow(12, 12, 40, 4e-3), 1e-3, "SZ_HIP_SEG_SEGB=1", None),
        ("one-bit-6x6x40-f64", _slow(6, 6, 40, 4e-3, np.float64), 1e-3, "SZ_HIP_SEG_SEGB=1", None),
        # alphabets on both sides of 64 symbols and beyond the per-column histograms' 256
        ("alphabet-64", _noisy((20, 24, 96), 6e-4, 3), 1e-4, "", (33, 64)),
        ("alphabet-256", _noisy((20, 24, 96), 1.5e-3, 4), 1e-4, "", (65, 256)),
        ("alphabet-1024", _noisy((20, 24, 96), 2.5e-2, 5), 1e-4, "", (257, 65535)),
        # float64, and rows whose length is a multiple of four only / of nothing (vw = 4 and 1)
        ("f64-row512", s_field(7, 12, 512, np.float64), 1e-4, "", None),
        ("f64-rows49", s_field(13, 13, 100, np.float64), 1e-5, "", None),
        ("vw4", s_field(20, 18, 44), 1e-4, "", None),
        ("vw1", s_field(20, 18, 45), 1e-4, "", None),
        ("vw4-long", s_field(12, 12, 500), 1e-4, "", None),
        ("vw1-long-segb3", s_field(12, 12, 501), 1e-4, "SZ_HIP_SEG_SEGB=3", None),
        # a single block along the row (the general form of the kernel: runs of up to 11 codes)
        ("one-block-row", s_field(30, 30, 11), 1e-4, "", None),
        ("two-wide-blocks", s_field(30, 30, 17), 1e-4, "", None),
    ]


CASES = None      # (built on first use)
NAMES = ["row512", "row512-segb3", "row1000-tile4", "rows49", "one-bit-6x6x40", "one-bit-12x12x40", "one-bit-6x6x40-f64", "alphabet-64", "alphabet-256",
         "alphabet-1024", "f64-row512", "f64-rows49", "vw4", "vw1", "vw4-long", "vw1-long-segb3", "one-block-row", "two-wide-blocks"]


def _case(name):
    global CASES
    if CASES is None:
        CASES = {c[0]: c for c in _cases()}
        assert sorted(CASES) == sorted(NAMES)
    return CASES[name]


def _check(monkeypatch, name):
    import oracle_lib as O
    import sz_amd
    _, d, eb, switch, alphabet = _case(name)
    for kv in filter(None, switch.split(";")):
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)
    assert sz_amd.SZ_Init(os.path.join(ROOT, "tests", "golden", "sz_speed.config")) == 0
    try:
        ref, _ = O.compress(d, O.ABS, eb)
        want = O.decompress(ref, d.shape, d.dtype)
        assert float(np.abs(want.astype(np.float64) - d).max()) <= eb       # (the oracle itself takes the input)
        got = sz_amd.SZ_compress_args(d, sz_amd.ABS, eb)
        st = sz_amd.SZ_hip_last_stats()
        print(name, "bytes", len(got), "intervals", int(st.intervals), "packing", int(st.packing))
        if alphabet is not None:
            assert alphabet[0] <= int(st.intervals) <= alphabet[1], (name, int(st.intervals))
        assert int(st.packing) == 1, (name, "the packing passes on natural-order codes did not run")
        assert got == ref, (name, len(got), len(ref))
        dec = sz_amd.SZ_decompress(got, d.shape, d.dtype)
        assert np.array_equal(dec.view(np.uint8), want.view(np.uint8)), (name, "decoded values differ from the reference decoder's")
    finally:
        sz_amd.SZ_Finalize()


@pytest.fixture
def shim():
    import sim_lib
    from sz_amd import api
    old = api._lib
    api._lib = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    yield
    api._lib = old


@pytest.mark.parametrize("name", NAMES)
def test_round_geometry_on_the_cpu_shim(shim, monkeypatch, name):
    _check(monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_round_geometry_on_the_gpu(monkeypatch, name):
    _check(monkeypatch, name)
