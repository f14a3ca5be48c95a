"""The reference's OpenMP container (sz/src/sz_omp.c:63-358: a 3-D array cut into thread_num independent boxes, one Huffman code book, one
byte-aligned payload per box) on the HIP side: sz_amd/csrc/szh_omp.h, szhip_compress_omp / szhip_decompress_omp.

The bar: the stream is byte for byte what oracle/szo_omp_impl.h writes (itself pinned against the unmodified reference built with -fopenmp,
tests/test_omp_container.py), on the recorded reference cases md5 for md5 with the reference's own output; the decoded array is bit for bit
what the oracle decodes.

(The file sorts last for a historical reason: its GPU tests were written after round 3's hardware time was spent.  They have run since --
driver box at the end of round 3, every GPU call of round 4 -- and are green.)

CPU (-m "not gpu"): the product code through the HIP-on-CPU shim (tests/sim).  GPU (-m gpu): the same cases through the built library, a
256^3 array against the oracle and the 512^3 array of the bench through the round trip.  The `col-*` cases (32 x 32 box faces) run round 4's
column-per-lane sweep, per-box entropy stage and look-up-table decoder; the others the first form of the kernels."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
RECORDED = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_recorded_omp.json")))
META = bytes(range(1, 33))


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _special(shape, dtype):
    """zeros of both signs, a NaN, an infinity, values far outside the quantiser's range, a constant stretch"""
    from sz_amd.fields import s_field
    d = s_field(*shape, np.dtype(dtype).type)
    f = d.ravel()
    f[3] = 0.0; f[4] = -0.0; f[5] = 1e30; f[6] = -1e30; f[40:90] = -0.0; f[100:400] = 0.25
    f[f.size // 2] = np.nan; f[f.size // 2 + 7] = np.inf
    return d


def _cases():
    from sz_amd.fields import l_field, m_field, s_field
    yield "S-16-t8", s_field(16, 16, 16), 1e-3, 8, 0
    yield "S-32-t64-fixed256", s_field(32, 32, 32), 1e-4, 64, 256
    yield "S-16x24x40-t16", s_field(16, 24, 40), 1e-3, 16, 0
    yield "S-f64-12x10x14-t8", s_field(12, 10, 14, np.float64), 1e-3, 8, 0             # rows of 7: the scalar path
    yield "S-f64-16x16x32-t8", s_field(16, 16, 32, np.float64), 1e-5, 8, 0
    yield "S-32-t1", s_field(32, 32, 32), 1e-3, 1, 0                                    # one box
    yield "S-8x8x18-t4", s_field(8, 8, 18), 1e-3, 4, 0                                  # rows of 18 codes: unaligned code rows
    yield "L-32-t8", l_field(32, 32, 32), 1e-3, 8, 0
    yield "M-32-t8-tight", np.ascontiguousarray(m_field(32)), 1e-6, 8, 0                # most values verbatim
    yield "special-f32", _special((16, 16, 32), np.float32), 1e-3, 8, 0
    yield "special-f64", _special((16, 16, 32), np.float64), 1e-3, 8, 64
    yield "constant", np.full((16, 16, 16), 1.5, dtype=np.float32), 1e-3, 8, 0           # one symbol: empty payloads
    fill = s_field(16, 16, 32); fill.ravel()[::7] = 1e30
    yield "fill-values-optimised", fill, 1e-4, 8, 0                                      # quotients beyond 2^64 in the interval optimiser
    yield "wide-codes", (np.random.default_rng(5).standard_normal((16, 16, 32)) * 50).astype(np.float32), 1e-3, 8, 65536
    # a payload and a node table too large for the decoder's LDS staging (one box of 32^3, ~14 bits per code)
    # 32 x 32 box faces, boxes in pairs: the column-per-lane sweep (szh_ompcol.h, round 4); everything above runs on k_omp_box
    yield "col-S-64-t8", s_field(64, 64, 64), 1e-4, 8, 0                                # eight 32^3 boxes
    yield "col-S-8x64x64-t8", s_field(8, 64, 64), 1e-3, 8, 0                            # four planes a box
    yield "col-S-2x64x64-t8", s_field(2, 64, 64), 1e-3, 8, 0                            # ONE plane a box: first and last line at once
    yield "col-L-6x64x64-t8-fixed64", l_field(6, 64, 64), 1e-3, 8, 64                   # three planes
    yield "col-S-f64-8x64x64-t8", s_field(8, 64, 64, np.float64), 1e-5, 8, 0
    yield "col-S-f64-64x64x32-t4", s_field(64, 64, 32, np.float64), 1e-3, 4, 0          # a 2 x 2 x 1 grid of 32^3 boxes
    yield "col-M-tight", np.ascontiguousarray(m_field(64)[:8]), 1e-6, 8, 0              # most values verbatim: the inverse with verbatim values
    yield "col-special-f32", _special((8, 64, 64), np.float32), 1e-3, 8, 0
    yield "col-special-f64", _special((8, 64, 64), np.float64), 1e-3, 8, 64
    yield "col-constant", np.full((4, 64, 64), 1.5, dtype=np.float32), 1e-3, 8, 0
    yield "col-wide-codes", (np.random.default_rng(7).standard_normal((4, 64, 64)) * 50).astype(np.float32), 1e-3, 8, 65536
    mix = s_field(8, 64, 128); mix[:, :32, 32:64] = (np.random.default_rng(8).standard_normal((8, 32, 32)) * 3).astype(np.float32)
    yield "col-one-noisy-box-t16", mix, 1e-4, 16, 0                                     # wavefronts with and without verbatim values side by side
    yield "wide-codes-one-box", (np.random.default_rng(6).standard_normal((32, 32, 32)) * 50).astype(np.float32), 1e-3, 1, 65536


def _run_cases(ctx, oracle, cases):
    import sz_amd
    for name, d, eb, threads, iv in cases:
        p = oracle.default_params(); p.quantization_intervals = iv
        ref = oracle.omp_compress(d, eb, threads, META, p)
        got, n, st = ctx.compress_omp(d.ctypes.data, False, d.shape, d.dtype, eb, threads, META, sz_amd.api.szhip_params(100, 0.99, 65536, iv))
        assert n == len(ref) and got == ref, name
        out = np.empty_like(d)
        buf = ctypes.create_string_buffer(ref, len(ref))
        ctx.decompress_omp(ctypes.addressof(buf), False, len(ref), len(META), d.shape, d.dtype, out.ctypes.data, False)
        want = oracle.omp_decompress(ref, len(META), d.shape, d.dtype)
        assert np.array_equal(_bits(out), _bits(want)), name
        ok = np.isfinite(d)
        assert float(np.abs(out[ok].astype(np.float64) - d[ok].astype(np.float64)).max()) <= eb, name


def _recorded(ctx, oracle, names):
    import record_reference_omp as R
    for name in names:
        rec = RECORDED[name]
        d = R.make_field(rec["field"], tuple(rec["shape"]), rec["dtype"])
        meta = bytes.fromhex(rec["meta_hex"])
        got, n, st = ctx.compress_omp(d.ctypes.data, False, d.shape, d.dtype, rec["eb"], rec["threads"], meta)
        assert n == rec["stream_len"] and got[:len(meta)] == meta, name
        assert hashlib.md5(got[len(meta):]).hexdigest() == rec["body_md5"], name              # the reference's own bytes
        out = np.empty_like(d)
        buf = ctypes.create_string_buffer(got, len(got))
        ctx.decompress_omp(ctypes.addressof(buf), False, len(got), len(meta), d.shape, d.dtype, out.ctypes.data, False)
        if rec["decoded_md5"] is not None:
            assert hashlib.md5(out.tobytes()).hexdigest() == rec["decoded_md5"], name         # the reference's own decoded array
        else:                                                                                 # float64: no reference decoder (tests/test_omp_container.py)
            want = oracle.omp_decompress(got, len(meta), d.shape, d.dtype)
            assert np.array_equal(_bits(out), _bits(want)), name


def _refusals(ctx):
    import sz_amd
    d = np.zeros((33, 16, 16), dtype=np.float32)
    with pytest.raises(sz_amd.SZError, match="does not divide"):
        ctx.compress_omp(d.ctypes.data, False, d.shape, d.dtype, 1e-3, 8, META)
    d = np.zeros((64, 64, 8), dtype=np.float32)
    with pytest.raises(sz_amd.SZError, match="box face"):
        ctx.compress_omp(d.ctypes.data, False, d.shape, d.dtype, 1e-3, 1, META)
    out = np.zeros((16, 16, 16), dtype=np.float32)
    junk = ctypes.create_string_buffer(bytes(64), 64)
    with pytest.raises(sz_amd.SZError):
        ctx.decompress_omp(ctypes.addressof(junk), False, 64, 32, out.shape, out.dtype, out.ctypes.data, False)


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


def test_omp_container_on_cpu_shim_matches_oracle(oracle, shim_ctx):
    _run_cases(shim_ctx, oracle, _cases())
    _refusals(shim_ctx)


def test_omp_container_many_boxes_layout_on_cpu_shim(oracle, shim_ctx, monkeypatch):
    """the two-launch form of the boxes' layout (payload sizes by a wavefront per box, then the scans), which arrays of more than 8192 boxes take"""
    monkeypatch.setenv("SZ_HIP_OMP_MANY", "1")
    _run_cases(shim_ctx, oracle, [c for c in _cases() if c[0] in ("col-S-8x64x64-t8", "col-S-f64-8x64x64-t8", "col-one-noisy-box-t16")])


def test_omp_container_on_cpu_shim_gives_the_recorded_reference_bytes(oracle, shim_ctx):
    _recorded(shim_ctx, oracle, ["L-32-f32-t8", "S-64-f32-t64", "S-64x32x96-f32-t16", "Sfill-64x32x32-f32-t8", "Snan-32-f32-t8", "S-8x64x64-f64-t8", "M-32x64x64-f64-t16",
                                "S-8x1x66-f32-t1", "S-16x1x40-f64-t1"])         # (the last two: dim 1 one value wide -- the interval optimiser's walk, k_sample_walk)


@pytest.mark.slow
def test_omp_container_on_cpu_shim_recorded_reference_bytes_large(oracle, shim_ctx):
    _recorded(shim_ctx, oracle, ["S-64-f32-t8", "M-64-f32-t8", "S-128x64x64-f32-t32", "S-64-f64-t8", "Sfill-16x64x64-f64-t8"])


def test_truncated_and_damaged_omp_streams_are_refused_on_cpu_shim(oracle, shim_ctx):
    import sz_amd
    from sz_amd.fields import s_field
    d = s_field(16, 16, 16)
    ref = oracle.omp_compress(d, 1e-3, 8, META)
    out = np.empty_like(d)
    for cut in (len(META) + 3, len(META) + 30, len(ref) // 2, len(ref) - 1):
        buf = ctypes.create_string_buffer(ref[:cut], cut)
        with pytest.raises(sz_amd.SZError):
            shim_ctx.decompress_omp(ctypes.addressof(buf), False, cut, len(META), d.shape, d.dtype, out.ctypes.data, False)
    bad = bytearray(ref); bad[len(META):len(META) + 4] = (7).to_bytes(4, "big")          # a thread_num that is not this array's grid
    buf = ctypes.create_string_buffer(bytes(bad), len(bad))
    with pytest.raises(sz_amd.SZError):
        shim_ctx.decompress_omp(ctypes.addressof(buf), False, len(bad), len(META), d.shape, d.dtype, out.ctypes.data, False)
    # a verbatim-value count that does not fit the box's codes (the table entry of box 0 raised by one, the stream lengthened to match)
    tree_bytes = int.from_bytes(ref[len(META) + 12:len(META) + 16], "big")
    at = len(META) + 20 + tree_bytes
    bad = bytearray(ref); bad[at:at + 4] = (int.from_bytes(ref[at:at + 4], "little") + 1).to_bytes(4, "little"); bad += bytes(4)
    buf = ctypes.create_string_buffer(bytes(bad), len(bad))
    with pytest.raises(sz_amd.SZError):
        shim_ctx.decompress_omp(ctypes.addressof(buf), False, len(bad), len(META), d.shape, d.dtype, out.ctypes.data, False)


def _api_round(L, oracle):
    """SZ_compress_float_3D_MDQ_openmp / decompressDataSeries_float_3D_openmp (sz/include/sz_omp.h) on the recorded reference cases: the
    WHOLE stream, parameter bytes included (but for the one byte the reference does not write the same way twice)."""
    import record_reference_omp as R
    sz = ctypes.c_size_t
    L.SZ_Init.argtypes = [ctypes.c_char_p]
    L.SZ_compress_float_3D_MDQ_openmp.restype = ctypes.c_void_p
    L.SZ_compress_float_3D_MDQ_openmp.argtypes = [ctypes.c_void_p, sz, sz, sz, ctypes.c_float, ctypes.POINTER(sz)]
    L.SZ_compress_double_3D_MDQ_openmp.restype = ctypes.c_void_p
    L.SZ_compress_double_3D_MDQ_openmp.argtypes = [ctypes.c_void_p, sz, sz, sz, ctypes.c_double, ctypes.POINTER(sz)]
    L.decompressDataSeries_float_3D_openmp.argtypes = [ctypes.POINTER(ctypes.c_void_p), sz, sz, sz, ctypes.c_void_p]
    L.decompressDataSeries_double_3D_openmp.argtypes = [ctypes.POINTER(ctypes.c_void_p), sz, sz, sz, ctypes.c_void_p]
    L.free.argtypes = [ctypes.c_void_p]
    assert L.SZ_Init(os.path.join(ROOT, "tests", "golden", "sz_speed.config").encode()) == 0
    try:
        for name in ("L-32-f32-t8", "S-64x32x96-f32-t16"):
            rec = RECORDED[name]
            d = R.make_field(rec["field"], tuple(rec["shape"]), rec["dtype"])
            L.SZ_hip_set_omp_threads(rec["threads"])
            n = sz(0)
            p = L.SZ_compress_float_3D_MDQ_openmp(d.ctypes.data, *d.shape, rec["eb"], ctypes.byref(n))
            assert p and n.value == rec["stream_len"], name
            s = ctypes.string_at(p, n.value)
            L.free(p)
            meta = bytes.fromhex(rec["meta_hex"])
            assert hashlib.md5(s[len(meta):]).hexdigest() == rec["body_md5"], name
            assert [i for i in range(len(meta)) if s[i] != meta[i]] in ([], [19]), name           # byte 19: not stable in the reference itself
            out = ctypes.c_void_p()
            buf = ctypes.create_string_buffer(s[len(meta):], len(s) - len(meta))
            L.decompressDataSeries_float_3D_openmp(ctypes.byref(out), *d.shape, buf)
            assert out.value, name
            a = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_float)), shape=(d.size,)).copy()
            L.free(out)
            assert hashlib.md5(a.tobytes()).hexdigest() == rec["decoded_md5"], name
        # the default box count, and the double entry points against the oracle
        L.SZ_hip_set_omp_threads(0)
        from sz_amd.fields import s_field
        d = s_field(32, 32, 64, np.float64)
        n = sz(0)
        p = L.SZ_compress_double_3D_MDQ_openmp(d.ctypes.data, *d.shape, 1e-5, ctypes.byref(n))
        s = ctypes.string_at(p, n.value)
        L.free(p)
        assert int.from_bytes(s[32:36], "big") == 2                                                # 2 boxes of 32 x 32 x 32
        assert s[32:] == oracle.omp_compress(d, 1e-5, 2, s[:32])[32:]
        out = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(s[32:], len(s) - 32)
        L.decompressDataSeries_double_3D_openmp(ctypes.byref(out), *d.shape, buf)
        a = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_double)), shape=(d.size,)).copy().reshape(d.shape)
        L.free(out)
        assert np.array_equal(_bits(a), _bits(oracle.omp_decompress(s, 32, d.shape, d.dtype)))
    finally:
        L.SZ_hip_set_omp_threads(0)
        L.SZ_Finalize()


def test_reference_named_omp_entry_points_on_cpu_shim(oracle, built):
    import sim_lib
    _api_round(ctypes.CDLL(sim_lib.shim_path()), oracle)


@pytest.mark.gpu
def test_hip_reference_named_omp_entry_points(oracle, built):
    from sz_amd import api
    _api_round(ctypes.CDLL(api.lib_path()), oracle)


@pytest.mark.gpu
def test_hip_omp_container_matches_oracle(oracle, built):
    import sz_amd
    ctx = sz_amd.HipContext(0)
    _run_cases(ctx, oracle, _cases())
    _recorded(ctx, oracle, sorted(RECORDED))
    _refusals(ctx)
    ctx.close()


@pytest.mark.gpu
def test_hip_omp_container_256_against_oracle_and_512_round_trip(oracle, built):
    import sz_amd
    from sz_amd.fields import s_field
    ctx = sz_amd.HipContext(0)
    d = s_field(256, 256, 256)
    ref = oracle.omp_compress(d, 1e-4, 512, META)                                        # 512 boxes of 32^3
    got, n, st = ctx.compress_omp(d.ctypes.data, False, d.shape, d.dtype, 1e-4, 512, META)
    assert got == ref
    out = np.empty_like(d)
    buf = ctypes.create_string_buffer(ref, len(ref))
    ctx.decompress_omp(ctypes.addressof(buf), False, len(ref), len(META), d.shape, d.dtype, out.ctypes.data, False)
    assert np.array_equal(_bits(out), _bits(oracle.omp_decompress(ref, len(META), d.shape, d.dtype)))
    d = s_field(512, 512, 512)
    got, n, st = ctx.compress_omp(d.ctypes.data, False, d.shape, d.dtype, 1e-4, 4096, META)
    assert n < d.nbytes / 8
    out = np.empty_like(d)
    buf = ctypes.create_string_buffer(got, len(got))
    ctx.decompress_omp(ctypes.addressof(buf), False, len(got), len(META), d.shape, d.dtype, out.ctypes.data, False)
    assert float(np.abs(out.astype(np.float64) - d).max()) <= 1e-4
    # idempotence: the decoded array compresses to a stream that decodes to itself
    got2, n2, _ = ctx.compress_omp(out.ctypes.data, False, out.shape, out.dtype, 1e-4, 4096, META)
    out2 = np.empty_like(d)
    buf2 = ctypes.create_string_buffer(got2, len(got2))
    ctx.decompress_omp(ctypes.addressof(buf2), False, len(got2), len(META), d.shape, d.dtype, out2.ctypes.data, False)
    assert float(np.abs(out2.astype(np.float64) - out).max()) <= 1e-4
    ctx.close()


# ---- inputs with fill values and NaN through the other paths (SZ 2.1 3-D / 2-D, the 1-D chain): found by tools/omp_diff_fuzz.py at the end of
# round 3 -- the interval optimisers convert (|prediction error| / eb + 1) / 2 to `unsigned long` (sz_float.c:4664, :5092), and outside that type's
# range the stream depends on what the reference's x86-64 build does (a quotient >= 2^64 lands in the FIRST bin, a NaN in the last); the range
# scan skips NaN (dataCompression.c:97-113).  (In this file because the GPU variant was added after round 3's hardware time; green on hardware since.)
def _fill_value_cases():
    from sz_amd.fields import s_field
    rng = np.random.default_rng(3)
    for shape in ((24, 30, 36), (40, 50), (5000,)):
        for with_nan in (False, True):
            d = s_field(*((1,) * (3 - len(shape)) + shape)).reshape(shape).copy()
            f = d.ravel()
            f[rng.integers(0, f.size, f.size // 7)] = 1e30
            if with_nan:
                f[rng.integers(1, f.size, 5)] = np.nan
            yield shape, with_nan, d


def _fill_value_round(oracle):
    import sz_amd
    assert sz_amd.SZ_Init(os.path.join(ROOT, "tests", "golden", "sz_speed.config")) == 0
    try:
        for shape, with_nan, d in _fill_value_cases():
            ref, _ = oracle.compress(d, oracle.ABS, 1e-4)
            assert sz_amd.SZ_compress_args(d, sz_amd.ABS, 1e-4) == ref, (shape, with_nan)
    finally:
        sz_amd.SZ_Finalize()


def test_fill_values_and_nan_give_the_oracle_streams_on_cpu_shim(oracle, built):
    import sim_lib
    from sz_amd import api
    saved = api._lib
    api._lib = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    try:
        _fill_value_round(oracle)
    finally:
        api._lib = saved


@pytest.mark.gpu
def test_hip_fill_values_and_nan_give_the_oracle_streams(oracle, built):
    _fill_value_round(oracle)


def test_bench_omp_object_rehearsal_on_cpu_shim(built):
    """bench.py --omp-boxes (the opt-in object for the first hardware run) rehearsed on the shim: the code path runs and its round trip holds
    the bound.  Nothing it prints is a measurement."""
    import subprocess
    import sim_lib
    env = dict(os.environ, SZ_AMD_LIB=sim_lib.shim_path())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--dry-run", "--edge", "32",
                        "--full", "--omp-boxes", "8"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-800:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"metric"')][-1])
    o = line["omp_container"]
    assert o["boxes"] == 8 and o["out_bytes"] > 0 and o["max_abs_err"] <= 1e-4


# ---- GPU replay of the reference outputs recorded after the last hardware run (tests/ref_cases.py: fill-1e30-*, nan-sparse-*)
import ref_cases  # noqa: E402
import test_ref_recorded as _TR  # noqa: E402

_NEW = [c for c in ref_cases.CASES if _TR._new_since_last_hardware_run(c)]


@pytest.mark.gpu
@pytest.mark.parametrize("c", _NEW, ids=[c["name"] for c in _NEW])
def test_hip_reproduces_reference_outputs_recorded_after_the_last_hardware_run(built, c, tmp_path):
    _TR.check_hip_reproduces(c, tmp_path)
    r = _TR.REC[c["name"]]
    if "stream_file" in r and r.get("decoded_md5"):               # and decodes the reference-made stream
        import sz_amd
        stream = open(os.path.join(ROOT, "tests", "golden", r["stream_file"]), "rb").read()
        dec = sz_amd.SZ_decompress(stream, tuple(r["shape"]), np.dtype(r["dtype"]))
        assert hashlib.md5(dec.tobytes()).hexdigest() == r["decoded_md5"], c["name"]
