"""SZ_compress_args over many same-shape arrays in one call: SZ_hip_compress_args_batch, SZ_hip_decompress_batch, SZ_hip_compare_batch (include/sz.h) and their
Python mirror.  Every case runs on the CPU shim (tests/sim) and, marked gpu, on the device, where the arrays sit at guarded device pointers.

Each stream of a batch is checked two ways:
  (a) against the single call: streams[i] equals SZ_compress_args of this library under SZ_HIP_MODE=omp for array i alone, as the first call after the same SZ_Init;
  (b) against the oracle, independent of the code under test: the test computes the array's range with numpy in the array's type and the bound by the reference's
      rule (dataCompression.c:288-332, conf.c:54-65); a container item equals oracle.omp_compress(a_i, eb_i, 8, streams[i][:32]) (the parameter bytes are the
      stream's own, the mark in byte 19 among them), a constant item equals oracle.compress(a_i, mode, ...).
What keeps a loop over single calls from passing: batched[i] == 1 exactly for the items with range > bound, and SZ_hip_last_stats().quant_kernel_launches counts one
sweep launch per form, whatever the number of arrays.

The arrays: S-field slices scaled by 1, 1e3 and 1e-3 (their relative bounds differ by six orders of magnitude), an S-field with a box of noise, one with 1e30
and a NaN inside (the range skips the NaN, the 1e30 makes the bound huge), a constant array, and an array of two values a hair apart (its range is below an ABS
bound, but not below a relative one).  Shapes as tests/test_omp_batch.py with SZ_HIP_OMP_THREADS=8: (8, 64, 64) boxes with 32 x 32 faces (k_omp_col), (16, 16, 16)
(k_omp_box)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ptr_cases as P  # noqa: E402
from test_omp_batch import _field, _form, _noisy  # noqa: E402

f32, f64 = np.float32, np.float64
COL, BOX = (8, 64, 64), (16, 16, 16)
THREADS, MARK = 8, 0x4F
CONFIG = os.path.join(ROOT, "tests", "golden", "sz_speed.config")     # psnr = 80, normErr = 0.05, predThreshold = 0.99, szMode = SZ_BEST_SPEED
ABS, REL, ABS_AND_REL, ABS_OR_REL, PSNR, NORM, PW_REL = 0, 1, 2, 3, 4, 5, 10
BACKENDS = [pytest.param("gpu", marks=pytest.mark.gpu, id="on_the_gpu"), pytest.param("shim", id="on_the_cpu_shim")]
_ARR = {}


@pytest.fixture
def shim(built):
    import sim_lib
    from sz_amd import api
    old = api._lib
    api._lib = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    yield
    api._lib.SZ_Finalize()
    api._lib = old


@pytest.fixture
def gpu(built):
    import sz_amd
    yield
    sz_amd.SZ_Finalize()


@pytest.fixture(params=BACKENDS)
def dev(request, monkeypatch):
    """True: the product library on the GPU; False: the same code over the CPU shim.  The box count is forced to 8, SZ_HIP_MODE is NOT set (the batch call must not
    need it).  Pointers into guarded allocations are passed as DEVICE pointers on both (on the shim device memory is host memory)"""
    monkeypatch.setenv("SZ_HIP_OMP_THREADS", str(THREADS))
    monkeypatch.delenv("SZ_HIP_MODE", raising=False)
    request.getfixturevalue("gpu" if request.param == "gpu" else "shim")
    return request.param == "gpu"


def init():
    import sz_amd
    assert sz_amd.SZ_Init(CONFIG) == 0


def arrays(shape, dtype):
    key = (shape, np.dtype(dtype).name)
    if key not in _ARR:
        from sz_amd.fields import s_field
        s = s_field(*shape, np.dtype(dtype).type)
        special = s_field(*shape, np.dtype(dtype).type, z0=8)
        special.ravel()[5] = 1e30
        special.ravel()[special.size // 2] = np.nan
        hair = np.full(shape, 1.0, dtype=dtype)
        hair.ravel()[1::2] = np.nextafter(dtype(1.0), dtype(2.0))
        out = [("s", s), ("s*1e3", (s * dtype(1e3)).astype(dtype)), ("s*1e-3", (s * dtype(1e-3)).astype(dtype)), ("noisy", _noisy(shape, dtype)),
               ("special", special), ("constant", np.full(shape, 1.5, dtype=dtype)), ("hair", hair)]
        for _, a in out:
            a.setflags(write=False)
        _ARR[key] = [(k, np.ascontiguousarray(a)) for k, a in out]
    return _ARR[key]


def bound_of(a, mode, abs_b, rel):
    """(range, bound) of array `a` by the reference's rule: the range is max - min in the array's type with NaNs skipped (computeRangeSize_float), the bound
    getRealPrecision_float's (AND / OR narrow both operands to float for float data), conf.c:54-65 for PSNR (psnr 80, predThreshold the float 0.99) and NORM (0.05)"""
    T = a.dtype.type
    with np.errstate(all="ignore"):
        rng = float(T(np.nanmax(a)) - T(np.nanmin(a)))
    if mode == ABS:
        return rng, abs_b
    if mode == REL:
        return rng, rel * rng
    if mode in (ABS_AND_REL, ABS_OR_REL):
        x, y = (float(f32(abs_b)), float(f32(rel * rng))) if T is f32 else (abs_b, rel * rng)
        return rng, min(x, y) if mode == ABS_AND_REL else max(x, y)
    if mode == PSNR:
        return rng, rng * math.pow(10, (80.0 + 10 * math.log10(1 - 2.0 / 3.0 * float(f32(0.99)))) / -20)
    if mode == NORM:
        return rng, math.sqrt(3.0 / a.size) * 0.05
    raise KeyError(mode)


def place(dev, arrs, offs):
    return [P.carve(a.nbytes, o, device=dev).put(a) for a, o in zip(arrs, offs)]


def single(a, mode, abs_b, rel, monkeypatch):
    """SZ_compress_args under SZ_HIP_MODE=omp for the array alone, as the first call after SZ_Init"""
    import sz_amd
    init()
    monkeypatch.setenv("SZ_HIP_MODE", "omp")
    try:
        return sz_amd.SZ_compress_args(a, mode, abs_b, rel)
    finally:
        monkeypatch.delenv("SZ_HIP_MODE")


def run_batch(dev, arrs, mode, abs_b, rel, offs=None, host=False):
    import sz_amd
    offs = offs or [(0, arrs[0].itemsize, 8)[i % 3] for i in range(len(arrs))]
    regs = None if host else place(dev, arrs, offs)
    ptrs = [a.ctypes.data for a in arrs] if host else [r.ptr for r in regs]
    init()
    rc, streams, batched = sz_amd.SZ_hip_compress_args_batch(ptrs, not host, arrs[0].shape, arrs[0].dtype, mode, abs_b, rel)
    launches = sz_amd.SZ_hip_last_stats().quant_kernel_launches
    assert rc == 0
    if regs:
        for r, a in zip(regs, arrs):
            r.check("input")
            assert np.array_equal(r.get(), a.reshape(-1).view(np.uint8)), "an input was written"
    return streams, batched, launches, ptrs


def check_streams(oracle, monkeypatch, names, arrs, streams, batched, mode, abs_b, rel, what):
    want_batched = []
    for i, (k, a) in enumerate(zip(names, arrs)):
        rng, eb = bound_of(a, mode, abs_b, rel)
        container = rng > eb
        want_batched.append(1 if container else 0)
        print(f"{what} item {i} ({k}): range {rng!r}, bound {eb!r}, {'container' if container else 'constant'}, batched {batched[i]}, {len(streams[i])} bytes")
        one = single(a, mode, abs_b, rel, monkeypatch)
        assert streams[i] == one, f"{what} item {i} ({k}): the batch's stream ({len(streams[i])} bytes) is not SZ_compress_args' ({len(one)} bytes)"
        if container:
            assert streams[i][19] == MARK
            ref = oracle.omp_compress(a, eb, THREADS, streams[i][:32])
            assert streams[i] == ref, f"{what} item {i} ({k}): not the oracle's container at the bound {eb!r}"
        else:
            ref, _ = oracle.compress(a, mode, abs_b, rel)
            assert streams[i] == ref, f"{what} item {i} ({k}): not the oracle's constant stream"
    assert list(batched) == want_batched, f"{what}: batched = {list(batched)}, the items with range > bound are {want_batched}"
    return want_batched


MODES = [("REL", REL, 0.0, 1e-3), ("ABS_AND_REL", ABS_AND_REL, 1e-3, 1e-3), ("ABS_OR_REL", ABS_OR_REL, 1e-3, 1e-3), ("PSNR", PSNR, 0.0, 0.0), ("NORM", NORM, 0.0, 0.0),
         ("ABS", ABS, 1e-3, 0.0)]


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("shape", (COL, BOX), ids=("col", "box"))
@pytest.mark.parametrize("name,mode,abs_b,rel", MODES, ids=[m[0] for m in MODES])
def test_streams_are_the_single_calls_and_the_oracles(dev, oracle, monkeypatch, name, mode, abs_b, rel, shape, dtype):
    """(with abs 1e-3 and rel 1e-3 the absolute bound wins AND for the arrays of range > 1 and loses for s*1e-3 and hair; the other way round for OR)"""
    names, arrs = zip(*arrays(shape, dtype))
    streams, batched, launches, ptrs = run_batch(dev, arrs, mode, abs_b, rel)
    want = check_streams(oracle, monkeypatch, names, arrs, streams, batched, mode, abs_b, rel, f"{name} {shape} {np.dtype(dtype).name}")
    # (a container whose optimiser picked more than 1024 intervals -- read off its oracle-checked stream -- runs through the single call inside the batch: szhip.h)
    esz = np.dtype(dtype).itemsize
    forms = {_form(shape, p) for p, b, s in zip(ptrs, want, streams) if b and _field(s, esz, "intervals") <= 1024}
    print(f"sweep launches {launches}, forms {sorted(forms)}")
    assert launches == len(forms), f"{launches} sweep launches for the forms {sorted(forms)} of the shared launches' items"


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("count", (1, 2, 3, 4, 5, 6))
def test_counts_host_arrays_and_the_round_trip(dev, oracle, monkeypatch, count, dtype):
    """`count` host arrays under REL 1e-3 (the constant array among them from count 6 on); the decode is bit for bit SZ_decompress of each stream, the oracle's decode
    of a container stays within its bound, and the batched report over the round trip finds no point over the bound in the stream's header"""
    import sz_amd
    shape = BOX
    names, arrs = zip(*arrays(shape, dtype)[:count])
    streams, batched, launches, _ = run_batch(dev, arrs, REL, 0.0, 1e-3, host=True)
    want = check_streams(oracle, monkeypatch, names, arrs, streams, batched, REL, 0.0, 1e-3, f"{count} host arrays")
    assert launches == (1 if any(b and _field(s, np.dtype(dtype).itemsize, "intervals") <= 1024 for b, s in zip(want, streams)) else 0)            # (staged at multiples of 16: one form)
    esz = np.dtype(dtype).itemsize
    outs = place(dev, [np.zeros(shape, dtype) for _ in range(count)], [(0, esz, 8)[i % 3] for i in range(count)])
    init()
    assert sz_amd.SZ_hip_decompress_batch(streams, [r.ptr for r in outs], True, shape, dtype) == 0
    decs, bounds = [], []
    for i, (a, s, r) in enumerate(zip(arrs, streams, outs)):
        r.check(f"output {i}")
        got = r.get().view(dtype).reshape(shape)
        init()
        ref = sz_amd.SZ_decompress(s, shape, dtype)
        assert np.array_equal(P.bits(got), P.bits(ref)), f"item {i}: the batched decode differs from SZ_decompress"
        rng, eb = bound_of(a, REL, 0.0, 1e-3)
        if want[i]:
            hdr = np.frombuffer(s[36:36 + esz], dtype=">f4" if dtype is f32 else ">f8")[0]
            assert float(hdr) == float(dtype(eb)), f"item {i}: the header's bound {hdr!r}, the rule gives {eb!r}"
            od = oracle.omp_decompress(s, 32, shape, dtype)
            ok = np.isfinite(a)
            assert float(np.abs(od[ok].astype(f64) - a[ok].astype(f64)).max()) <= float(hdr), f"item {i}: the oracle's decode leaves its bound"
            bounds.append(float(hdr))
        else:
            bounds.append(eb)
        decs.append(np.ascontiguousarray(got))
    ro = place(dev, arrs, [0] * count)
    rd = place(dev, decs, [esz] * count)
    qs = sz_amd.SZ_hip_compare_batch([r.ptr for r in ro], [r.ptr for r in rd], True, shape, dtype, bounds)
    assert sz_amd.SZ_hip_last_stats().quant_kernel_launches == 1
    for i, q in enumerate(qs):
        print(f"item {i}: max error {q.max_abs_err!r}, bound {bounds[i]!r}, over {q.n_over_abs}")
        assert q.n_over_abs == 0 and q.n == arrs[i].size, f"item {i}: {q}"
        assert q.raw == sz_amd.SZ_hip_compare(arrs[i], decs[i], bounds[i]).raw, f"item {i}: not SZ_hip_compare's record"


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
def test_decode_of_mixed_and_damaged_streams(dev, oracle, dtype):
    """a batch's streams with an SZ 2.1 stream mixed in decode through their own paths; one truncated stream gives SZ_NSCS with the others decoded"""
    import sz_amd
    shape = BOX
    names, arrs = zip(*arrays(shape, dtype))
    streams, batched, _, _ = run_batch(dev, arrs, REL, 0.0, 1e-3)
    init()
    sz21 = sz_amd.SZ_compress_args(arrs[0], ABS, 1e-3)               # (SZ_HIP_MODE is not set: the SZ 2.1 stream)
    assert sz21[19] != MARK
    mixed = list(streams) + [sz21]
    want = []
    for s in mixed:
        init()
        want.append(sz_amd.SZ_decompress(s, shape, dtype))
    esz = np.dtype(dtype).itemsize
    outs = place(dev, [np.zeros(shape, dtype) for _ in mixed], [(0, esz, 8)[i % 3] for i in range(len(mixed))])
    init()
    assert sz_amd.SZ_hip_decompress_batch(mixed, [r.ptr for r in outs], True, shape, dtype) == 0
    for i, (r, w) in enumerate(zip(outs, want)):
        r.check(f"output {i}")
        assert np.array_equal(P.bits(r.get().view(dtype)), P.bits(w)), f"stream {i}: the batched decode differs from SZ_decompress"
    damaged = list(mixed)
    damaged[1] = damaged[1][:len(damaged[1]) // 2]
    outs = place(dev, [np.zeros(shape, dtype) for _ in mixed], [0] * len(mixed))
    init()
    assert sz_amd.SZ_hip_decompress_batch(damaged, [r.ptr for r in outs], True, shape, dtype, raise_on_error=False) == sz_amd.SZ_NSCS
    for i, (r, w) in enumerate(zip(outs, want)):
        r.check(f"output {i}")
        if i != 1:
            assert np.array_equal(P.bits(r.get().view(dtype)), P.bits(w)), f"stream {i} did not decode beside the damaged one"


def test_refusals(dev, tmp_path):
    import sz_amd
    a = arrays(BOX, f32)[0][1]
    r = place(dev, [a], [0])[0]
    init()
    for what, shape, mode in (("a PW_REL mode", BOX, PW_REL), ("a shape without a box grid", (15, 16, 16), REL)):
        rc, streams, _ = sz_amd.SZ_hip_compress_args_batch([r.ptr], True, shape, f32, mode, 1e-3, 1e-3, raise_on_error=False)
        assert rc == sz_amd.SZ_NSCS and streams == [None], what
    cfg = tmp_path / "sz.config"
    cfg.write_text(open(CONFIG).read().replace("szMode = SZ_BEST_SPEED", "szMode = SZ_BEST_COMPRESSION"))
    assert sz_amd.SZ_Init(str(cfg)) == 0
    rc, streams, _ = sz_amd.SZ_hip_compress_args_batch([r.ptr], True, BOX, f32, REL, 0.0, 1e-3, raise_on_error=False)
    assert rc == sz_amd.SZ_NSCS and streams == [None], "a szMode that is not SZ_BEST_SPEED"
    r.check("refusals")
