"""The drop-in calls for arrays and streams in device memory (include/sz.h: SZ_hip_compress_device, SZ_hip_compress_device_into, SZ_hip_decompress_device) and the
four copy-shaped kernels behind them (include/szhip.h: szhip_store_be, szhip_load_be, szhip_fill, szhip_clamp; sz_amd/csrc/szh_store.h).

The bar: the device entry returns byte for byte what SZ_compress_args returns for a host copy of the array under the same configuration file, decodes bit for bit
what SZ_decompress decodes, writes nothing outside its outputs and never writes its input.  Arrays, streams and buffers are regions carved out of larger allocations
at chosen byte offsets with 0xA5 guards all round (tests/ptr_cases.py).

GPU (-m gpu): torch uint8 tensors as device memory, every case of tests/ref_cases.py.  CPU: the same host code and the same kernel bodies through the HIP-on-CPU
shim (tests/sim), where "device" memory is host memory; the shim runs every lane as a fibre, so there the cases of at most SHIM_FAST values run, as
tests/test_device_pointers.py runs the smallest arrays of its lists, and one larger case of every stream kind they leave out (SHIM_KINDS) with fewer placements."""
import ctypes
import hashlib
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ptr_cases as P  # noqa: E402
import ref_cases  # noqa: E402
import test_ref_recorded as R  # noqa: E402

f32, f64 = np.float32, np.float64
ABS, PW_REL = ref_cases.ABS, ref_cases.PW_REL
SHIM_FAST = 4200                     # values
# the stream kinds no case of at most SHIM_FAST values has: SZ 2.1 with regression blocks, the lossless stage, MSST19 and the log-domain form with sign bytes
SHIM_KINDS = ["C1-f32", "C1-zstd", "pwr-first-negative-3D-f32", "pwrlog-negative-3D-f32"]


# ------------------------------------------------------------------------------------------------------------------ cases

def _raw_f32(n):
    return np.random.default_rng(5).standard_normal(n).astype(f32)


def _raw_f64(shape):
    return np.random.default_rng(5).standard_normal(shape)


def _zeros_2000():
    r = np.random.default_rng(5)
    d = r.standard_normal(2000).astype(f32)
    d[r.random(2000) < 0.05] = 0
    d[0] = 0.37                      # (the MSST19 scan starts nearZero from element 0: a zero there leaves the zeros in place)
    return d


case = ref_cases.case
# item 4: the raw store at the kernel's edges (flag byte 0x50 on the CPU oracle for every one of them) ...
RAW = [case(f"raw-1d-{n}-f32", lambda n=n: _raw_f32(n), abs=1e-7) for n in (21, 1023, 1024, 1025, 4097)] + \
      [case("raw-7x9x11-f32", lambda: _raw_f32(693).reshape(7, 9, 11), abs=1e-7), case("raw-33x47-f32", lambda: _raw_f32(1551).reshape(33, 47), abs=1e-7)] + \
      [case(f"raw-{a}x{b}-f64", lambda a=a, b=b: _raw_f64((a, b)), abs=1e-15) for a, b in ((3, 341), (4, 256), (5, 205), (17, 241))] + \
      [case("raw-7x9x11-f64", lambda: _raw_f64((7, 9, 11)), abs=1e-15), case("raw-1d-21-f64", lambda: _raw_f64(21), abs=1e-15)]
# ... and the constant stream
CONST = [case(f"const-{n}-{np.dtype(t).name}", lambda n=n, t=t: np.full(n, 3.25, t), abs=1e-3) for n in (21, 1025) for t in (f32, f64)] + \
        [case(f"const-5x6x7-{np.dtype(t).name}", lambda t=t: np.full((5, 6, 7), -2.5, t), abs=1e-3) for t in (f32, f64)]
# the OpenMP container (SZ_HIP_MODE=omp): a 3-D array the box rule divides, both types, and one with protectValueRange
OMP = [case("omp-s64-f32", lambda: P._array("omp-s64-t8")[0]), case("omp-s16x24x40-f64", lambda: P._array("omp-s16x24x40-t16")[0].astype(f64), abs=1e-3),
       case("omp-s16x24x40-protect-f32", lambda: P._array("omp-s16x24x40-t16")[0], abs=1e-3, protectValueRange="YES"),
       case("omp-s8x8x18-f32", lambda: P._array("omp-s8x8x18-t4")[0], abs=1e-3)]
CLAMP = ["S-protectValueRange-f64", "sz14-S-protect-f32"]

_DATA = {}


def data_of(c):
    if c["name"] not in _DATA:
        d = np.ascontiguousarray(c["data"]())
        d.setflags(write=False)
        _DATA[c["name"]] = d
    return _DATA[c["name"]]


def _size(c):
    r = R.REC.get(c["name"])
    return int(np.prod(r["shape"])) if r else data_of(c).size


def _ids(cases):
    return [c["name"] for c in cases]


def _shim_params(cases):
    """the cases a shim test runs"""
    return [pytest.param(c, id=c["name"]) for c in cases if _size(c) <= SHIM_FAST or c["name"] in SHIM_KINDS]


def _placements(c, full):
    """on the shim: every placement the test names, for a SHIM_KINDS case the last of them alone"""
    return full if _size(c) <= SHIM_FAST else full[-1:]


ALL = ref_cases.CASES
SPEED = [c for c in ALL if not R._wrapped(c)]
DECODE = [c for c in ALL]            # (the <= 20-value case goes through the same test)


# ------------------------------------------------------------------------------------------------------------------ the library under test

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


class Conf:
    """One configuration file per case; init() puts the library back to it, so that every call runs `under the same config file` whatever the call before it
    left in confparams_cpr / exe_params (the interval count of the last stream, the sticky accelerate_pw_rel_compression switch)."""

    def __init__(self, c, tmp_path, omp=False):
        self.path = str(tmp_path / "sz.config")
        ref_cases.write_config(self.path, c["conf"])
        self.omp = omp

    def init(self):
        import sz_amd
        assert sz_amd.SZ_Init(self.path) == 0

    def __enter__(self):
        if self.omp:
            os.environ["SZ_HIP_MODE"] = "omp"
        return self

    def __exit__(self, *a):
        os.environ.pop("SZ_HIP_MODE", None)


def _args(c):
    return c["mode"], c["abs"], c["rel"], c["pwr"]


def _host_stream(conf, c):
    import sz_amd
    conf.init()
    return sz_amd.SZ_compress_args(data_of(c), *_args(c))


def _same_bytes(got, want, what):
    got, want = np.frombuffer(bytes(got), dtype=np.uint8), np.frombuffer(bytes(want), dtype=np.uint8)
    assert got.size == want.size, f"{what}: {got.size} bytes, SZ_compress_args returns {want.size}"
    d = np.nonzero(got != want)[0]
    assert d.size == 0, f"{what}: {d.size} bytes differ from SZ_compress_args's, the first at {int(d[0])} (0x{int(got[d[0]]):02x}, want 0x{int(want[d[0]]):02x})"


def _same_bits(got, want, what):
    d = np.nonzero(P.bits(got) != P.bits(want))[0]
    assert d.size == 0, f"{what}: {d.size} values differ from SZ_decompress's, the first at {int(d[0])}"


def _unchanged(src, x, what):
    src.check(what + " (input)")
    assert np.array_equal(src.get(), x.reshape(-1).view(np.uint8)), f"{what}: the input array was written"


def _recorded(c, d, stream):
    """the stream against the reference's recorded output, where there is one for this input"""
    r = R.REC.get(c["name"])
    if r is None or hashlib.md5(d.tobytes()).hexdigest() != r["input_md5"] or R._wrapped(c):
        return                       # (a wrapped stream's bytes depend on the zstd / zlib build: compared to the host entry's, made in this process)
    if c["mode"] >= PW_REL:
        R._assert_same_pwr_stream(stream, c, d, r)             # (the sign bytes compared decoded: they too are zstd's)
    else:
        assert len(stream) == r["stream_bytes"] and hashlib.md5(R._mask(stream, r)).hexdigest() == r["stream_md5"], c["name"]


# ------------------------------------------------------------------------------------------------------------------ 1. same bytes as the host entry

def check_compress(dev, c, tmp_path, omp=False, flag=None):
    import sz_amd
    d = data_of(c)
    with Conf(c, tmp_path, omp) as conf:
        want = _host_stream(conf, c)
        if flag is not None:
            assert want[3] & flag == flag, f"{c['name']}: flag byte 0x{want[3]:02x} of the host entry's stream lacks 0x{flag:02x}: the case no longer takes this form"
        for off in ((0, d.itemsize) if dev else _placements(c, (0, d.itemsize))):
            what = f"{c['name']}, array at +{off}"
            src = P.carve(d.nbytes, off, device=dev).put(d)
            conf.init()
            got = sz_amd.SZ_hip_compress_device(src.ptr, d.shape, d.dtype, *_args(c))
            _same_bytes(got, want, what)
            _unchanged(src, d, what)
    _recorded(c, d, want)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("c", ALL, ids=_ids(ALL))
def test_compress_device_same_bytes_gpu(gpu, c, tmp_path):
    check_compress(True, c, tmp_path)


@pytest.mark.parametrize("c", _shim_params(ALL))
def test_compress_device_same_bytes_shim(shim, c, tmp_path):
    check_compress(False, c, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("c", OMP, ids=_ids(OMP))
def test_compress_device_omp_container_gpu(gpu, c, tmp_path):
    want = check_compress(True, c, tmp_path, omp=True)
    assert want[19] == 0x4f          # the container's mark: the case took the OpenMP path


@pytest.mark.parametrize("c", _shim_params(OMP))
def test_compress_device_omp_container_shim(shim, c, tmp_path):
    want = check_compress(False, c, tmp_path, omp=True)
    assert want[19] == 0x4f


# ------------------------------------------------------------------------------------------------------------------ 2. into a device buffer

def check_into(dev, c, tmp_path, omp=False):
    import sz_amd
    d = data_of(c)
    with Conf(c, tmp_path, omp) as conf:
        want = _host_stream(conf, c)
        n = len(want)
        src = P.carve(d.nbytes, 0, device=dev).put(d)
        every = list(itertools.product((0, 1, 8), (0, 64)))
        for off, extra in (every if dev else _placements(c, every[:1] + every[2:] + every[1:2])):      # (on the shim, of a SHIM_KINDS case: +0, capacity n + 64 -- in place)
            what = f"{c['name']}, buffer at +{off}, capacity {n} + {extra}"
            buf = P.carve(n + extra, off, device=dev)
            conf.init()
            got = sz_amd.SZ_hip_compress_device_into(src.ptr, d.shape, d.dtype, buf.ptr, n + extra, *_args(c))
            assert got == n, f"{what}: length {got}"
            _same_bytes(buf.get(n), want, what)
            buf.check(what)
        if n > 0:
            buf = P.carve(n - 1, 1, device=dev)
            conf.init()
            with pytest.raises(sz_amd.SZError):
                sz_amd.SZ_hip_compress_device_into(src.ptr, d.shape, d.dtype, buf.ptr, n - 1, *_args(c))
            buf.check(f"{c['name']}, capacity {n} - 1")
            buf = P.carve(n, 0, device=dev)                     # ... and the context is still usable
            conf.init()
            assert sz_amd.SZ_hip_compress_device_into(src.ptr, d.shape, d.dtype, buf.ptr, n, *_args(c)) == n
            _same_bytes(buf.get(n), want, f"{c['name']}, the call after the refused one")
        _unchanged(src, d, c["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("c", SPEED, ids=_ids(SPEED))
def test_compress_device_into_gpu(gpu, c, tmp_path):
    check_into(True, c, tmp_path)


@pytest.mark.parametrize("c", _shim_params(SPEED))
def test_compress_device_into_shim(shim, c, tmp_path):
    check_into(False, c, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("c", OMP, ids=_ids(OMP))
def test_compress_device_into_omp_container_gpu(gpu, c, tmp_path):
    check_into(True, c, tmp_path, omp=True)


@pytest.mark.parametrize("c", _shim_params(OMP))
def test_compress_device_into_omp_container_shim(shim, c, tmp_path):
    check_into(False, c, tmp_path, omp=True)


def check_into_refuses_lossless_stage(dev, tmp_path, capfd):
    import sz_amd
    c = ref_cases.BY_NAME["C1-zstd"]
    d = data_of(c)
    with Conf(c, tmp_path) as conf:
        src = P.carve(d.nbytes, 0, device=dev).put(d)
        buf = P.carve(d.nbytes, 0, device=dev)
        conf.init()
        n = ctypes.c_size_t(7)
        rc = sz_amd.lib().SZ_hip_compress_device_into(0, src.ptr, buf.ptr, d.nbytes, ctypes.byref(n), *_args(c), *sz_amd.api._dims5(d.shape))
        assert rc == sz_amd.SZ_NSCS and n.value == 0
        buf.check("refused configuration")
        assert np.all(buf.get() == P.FILL)
    ctypes.CDLL(None).fflush(None)                  # (the library prints through C's stdio)
    assert "szMode = SZ_BEST_SPEED only" in capfd.readouterr().out


@pytest.mark.gpu
def test_compress_device_into_refuses_lossless_stage_gpu(gpu, tmp_path, capfd):
    check_into_refuses_lossless_stage(True, tmp_path, capfd)


def test_compress_device_into_refuses_lossless_stage_shim(shim, tmp_path, capfd):
    check_into_refuses_lossless_stage(False, tmp_path, capfd)


# ------------------------------------------------------------------------------------------------------------------ 3. decode

def _decode_all_ways(dev, stream, want, what):
    """the stream from host memory and from a device region at byte offsets 0 and 3, into a carved output at element offsets 0 and 1"""
    import sz_amd
    esz = want.dtype.itemsize
    sources = [("host", None)] + [(f"device +{so}", P.carve(len(stream), so, device=dev).put(stream)) for so in (0, 3)]
    ways = list(itertools.product(sources, (0, 1)))
    if not dev and want.size > SHIM_FAST:
        ways = [ways[1], ways[4]]    # (the shim, a SHIM_KINDS case: host -> element +1, device +3 -> element +0)
    for (sname, sreg), eo in ways:
        w = f"{what}, stream on {sname}, output at element +{eo}"
        dst = P.carve(want.nbytes, eo * esz, device=dev)
        sz_amd.SZ_Init(None)
        if sreg is None:
            sz_amd.SZ_hip_decompress_device(stream, False, len(stream), dst.ptr, want.shape, want.dtype)
        else:
            sz_amd.SZ_hip_decompress_device(sreg.ptr, True, len(stream), dst.ptr, want.shape, want.dtype)
            sreg.check(w + " (stream)")
            assert sreg.get().tobytes() == bytes(stream), f"{w}: the stream was written"
        dst.check(w)
        _same_bits(dst.get().view(want.dtype), want.reshape(-1), w)


def check_decode(dev, c, tmp_path, omp=False):
    import sz_amd
    d = data_of(c)
    with Conf(c, tmp_path, omp) as conf:
        stream = _host_stream(conf, c)
        want = sz_amd.SZ_decompress(stream, d.shape, d.dtype)
        _decode_all_ways(dev, stream, want, c["name"])
    return stream, want


@pytest.mark.gpu
@pytest.mark.parametrize("c", DECODE, ids=_ids(DECODE))
def test_decompress_device_gpu(gpu, c, tmp_path):
    check_decode(True, c, tmp_path)


@pytest.mark.parametrize("c", _shim_params(DECODE))
def test_decompress_device_shim(shim, c, tmp_path):
    check_decode(False, c, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("c", OMP, ids=_ids(OMP))
def test_decompress_device_omp_container_gpu(gpu, c, tmp_path):
    check_decode(True, c, tmp_path, omp=True)


@pytest.mark.parametrize("c", _shim_params(OMP))
def test_decompress_device_omp_container_shim(shim, c, tmp_path):
    check_decode(False, c, tmp_path, omp=True)


def check_stored(dev, c):
    import sz_amd
    r = R.REC[c["name"]]
    stream = open(os.path.join(R.HERE, "golden", r["stream_file"]), "rb").read()
    assert hashlib.md5(stream).hexdigest() == r["stream_md5"]
    sz_amd.SZ_Init(None)
    want = sz_amd.SZ_decompress(stream, tuple(r["shape"]), np.dtype(r["dtype"]))
    _decode_all_ways(dev, stream, want, c["name"] + " (reference-made stream)")


@pytest.mark.gpu
@pytest.mark.parametrize("c", R.STORED, ids=_ids(R.STORED))
def test_decompress_device_reference_made_stream_gpu(gpu, c):
    check_stored(True, c)


@pytest.mark.parametrize("c", _shim_params(R.STORED))
def test_decompress_device_reference_made_stream_shim(shim, c):
    check_stored(False, c)


# ------------------------------------------------------------------------------------------------------------------ 4. the kernels at their edges

def check_raw(dev, c, tmp_path):
    d = data_of(c)
    check_compress(dev, c, tmp_path, flag=0x10)
    check_into(dev, c, tmp_path)
    stream, want = check_decode(dev, c, tmp_path)
    assert stream[3] == 0x50
    _same_bits(want, d, c["name"] + ": the raw store is lossless")


@pytest.mark.gpu
@pytest.mark.parametrize("c", RAW, ids=_ids(RAW))
def test_raw_store_gpu(gpu, c, tmp_path):
    check_raw(True, c, tmp_path)


@pytest.mark.parametrize("c", RAW, ids=_ids(RAW))
def test_raw_store_shim(shim, c, tmp_path):
    check_raw(False, c, tmp_path)


def check_const(dev, c, tmp_path):
    d = data_of(c)
    want = check_compress(dev, c, tmp_path, flag=0x01)
    assert len(want) == (44 if d.dtype == f32 else 56)
    check_into(dev, c, tmp_path)
    _, dec = check_decode(dev, c, tmp_path)         # (guards all round the n values: exactly n were filled)
    _same_bits(dec, d, c["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("c", CONST, ids=_ids(CONST))
def test_constant_stream_gpu(gpu, c, tmp_path):
    check_const(True, c, tmp_path)


@pytest.mark.parametrize("c", CONST, ids=_ids(CONST))
def test_constant_stream_shim(shim, c, tmp_path):
    check_const(False, c, tmp_path)


def check_clamp_case(dev, name, tmp_path):
    import sz_amd
    c = ref_cases.BY_NAME[name]
    d = data_of(c)
    with Conf(c, tmp_path) as conf:
        stream = _host_stream(conf, c)
        assert stream[3] & 0x04
        want = sz_amd.SZ_decompress(stream, d.shape, d.dtype)
        unclamped = bytearray(stream)
        unclamped[3] &= ~0x04 & 0xff
        dst = P.carve(d.nbytes, 0, device=dev)
        sz_amd.SZ_Init(None)
        sz_amd.SZ_hip_decompress_device(bytes(unclamped), False, len(stream), dst.ptr, d.shape, d.dtype)
        loose = dst.get().view(d.dtype)
        assert np.count_nonzero(P.bits(loose) != P.bits(want)) >= 1, f"{name}: the clamp changes nothing in this case any more"
        _decode_all_ways(dev, stream, want, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLAMP)
def test_clamp_on_device_gpu(gpu, name, tmp_path):
    check_clamp_case(True, name, tmp_path)


@pytest.mark.parametrize("name", CLAMP)
def test_clamp_on_device_shim(shim, name, tmp_path):
    check_clamp_case(False, name, tmp_path)


def _values(n, dtype, seed):
    r = np.random.default_rng(seed)
    v = (r.standard_normal(n) * 10).astype(dtype)
    v[r.random(n) < 0.2] = 0
    v[r.random(n) < 0.1] = -0.0
    if n > 2:
        v[n // 2] = np.nan
        v[n - 1] = np.inf
    return v


def check_kernel_entries(dev, ctx, dtype):
    esz = np.dtype(dtype).itemsize
    be = np.dtype(dtype).newbyteorder(">")
    U = np.uint32 if dtype == f32 else np.uint64
    for n, vo, bo in itertools.product((1, 3, 4, 5, 63, 64, 65, 1025), (0, 4, 8, 12), (0, 1, 7, 8)):
        if vo % esz:
            continue
        what = f"{np.dtype(dtype).name}, n = {n}, values at +{vo}, bytes at +{bo}"
        x = _values(n, dtype, n)
        # store_be: values -> bytes, with and without a replacement for zeros
        for repl in (None, 0.0, 2.5):
            src = P.carve(x.nbytes, vo, device=dev).put(x)
            dst = P.carve(x.nbytes, bo, device=dev)
            ctx.store_be(src.ptr, n, dtype, dst.ptr, True, repl)
            y = x.copy()
            if repl is not None:
                y[x == 0] = repl
            assert dst.get().tobytes() == y.astype(be).tobytes(), f"store_be {what}, replacement {repl}"
            dst.check("store_be " + what)
            _unchanged(src, x, "store_be " + what)
        # load_be: bytes -> values
        raw = x.astype(be).tobytes()
        src = P.carve(len(raw), bo, device=dev).put(raw)
        dst = P.carve(x.nbytes, vo, device=dev)
        ctx.load_be(src.ptr, True, n, dtype, dst.ptr)
        assert np.array_equal(dst.get().view(U), x.view(U)), "load_be " + what
        dst.check("load_be " + what)
        src.check("load_be (stream) " + what)
        assert src.get().tobytes() == raw
        if bo == 0:
            # from a host stream too
            host = np.frombuffer(raw, dtype=np.uint8).copy()
            dst = P.carve(x.nbytes, vo, device=dev)
            ctx.load_be(host.ctypes.data, False, n, dtype, dst.ptr)
            assert np.array_equal(dst.get().view(U), x.view(U)), "load_be from the host " + what
            dst.check("load_be from the host " + what)
            # store_be into host memory
            src = P.carve(x.nbytes, vo, device=dev).put(x)
            out = np.full(x.nbytes + 32, P.FILL, dtype=np.uint8)
            ctx.store_be(src.ptr, n, dtype, out.ctypes.data + 16, False)
            assert out[16:16 + x.nbytes].tobytes() == raw and np.all(out[:16] == P.FILL) and np.all(out[16 + x.nbytes:] == P.FILL), "store_be to the host " + what
            # fill
            dst = P.carve(x.nbytes, vo, device=dev)
            ctx.fill(-2.5, n, dtype, dst.ptr)
            assert np.array_equal(dst.get().view(dtype), np.full(n, -2.5, dtype)), "fill " + what
            dst.check("fill " + what)
            # clamp: np.clip passes a NaN through, as the reference's comparisons do
            buf = P.carve(x.nbytes, vo, device=dev).put(x)
            ctx.clamp(buf.ptr, n, dtype, -3.0, 4.5)
            want = np.clip(x, dtype(-3.0), dtype(4.5))
            want[(x >= -3.0) & (x <= 4.5)] = x[(x >= -3.0) & (x <= 4.5)]      # (values inside stay bit for bit: -0.0 stays -0.0)
            assert np.array_equal(buf.get().view(U), want.view(U)), "clamp " + what
            buf.check("clamp " + what)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [f32, f64], ids=["f32", "f64"])
def test_kernel_entries_gpu(built, dtype):
    import sz_amd
    ctx = sz_amd.HipContext(0)
    try:
        check_kernel_entries(True, ctx, dtype)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [f32, f64], ids=["f32", "f64"])
def test_kernel_entries_shim(shim, dtype):
    import sz_amd
    ctx = sz_amd.HipContext(0)
    try:
        check_kernel_entries(False, ctx, dtype)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 5. the MSST19 raw copy
# The raw copy overwrites the flag byte with 0x50 in every form (sz_float.c:538, sz_float_pwr.c:1973), so no stream carries 0x10 | 0x08 and the flag cannot tell
# that the table-driven form's raw copy ran.  What can: the reference's MSST19 wrappers store the array whose zeros they have overwritten (sz_float_pwr.c:2053-2058),
# so the payload differs from the big-endian array exactly where the array is zero.

MSST_RAW = [ref_cases.BY_NAME["pwr-raw-zeros-2D-f32"], case("msst19-raw-zeros-2000-f32", _zeros_2000, mode=PW_REL, pwr=1e-5)]


def check_msst_raw(dev, c, tmp_path):
    d = data_of(c)
    want = check_compress(dev, c, tmp_path, flag=0x10)
    assert want[3] == 0x50 and len(want) == 40 + d.nbytes
    stored = np.frombuffer(want[40:], dtype=">f4").astype(f32).reshape(d.shape)
    zeros = d == 0
    assert zeros.any() and np.all(stored[zeros] > 0) and np.unique(stored[zeros]).size == 1, "the zeros are stored as one positive value"
    assert np.array_equal(P.bits(stored[~zeros]), P.bits(d[~zeros]))
    check_into(dev, c, tmp_path)
    check_decode(dev, c, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("c", MSST_RAW, ids=_ids(MSST_RAW))
def test_msst19_raw_copy_replaces_zeros_gpu(gpu, c, tmp_path):
    check_msst_raw(True, c, tmp_path)


@pytest.mark.parametrize("c", MSST_RAW, ids=_ids(MSST_RAW))
def test_msst19_raw_copy_replaces_zeros_shim(shim, c, tmp_path):
    check_msst_raw(False, c, tmp_path)
