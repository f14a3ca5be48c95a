"""Failure returns and call statistics of the SZ 1.4 and OpenMP containers (szhip_compress_sz14 / szhip_decompress_sz14 / szhip_decompress_sz14_pwr,
szhip_compress_omp / szhip_decompress_omp), on the HIP-on-CPU shim only: damaged streams are not fed to a GPU.

Every stream is the oracle's.  It is cut at each field boundary of its header, inside the Huffman tree and one byte short of its end; single header fields
are replaced by values the decoders refuse; a caller's stream buffer is one byte too small or missing.  Each such call returns its error code, leaves a
message in szhip_last_error, and the next valid call on the same context gives the oracle's bytes (compress) or the oracle's decoded bits (decompress).
Streams are handed over as host pointers and as "device" pointers (the shim's device memory is host memory): the latter go through the decoders' prefix fetch.

The point-wise-relative stream is located by szhip_sz14_pwr_locate before the decoder sees it; that function takes no context, so a cut it refuses
leaves no message of its own behind (the assertion on the message is made where a context-carrying function refused).

The statistics a call reports (all fields of szhip_stats that are not timings) are compared with literals recorded from the library before the call
steps of these containers were shared with the SZ 2.1 path; `intervals` and `n_unpred` also with the fields of the oracle's stream header."""
import ctypes
import os

import numpy as np
import pytest

import sim_lib
from sz_amd.fields import plane_field, s_field

ERR_ARG, ERR_STREAM = -2, -4
META = bytes(range(1, 33))
STAT_FIELDS = ("n_elements", "n_blocks", "intervals", "n_unpred", "quant_kernel", "quant_kernel_launches", "out_bytes", "packing", "book_on_device")

# recorded at the parent of the commit that introduced szhip_steps.inc: name -> (after compress, after decompress), fields in STAT_FIELDS order
RECORDED = {
    "s-20x24x40": ((19200, 0, 64, 46, 0, 1, 7785, 0, 0), (19200, 0, 64, 46, 0, 1, 76800, 0, 0)),
    "plane-70x90": ((6300, 0, 128, 7, 0, 1, 3602, 0, 0), (6300, 0, 128, 7, 0, 1, 25200, 0, 0)),
    "series-3000": ((3000, 0, 256, 33, 0, 1, 7408, 0, 0), (3000, 0, 256, 33, 0, 1, 12000, 0, 0)),
    "pwrel-12x20x28": ((6720, 0, 512, 6, 0, 1, 10472, 0, 0), (6720, 0, 512, 6, 0, 1, 26880, 0, 0)),
    "omp-64-t8": ((262144, 8, 32, 2887, 3, 1, 97140, 0, 0), (262144, 8, 32, 2887, 3, 0, 1048576, 0, 0)),
    "omp-40x36x44-t8": ((63360, 8, 32, 1696, 5, 1, 29889, 0, 0), (63360, 8, 32, 1696, 5, 0, 253440, 0, 0)),
}


def _stats(st):
    return tuple(int(getattr(st, k)) for k in STAT_FIELDS)


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _shape3(x):
    return (0,) * (3 - x.ndim) + tuple(x.shape)


def _pw_field():
    """the smoke test's point-wise-relative array: both signs, zeros, a 3-D array"""
    rng = np.random.default_rng(11)
    pw = np.exp(2.0 * s_field(12, 20, 28, np.float64) + 0.05 * rng.standard_normal((12, 20, 28))) * np.sign(s_field(12, 20, 28, np.float64) + 0.2)
    pw[rng.random(pw.shape) < 0.03] = 0.0
    pw.reshape(-1)[0] = 0.5
    return np.ascontiguousarray(pw.astype(np.float32))


_CASES = {}       # name -> dict, computed once, never changed


def _sz14_case(oracle, name):
    if name not in _CASES:
        if name == "pwrel-12x20x28":
            x = _pw_field()
            po = oracle.default_params(); po.pw_rel_bound_ratio = 1e-2; po.accelerate_pw_rel = 1
            ref, _ = oracle.compress(x, oracle.PW_REL, 0.0, 0.0, params=po)
            assert ref[3] & 0x20 and ref[3] & 0x08                 # PW_REL in its table-driven (MSST19) form
            c = dict(x=x, eb=None, ref=ref, pwr=True, segment_size=po.segment_size)
            signs = (x.reshape(-1) < 0).astype(np.uint8); signs[0] = 0          # k_msst_scan: from element 1 on
            c["signs"] = signs
        else:
            x = {"s-20x24x40": lambda: s_field(20, 24, 40), "plane-70x90": lambda: plane_field(70, 90),
                 "series-3000": lambda: np.ascontiguousarray((np.cumsum(np.random.default_rng(7).standard_normal(3000)) * 0.01).astype(np.float32))}[name]()
            ref, _ = oracle.compress(x, oracle.ABS, 1e-4, params=oracle.default_params(with_regression=0))
            assert not ref[3] & 0x80 and not ref[3] & 0x10         # the SZ 1.4 container, not the raw copy
            c = dict(x=x, eb=1e-4, ref=ref, pwr=False)
        c["dec"] = oracle.decompress(ref, x.shape, x.dtype)
        c["body_off"] = 4 + 28 + 8
        # the fields of `fixed` (TightDataPointStorageF.c:54-265), from body_off on
        names = ["max_quant"] + (["rad_expo", "segment_size", "blob_size"] if c["pwr"] else []) + ["intervals", "median", "req_len"]
        sizes = [4] + ([1, 8, 4] if c["pwr"] else []) + [4, 4, 1]
        if c["pwr"]: names += ["plus_bits", "max_bits"]; sizes += [1, 1]
        names += ["eb", "type_size", "E", "nmid"] + (["min_log"] if c["pwr"] else []) + ["node_count", "tree_intervals"]
        sizes += [8, 8, 8, 8] + ([4] if c["pwr"] else []) + [4, 4]
        off, at = {}, c["body_off"]
        for k, s in zip(names, sizes):
            off[k] = (at, s); at += s
        c["off"], c["tree_at"] = off, at
        x.setflags(write=False); c["dec"].setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


OMP_INPUTS = {"omp-64-t8": ((64, 64, 64), 8), "omp-40x36x44-t8": ((40, 36, 44), 8)}     # eight 32^3 boxes (k_omp_col); rows of 22 values (the scalar k_omp_box)


def _omp_case(oracle, name):
    if name not in _CASES:
        shape, threads = OMP_INPUTS[name]
        x = s_field(*shape)
        ref = oracle.omp_compress(x, 1e-4, threads, META)
        b = len(META)
        nb = int.from_bytes(ref[b:b + 4], "big"); tree_bytes = int.from_bytes(ref[b + 12:b + 16], "big")
        fixed = b + 4 + 4 + 12
        off_ucount = fixed + tree_bytes; off_first = off_ucount + nb * 4; off_unpred = off_first + nb * 4
        E = int(np.frombuffer(ref[off_ucount:off_first], dtype="<u4").sum())
        off_sizes = off_unpred + E * 4; off_pay = off_sizes + nb * 8
        c = dict(x=x, eb=1e-4, ref=ref, threads=threads, dec=oracle.omp_decompress(ref, b, x.shape, x.dtype), nb=nb, E=E, fixed=fixed, tree_bytes=tree_bytes,
                 off_ucount=off_ucount, off_first=off_first, off_unpred=off_unpred, off_sizes=off_sizes, off_pay=off_pay)
        assert nb == threads and off_pay < len(ref)
        x.setflags(write=False); c["dec"].setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


@pytest.fixture(scope="module")
def shim(built):
    from sz_amd import api
    saved = api._lib
    L = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    L.szhip_decompress_sz14_pwr.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, sz, sz, sz, sz, sz, vp, vp, ctypes.c_int, ctypes.POINTER(api.szhip_stats)]
    L.szhip_decompress_sz14_pwr.restype = ctypes.c_int
    api._lib = L
    yield L
    api._lib = saved


@pytest.fixture()
def ctx(shim):
    import sz_amd
    c = sz_amd.HipContext(0)
    yield c
    c.close()


def _last_error(L, ctx):
    return L.szhip_last_error(ctx._h).decode(errors="replace")


# ---- SZ 1.4 container
def _dec14(L, ctx, c, stream, on_device):
    """-> (return code, decoded array, statistics)"""
    from sz_amd import api
    x = c["x"]
    buf = ctypes.create_string_buffer(bytes(stream), len(stream))
    out = np.zeros_like(x)
    st = api.szhip_stats()
    if c["pwr"]:
        rc = L.szhip_decompress_sz14_pwr(ctx._h, 0, ctypes.addressof(buf), 0, len(stream), c["body_off"], *_shape3(x), c["signs"].ctypes.data, out.ctypes.data, 0, ctypes.byref(st))
    else:
        rc = L.szhip_decompress_sz14(ctx._h, 0, ctypes.addressof(buf), int(on_device), len(stream), c["body_off"], *_shape3(x), out.ctypes.data, 0, ctypes.byref(st))
    return rc, out, st


def _refused14(L, ctx, c, stream, on_device, what, by_locate=False):
    rc, _, _ = _dec14(L, ctx, c, stream, on_device)
    assert rc == ERR_STREAM, (what, rc)
    if not by_locate:
        assert _last_error(L, ctx), what
    rc, out, _ = _dec14(L, ctx, c, c["ref"], on_device)                       # the next valid call on the same context
    assert rc == 0 and np.array_equal(_bits(out), _bits(c["dec"])), what


SZ14 = ["s-20x24x40", "plane-70x90", "series-3000", "pwrel-12x20x28"]
SZ14_ON_DEVICE = [(n, d) for n in SZ14 for d in (0, 1) if not (d and n.startswith("pwrel"))]     # (szhip_decompress_sz14_pwr reads the header on the host)


@pytest.mark.parametrize("name,on_device", SZ14_ON_DEVICE)
def test_sz14_stream_cut_at_every_header_field(oracle, shim, ctx, name, on_device):
    c = _sz14_case(oracle, name)
    ref = c["ref"]
    cuts = [(k, at + s) for k, (at, s) in c["off"].items()] + [("inside the tree", c["tree_at"] + 3), ("one byte short of the exact-value tables", len(ref) - 1)]
    assert c["tree_at"] + 3 < len(ref) - 1
    for k, cut in cuts:
        # szhip_sz14_pwr_locate refuses a PW_REL stream that ends before its sign bytes do
        _refused14(shim, ctx, c, ref[:cut], on_device, f"{name}: cut behind {k} ({cut} of {len(ref)} bytes)", by_locate=c["pwr"] and cut < len(ref) - 1)


@pytest.mark.parametrize("name,on_device", SZ14_ON_DEVICE)
def test_sz14_header_fields_the_decoder_refuses(oracle, shim, ctx, name, on_device):
    c = _sz14_case(oracle, name)
    n = c["x"].size
    for field, value in (("intervals", 2), ("intervals", 131072), ("req_len", 8), ("node_count", 0), ("E", n + 1)):
        at, s = c["off"][field]
        bad = bytearray(c["ref"]); bad[at:at + s] = int(value).to_bytes(s, "big")
        _refused14(shim, ctx, c, bad, on_device, f"{name}: {field} = {value}")


def _compress14(L, ctx, c, mode, out_ptr, cap):
    from sz_amd import api
    x = c["x"]
    rng, med = api.sz14_range(x.min(), x.max(), x.dtype)
    p = api.szhip_params(100, 0.99, 65536, 0)
    out, n, st = ctypes.c_void_p(out_ptr), ctypes.c_size_t(cap), api.szhip_stats()
    rc = L.szhip_compress_sz14(ctx._h, 0, x.ctypes.data, 0, *_shape3(x), c["eb"], rng, med, ctypes.byref(p), c["ref"][:32], 32, mode, ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
    return rc, out, n.value, st


def _take(L, out, n):
    b = ctypes.string_at(out.value, n); L.free(out); return b


@pytest.mark.parametrize("name", SZ14[:3])
def test_sz14_caller_buffer_too_small_or_missing(oracle, shim, ctx, name):
    c = _sz14_case(oracle, name)
    L = len(c["ref"])
    room = ctypes.create_string_buffer(L + 64)
    for what, ptr, cap in (("capacity len - 1", ctypes.addressof(room), L - 1), ("null *out", None, L)):
        rc, _, _, _ = _compress14(shim, ctx, c, 2, ptr, cap)
        assert rc == ERR_ARG and _last_error(shim, ctx), (name, what, rc)
        rc, out, n, _ = _compress14(shim, ctx, c, 0, None, 0)
        assert rc == 0 and _take(shim, out, n) == c["ref"], (name, what)
    rc, out, n, _ = _compress14(shim, ctx, c, 2, ctypes.addressof(room), L)      # the stream's exact length is enough
    assert rc == 0 and n == L and room.raw[:L] == c["ref"]


def _header_counts14(c):
    return int.from_bytes(c["ref"][slice(*_span(c["off"]["intervals"]))], "big"), int.from_bytes(c["ref"][slice(*_span(c["off"]["E"]))], "big")


def _span(at_size):
    return at_size[0], at_size[0] + at_size[1]


@pytest.mark.parametrize("name", SZ14)
def test_sz14_statistics(oracle, shim, ctx, name):
    import sz_amd
    c = _sz14_case(oracle, name)
    x = c["x"]
    if c["pwr"]:          # the preparation passes and the sign bytes are sz_api.c's: through SZ_compress_args, whose context is the library's own
        assert sz_amd.SZ_Init(os.path.join(sim_lib.ROOT, "tests", "golden", "sz_speed.config")) == 0
        try:
            sz_amd.conf_params().segment_size = c["segment_size"]
            assert sz_amd.SZ_compress_args(x, sz_amd.PW_REL, 0.0, 0.0, 1e-2) == c["ref"]
            st = sz_amd.SZ_hip_last_stats()
        finally:
            sz_amd.SZ_Finalize()
    else:
        rc, out, n, st = _compress14(shim, ctx, c, 0, None, 0)
        assert rc == 0 and _take(shim, out, n) == c["ref"]
    rc, out, sd = _dec14(shim, ctx, c, c["ref"], 0)
    assert rc == 0 and np.array_equal(_bits(out), _bits(c["dec"]))
    intervals, E = _header_counts14(c)
    for s in (st, sd):
        assert (s.intervals, s.n_unpred) == (intervals, E)
    assert (_stats(st), _stats(sd)) == RECORDED[name]


# ---- OpenMP container
def _dec_omp(L, ctx, c, stream, on_device):
    from sz_amd import api
    x = c["x"]
    buf = ctypes.create_string_buffer(bytes(stream), len(stream))
    out = np.zeros_like(x)
    st = api.szhip_stats()
    rc = L.szhip_decompress_omp(ctx._h, 0, ctypes.addressof(buf), int(on_device), len(stream), len(META), *x.shape, out.ctypes.data, 0, ctypes.byref(st))
    return rc, out, st


def _refused_omp(L, ctx, c, stream, on_device, what):
    rc, _, _ = _dec_omp(L, ctx, c, stream, on_device)
    assert rc == ERR_STREAM and _last_error(L, ctx), (what, rc)
    rc, out, _ = _dec_omp(L, ctx, c, c["ref"], on_device)
    assert rc == 0 and np.array_equal(_bits(out), _bits(c["dec"])), what


OMP_ON_DEVICE = [(n, d) for n in OMP_INPUTS for d in (0, 1)]


@pytest.mark.parametrize("name,on_device", OMP_ON_DEVICE)
def test_omp_stream_cut_at_every_header_field(oracle, shim, ctx, name, on_device):
    c = _omp_case(oracle, name)
    ref, b = c["ref"], len(META)
    cuts = [("thread_num", b + 4), ("eb", b + 8), ("intervals", b + 12), ("tree_bytes", b + 16), ("fixed", c["fixed"]), ("inside the tree", c["fixed"] + c["tree_bytes"] // 2),
            ("the tree", c["off_ucount"]), ("the counts of verbatim values", c["off_first"]), ("the first values", c["off_unpred"]), ("the verbatim values", c["off_sizes"]),
            ("the payload sizes", c["off_pay"]), ("one byte short of the last payload", len(ref) - 1)]
    for k, cut in cuts:
        _refused_omp(shim, ctx, c, ref[:cut], on_device, f"{name}: cut behind {k} ({cut} of {len(ref)} bytes)")


@pytest.mark.parametrize("name,on_device", OMP_ON_DEVICE)
def test_omp_header_fields_the_decoder_refuses(oracle, shim, ctx, name, on_device):
    c = _omp_case(oracle, name)
    b = len(META)
    bel = c["x"].size // c["nb"]
    for field, at, value, order in (("intervals", b + 8, 2, "big"), ("intervals", b + 8, 131072, "big"), ("node_count", b + 16, 0, "big"), ("thread_num", b, 7, "big"),
                                    ("count of verbatim values of box 0", c["off_ucount"], bel + 1, "little")):
        bad = bytearray(c["ref"]); bad[at:at + 4] = int(value).to_bytes(4, order)
        _refused_omp(shim, ctx, c, bad, on_device, f"{name}: {field} = {value}")


def _compress_omp(L, ctx, c, mode, out_ptr, cap):
    from sz_amd import api
    x = c["x"]
    p = api.szhip_params(100, 0.99, 65536, 0)
    out, n, st = ctypes.c_void_p(out_ptr), ctypes.c_size_t(cap), api.szhip_stats()
    rc = L.szhip_compress_omp(ctx._h, 0, x.ctypes.data, 0, *x.shape, c["eb"], c["threads"], ctypes.byref(p), META, len(META), mode, ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
    return rc, out, n.value, st


@pytest.mark.parametrize("name", list(OMP_INPUTS))
def test_omp_caller_buffer_too_small_or_missing(oracle, shim, ctx, name):
    c = _omp_case(oracle, name)
    L = len(c["ref"])
    room = ctypes.create_string_buffer(L + 64)
    for what, ptr, cap in (("capacity len - 1", ctypes.addressof(room), L - 1), ("null *out", None, L)):
        rc, _, _, _ = _compress_omp(shim, ctx, c, 2, ptr, cap)
        assert rc == ERR_ARG and _last_error(shim, ctx), (name, what, rc)
        rc, out, n, _ = _compress_omp(shim, ctx, c, 0, None, 0)
        assert rc == 0 and _take(shim, out, n) == c["ref"], (name, what)
    rc, out, n, _ = _compress_omp(shim, ctx, c, 2, ctypes.addressof(room), L)
    assert rc == 0 and n == L and room.raw[:L] == c["ref"]


@pytest.mark.parametrize("name", list(OMP_INPUTS))
def test_omp_statistics(oracle, shim, ctx, name):
    c = _omp_case(oracle, name)
    rc, out, n, st = _compress_omp(shim, ctx, c, 0, None, 0)
    assert rc == 0 and _take(shim, out, n) == c["ref"]
    rc, out, sd = _dec_omp(shim, ctx, c, c["ref"], 0)
    assert rc == 0 and np.array_equal(_bits(out), _bits(c["dec"]))
    intervals = int.from_bytes(c["ref"][len(META) + 8:len(META) + 12], "big")
    for s in (st, sd):
        assert (s.intervals, s.n_unpred) == (intervals, c["E"])
    assert (_stats(st), _stats(sd)) == RECORDED[name]
