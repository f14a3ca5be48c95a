"""Every device entry point at pointers and capacities no allocator gives (include/szhip.h, "Device pointers and ordering").

The host code picks kernels and copy paths by the low four bits of the caller's pointers and by the capacity of a caller's stream buffer: k_beam or k_pencil
(beam_applies, szhip_rt.inc), k_col_unpack or k_permute<1> + k_unpred<1> on the way back, the fit pass from LDS tiles, three forms of the OpenMP container's
sweep, a stream written in place or through the context's buffer and a copy (szhip_sz21.inc), the Huffman decoders' lead-in in front of a payload that starts at
any byte.  Here the arrays, streams and stream buffers are regions carved out of larger allocations at chosen byte offsets (tests/ptr_cases.py), every byte
around them a guard: the stream must be the oracle's byte for byte, the decoded values the oracle decoder's bit for bit, no guard byte written, the input
unchanged, and `stats.quant_kernel` says which kernel the call reached.

GPU (-m gpu): torch uint8 tensors.  CPU: the same host decisions through the HIP-on-CPU shim (tests/sim), on the smallest arrays of each list."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ptr_cases as P  # noqa: E402

f32, f64 = np.float32, np.float64
ERR_ARG = r"\(-2\)"                 # SZHIP_ERR_ARG in the binding's message


# ------------------------------------------------------------------------------------------------------------------ contexts

@pytest.fixture(scope="module")
def gctx(built):
    import sz_amd
    c = sz_amd.HipContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpool(built):
    import sz_amd
    p = sz_amd.HipPool(0, 2)
    yield p
    p.close()


@pytest.fixture
def shim(built):
    import sim_lib
    from sz_amd import api
    old = api._lib
    api._lib = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    yield
    api._lib = old


@pytest.fixture
def sctx(shim):
    import sz_amd
    c = sz_amd.HipContext(0)
    yield c
    c.close()


@pytest.fixture
def spool(shim):
    import sz_amd
    p = sz_amd.HipPool(0, 1)          # (the shim runs one workgroup at a time on the calling thread: one lane)
    yield p
    p.close()


# ------------------------------------------------------------------------------------------------------------------ checks

def _same_bytes(got, want, what):
    got, want = np.frombuffer(bytes(got), dtype=np.uint8), np.frombuffer(bytes(want), dtype=np.uint8)
    assert got.size == want.size, f"{what}: {got.size} bytes, the oracle's stream has {want.size}"
    d = np.nonzero(got != want)[0]
    assert d.size == 0, f"{what}: {d.size} bytes differ from the oracle's, the first at {int(d[0])} (0x{int(got[d[0]]):02x}, want 0x{int(want[d[0]]):02x})"


def _same_values(region, c, what):
    got = region.get().view(c["x"].dtype)
    d = np.nonzero(P.bits(got) != P.bits(c["dec"]))[0]
    assert d.size == 0, f"{what}: {d.size} decoded values differ from the oracle decoder's, the first at {int(d[0])}"


def _unchanged(src, x, what):
    src.check(what + " (input)")
    assert np.array_equal(src.get(), x.reshape(-1).view(np.uint8)), f"{what}: the input array was written"


def _source(dev, c, off):
    return P.carve(c["x"].nbytes, off, device=dev).put(c["x"])


def _stream(dev, ref, off):
    return P.carve(len(ref), off, device=dev).put(ref)


def _compress(ctx, src, c, **kw):
    x = c["x"]
    return ctx.compress(src.ptr, True, P.shape3(x), x.dtype, c["eb"], c["ref"][:P.meta_len(x)], **kw)


def _decompress(ctx, strm, dst, c, fn="decompress", body=None):
    x = c["x"]
    return getattr(ctx, fn)(strm.ptr, True, len(c["ref"]), P.meta_len(x) + 8 if body is None else body, P.shape3(x), x.dtype, dst.ptr, True)


# ---- 1. input pointer offsets, SZ 2.1 compress
def _in_offsets(name):
    return (0, 8) if name.endswith("f64") else (0, 4, 8, 12)


def check_compress(ctx, dev, oracle, name, off):
    c = P.reference(oracle, name)
    src = _source(dev, c, off)
    got, n, st = _compress(ctx, src, c)
    what = f"{name}, input at +{off}"
    print(f"PATH 1 compress {what}: quant_kernel {int(st.quant_kernel)}")
    _same_bytes(got, c["ref"], what)
    assert int(st.quant_kernel) == P.expected_sweep(c["x"], src.ptr), f"{what}: quant_kernel {int(st.quant_kernel)}"
    _unchanged(src, c["x"], what)


C1 = [(n, o) for n in P.SZ21 for o in _in_offsets(n)]
C1_SHIM = [(n, o) for n in ("s14x20x36", "s14x19x33") for o in _in_offsets(n)]
C1_TILE = [(n, o) for n in ("s24x40x56", "m40") for o in _in_offsets(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,off", C1, ids=[f"{n}-in{o}" for n, o in C1])
def test_compress_input_offsets_on_the_gpu(gctx, oracle, name, off):
    check_compress(gctx, True, oracle, name, off)


@pytest.mark.gpu
@pytest.mark.parametrize("name,off", C1_TILE, ids=[f"{n}-in{o}" for n, o in C1_TILE])
def test_compress_input_offsets_with_the_fit_pass_from_tiles_on_the_gpu(gctx, oracle, monkeypatch, name, off):
    monkeypatch.setenv("SZ_HIP_FIT_TILE", "1")
    check_compress(gctx, True, oracle, name, off)


@pytest.mark.parametrize("name,off", C1_SHIM, ids=[f"{n}-in{o}" for n, o in C1_SHIM])
def test_compress_input_offsets_on_the_cpu_shim(sctx, oracle, name, off):
    check_compress(sctx, False, oracle, name, off)


@pytest.mark.parametrize("off", (0, 4, 8, 12))
def test_compress_input_offsets_with_the_fit_pass_from_tiles_on_the_cpu_shim(sctx, oracle, monkeypatch, off):
    monkeypatch.setenv("SZ_HIP_FIT_TILE", "1")
    check_compress(sctx, False, oracle, "s24x40x56", off)


# ---- 2. output pointer and stream pointer offsets, SZ 2.1 decompress
STREAM_OFFS = (0, 1, 3, 8, 15)


def _dec_pairs(name):
    """(stream offset, output offset): the diagonal of the two lists and the two extremes"""
    outs = _in_offsets(name)
    pairs = list(zip(STREAM_OFFS, itertools.cycle(outs))) + [(STREAM_OFFS[0], outs[-1]), (STREAM_OFFS[-1], outs[0])]
    return list(dict.fromkeys(pairs))


def check_decompress(ctx, dev, oracle, name, s_off, o_off):
    c = P.reference(oracle, name)
    strm, dst = _stream(dev, c["ref"], s_off), P.carve(c["x"].nbytes, o_off, device=dev)
    st = _decompress(ctx, strm, dst, c)
    what = f"{name}, stream at +{s_off}, output at +{o_off}"
    print(f"PATH 2 decompress {what}: quant_kernel {int(st.quant_kernel)}")
    _same_values(dst, c, what)
    dst.check(what + " (output)")
    assert int(st.quant_kernel) == P.expected_sweep(c["x"], dst.ptr), f"{what}: quant_kernel {int(st.quant_kernel)}"
    strm.check(what + " (stream)")
    _same_bytes(strm.get(), c["ref"], what + ": the stream after the call")


C2 = [(n, s, o) for n in P.SZ21 for s, o in _dec_pairs(n)]
C2_SHIM = [(n, s, o) for n in ("s14x20x36", "s14x19x33") for s, o in _dec_pairs(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,s_off,o_off", C2, ids=[f"{n}-stream{s}-out{o}" for n, s, o in C2])
def test_decompress_stream_and_output_offsets_on_the_gpu(gctx, oracle, name, s_off, o_off):
    check_decompress(gctx, True, oracle, name, s_off, o_off)


@pytest.mark.parametrize("name,s_off,o_off", C2_SHIM, ids=[f"{n}-stream{s}-out{o}" for n, s, o in C2_SHIM])
def test_decompress_stream_and_output_offsets_on_the_cpu_shim(sctx, oracle, name, s_off, o_off):
    check_decompress(sctx, False, oracle, name, s_off, o_off)


# ---- 3. the caller's device buffer
BASES = (0, 1, 8, 16)
CAPS = ("len", "len+1", "len+63", "len+64", "len+4096")
SHORT = ("len-1", "0")
# with the code book built on the device the in-place threshold is the header without the tree + 18424 + 64, whatever the stream's length: 2 x len stays below
# it for this array, len + 32768 is above it
CAPS_BOOK = CAPS + ("2len", "len+32768")


def _cap(spec, L):
    return {"len": L, "len+1": L + 1, "len+63": L + 63, "len+64": L + 64, "len+4096": L + 4096, "2len": 2 * L, "len+32768": L + 32768, "len-1": L - 1, "0": 0}[spec]


def _into(via, h, src, c, dst, cap):
    """one compress call into the caller's buffer (dst.ptr, cap) through a context or a pool; returns (size, stats)"""
    x = c["x"]
    if via == "pool":
        return h.wait(h.submit(src.ptr, True, P.shape3(x), x.dtype, c["eb"], c["ref"][:P.meta_len(x)], None, dst.ptr, cap))
    p, n, st = _compress(h, src, c, out_ptr=dst.ptr, out_cap=cap)
    assert p == dst.ptr
    return n, st


def check_caller_buffer(via, h, dev, oracle, name, base, spec):
    c = P.reference(oracle, name)
    L = len(c["ref"])
    cap = _cap(spec, L)
    src, dst = _source(dev, c, 0), P.carve(cap, base, device=dev)
    n, st = _into(via, h, src, c, dst, cap)
    what = f"{name} through a {via}, buffer at +{base}, capacity {spec} = {cap}, book_on_device {int(st.book_on_device)}"
    got = dst.get()
    assert n == L, f"{what}: size {n}, the oracle's stream has {L}"
    _same_bytes(got[:L], c["ref"], what)
    tail = got[L:]
    bad = np.nonzero((tail != P.FILL) & (tail != 0))[0]
    assert bad.size == 0, f"{what}: byte {L + int(bad[0]) if bad.size else 0} behind the stream holds neither the fill byte nor zero"
    dst.check(what)
    _unchanged(src, c["x"], what)
    return st


def check_short_buffer(via, h, dev, oracle, name, base, spec):
    import sz_amd
    c = P.reference(oracle, name)
    L = len(c["ref"])
    cap = _cap(spec, L)
    src, dst = _source(dev, c, 0), P.carve(cap, base, device=dev)
    what = f"{name} through a {via}, buffer at +{base}, capacity {spec} = {cap}"
    with pytest.raises(sz_amd.SZError, match=ERR_ARG):
        _into(via, h, src, c, dst, cap)
    dst.check(what)
    _unchanged(src, c["x"], what)
    # the same context (every lane of the pool) afterwards: the oracle's stream
    good = [P.carve(L + 64, base, device=dev) for _ in range(2)]
    if via == "pool":
        x = c["x"]
        tks = [h.submit(src.ptr, True, P.shape3(x), x.dtype, c["eb"], c["ref"][:P.meta_len(x)], None, g.ptr, L + 64) for g in good]
        sizes = [h.wait(t)[0] for t in tks]
    else:
        sizes = [_into(via, h, src, c, g, L + 64)[0] for g in good]
    for g, n in zip(good, sizes):
        assert n == L
        _same_bytes(g.get(L), c["ref"], what + ": the next call")
        g.check(what + ": the next call")


C3 = [(v, n, b, s) for v in ("context", "pool") for n in ("s24x40x56", "m40") for b in BASES for s in CAPS]
C3_SHORT = [(v, n, b, s) for v in ("context", "pool") for n in ("s24x40x56", "m40") for b in BASES for s in SHORT]
C3_BOOK = [(v, b, s) for v in ("context", "pool") for b in BASES for s in CAPS_BOOK]
C3_SHIM = [(v, b, s) for v in ("context", "pool") for b in BASES for s in CAPS]
C3_SHIM_SHORT = [(v, b, s) for v in ("context", "pool") for b in BASES for s in SHORT]
_id3 = lambda t: "-".join(f"base{p}" if isinstance(p, int) else p for p in t)  # noqa: E731


@pytest.mark.gpu
@pytest.mark.parametrize("via,name,base,spec", C3, ids=[_id3(t) for t in C3])
def test_stream_into_the_callers_buffer_on_the_gpu(gctx, gpool, oracle, monkeypatch, via, name, base, spec):
    monkeypatch.delenv("SZ_HIP_DEV_BOOK", raising=False)
    check_caller_buffer(via, gpool if via == "pool" else gctx, True, oracle, name, base, spec)


@pytest.mark.gpu
@pytest.mark.parametrize("via,name,base,spec", C3_SHORT, ids=[_id3(t) for t in C3_SHORT])
def test_a_buffer_below_the_streams_length_is_refused_on_the_gpu(gctx, gpool, oracle, monkeypatch, via, name, base, spec):
    monkeypatch.delenv("SZ_HIP_DEV_BOOK", raising=False)
    check_short_buffer(via, gpool if via == "pool" else gctx, True, oracle, name, base, spec)


@pytest.mark.gpu
@pytest.mark.parametrize("via,base,spec", C3_BOOK, ids=[_id3(t) for t in C3_BOOK])
def test_stream_into_the_callers_buffer_with_the_device_book_on_the_gpu(gctx, gpool, oracle, monkeypatch, via, base, spec):
    monkeypatch.setenv("SZ_HIP_DEV_BOOK", "1")
    check_caller_buffer(via, gpool if via == "pool" else gctx, True, oracle, "sixty", base, spec)


@pytest.mark.gpu
@pytest.mark.parametrize("via,base,spec", C3_SHIM_SHORT, ids=[_id3(t) for t in C3_SHIM_SHORT])
def test_a_buffer_below_the_streams_length_is_refused_with_the_device_book_on_the_gpu(gctx, gpool, oracle, monkeypatch, via, base, spec):
    monkeypatch.setenv("SZ_HIP_DEV_BOOK", "1")
    check_short_buffer(via, gpool if via == "pool" else gctx, True, oracle, "sixty", base, spec)


@pytest.mark.parametrize("via,base,spec", C3_SHIM, ids=[_id3(t) for t in C3_SHIM])
def test_stream_into_the_callers_buffer_on_the_cpu_shim(sctx, spool, oracle, monkeypatch, via, base, spec):
    monkeypatch.delenv("SZ_HIP_DEV_BOOK", raising=False)
    check_caller_buffer(via, spool if via == "pool" else sctx, False, oracle, "s14x20x36", base, spec)


@pytest.mark.parametrize("via,base,spec", C3_SHIM_SHORT, ids=[_id3(t) for t in C3_SHIM_SHORT])
def test_a_buffer_below_the_streams_length_is_refused_on_the_cpu_shim(sctx, spool, oracle, monkeypatch, via, base, spec):
    monkeypatch.delenv("SZ_HIP_DEV_BOOK", raising=False)
    check_short_buffer(via, spool if via == "pool" else sctx, False, oracle, "s14x20x36", base, spec)


@pytest.mark.parametrize("via,base,spec", C3_BOOK, ids=[_id3(t) for t in C3_BOOK])
def test_stream_into_the_callers_buffer_with_the_device_book_on_the_cpu_shim(sctx, spool, oracle, monkeypatch, via, base, spec):
    monkeypatch.setenv("SZ_HIP_DEV_BOOK", "1")
    check_caller_buffer(via, spool if via == "pool" else sctx, False, oracle, "sixty", base, spec)


@pytest.mark.parametrize("via,base,spec", C3_SHIM_SHORT, ids=[_id3(t) for t in C3_SHIM_SHORT])
def test_a_buffer_below_the_streams_length_is_refused_with_the_device_book_on_the_cpu_shim(sctx, spool, oracle, monkeypatch, via, base, spec):
    monkeypatch.setenv("SZ_HIP_DEV_BOOK", "1")
    check_short_buffer(via, spool if via == "pool" else sctx, False, oracle, "sixty", base, spec)


# ---- 4. one context, roles alternating: the workspaces (stream_buf, codes_nat / codes_blk, the beam's face buffers) allocated by one branch, reused by the other
# (array, "c" input offset -> where the stream goes | "d" stream offset, output offset)
SEQUENCE = [("A", "c", 0, None),                 # aligned input (k_beam), stream to the host
            ("A", "c", 4, (0, "len+64")),        # offset input (k_pencil), the caller's buffer written in place
            ("A", "d", 3, 0),                    # k_beam + k_col_unpack
            ("A", "d", 0, 4),                    # k_pencil + k_permute<1>
            ("B", "c", 8, (1, "len")),           # float64, offset input, the caller's buffer through the context's and a copy
            ("B", "d", 15, 0),
            ("C", "c", 0, (16, "len+63")),       # regression blocks, aligned buffer one byte short of in place
            ("C", "d", 1, 12)]


def check_sequence(ctx, dev, oracle, arrays):
    for step, (which, kind, a, b) in enumerate(SEQUENCE):
        name = arrays[which]
        c = P.reference(oracle, name)
        L = len(c["ref"])
        what = f"call {step + 1} of the sequence ({name}, {kind}, {a}, {b})"
        if kind == "c":
            src = _source(dev, c, a)
            if b is None:
                got, n, st = _compress(ctx, src, c)
            else:
                dst = P.carve(_cap(b[1], L), b[0], device=dev)
                n, st = _into("context", ctx, src, c, dst, dst.nbytes)
                got = dst.get(min(n, dst.nbytes))
                dst.check(what)
            _same_bytes(got, c["ref"], what)
            assert int(st.quant_kernel) == P.expected_sweep(c["x"], src.ptr), what
            _unchanged(src, c["x"], what)
        else:
            strm, dst = _stream(dev, c["ref"], a), P.carve(c["x"].nbytes, b, device=dev)
            st = _decompress(ctx, strm, dst, c)
            _same_values(dst, c, what)
            dst.check(what)
            strm.check(what)
            assert int(st.quant_kernel) == P.expected_sweep(c["x"], dst.ptr), what


@pytest.mark.gpu
def test_one_context_with_alternating_roles_on_the_gpu(built, oracle):
    import sz_amd
    ctx = sz_amd.HipContext(0)        # (a fresh one: its first allocations are this sequence's)
    try:
        check_sequence(ctx, True, oracle, {"A": "s24x40x56", "B": "s20x24x40-f64", "C": "m40"})
    finally:
        ctx.close()


def test_one_context_with_alternating_roles_on_the_cpu_shim(sctx, oracle):
    check_sequence(sctx, False, oracle, {"A": "s14x20x36", "B": "s20x24x40-f64", "C": "m40"})


# ---- 5. the OpenMP container
def _expected_omp(name, ptr):
    """stats.quant_kernel of the container's sweep (szhip_omp.inc): 3 k_omp_col (32 x 32 box faces), 4 k_omp_box with 16-byte row reads, 5 value by value"""
    if ptr % 16:
        return 5
    return {"omp-s64-t8": 3, "omp-s8x8x18-t4": 5, "omp-s16x24x40-t16": 4}[name]


def check_omp_compress(ctx, dev, oracle, name, off):
    c = P.reference(oracle, name, "omp")
    x = c["x"]
    src = _source(dev, c, off)
    got, n, st = ctx.compress_omp(src.ptr, True, x.shape, x.dtype, c["eb"], P.OMP[name], P.OMP_META)
    what = f"{name}, input at +{off}"
    print(f"PATH 5 compress {what}: quant_kernel {int(st.quant_kernel)}")
    _same_bytes(got, c["ref"], what)
    assert int(st.quant_kernel) == _expected_omp(name, src.ptr), f"{what}: quant_kernel {int(st.quant_kernel)}"
    _unchanged(src, x, what)


def check_omp_decompress(ctx, dev, oracle, name, s_off, o_off):
    c = P.reference(oracle, name, "omp")
    strm, dst = _stream(dev, c["ref"], s_off), P.carve(c["x"].nbytes, o_off, device=dev)
    st = _decompress(ctx, strm, dst, c, "decompress_omp", len(P.OMP_META))
    what = f"{name}, stream at +{s_off}, output at +{o_off}"
    print(f"PATH 5 decompress {what}: quant_kernel {int(st.quant_kernel)}")
    _same_values(dst, c, what)
    dst.check(what + " (output)")
    assert int(st.quant_kernel) == _expected_omp(name, dst.ptr), f"{what}: quant_kernel {int(st.quant_kernel)}"
    strm.check(what + " (stream)")
    _same_bytes(strm.get(), c["ref"], what + ": the stream after the call")


C5 = [(n, o) for n in P.OMP for o in (0, 4, 8)]
C5D = [(n, s, o) for n in P.OMP for s in (0, 1, 3, 15) for o in (0, 4)]
C5_SHIM = [t for t in C5 if t[0] != "omp-s64-t8"] + [("omp-s64-t8", 0), ("omp-s64-t8", 4)]
C5D_SHIM = [t for t in C5D if t[0] != "omp-s64-t8"] + [("omp-s64-t8", 0, 0), ("omp-s64-t8", 15, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,off", C5, ids=[f"{n}-in{o}" for n, o in C5])
def test_omp_container_input_offsets_on_the_gpu(gctx, oracle, name, off):
    check_omp_compress(gctx, True, oracle, name, off)


@pytest.mark.gpu
@pytest.mark.parametrize("name,s_off,o_off", C5D, ids=[f"{n}-stream{s}-out{o}" for n, s, o in C5D])
def test_omp_container_stream_and_output_offsets_on_the_gpu(gctx, oracle, name, s_off, o_off):
    check_omp_decompress(gctx, True, oracle, name, s_off, o_off)


@pytest.mark.parametrize("name,off", C5_SHIM, ids=[f"{n}-in{o}" for n, o in C5_SHIM])
def test_omp_container_input_offsets_on_the_cpu_shim(sctx, oracle, name, off):
    check_omp_compress(sctx, False, oracle, name, off)


@pytest.mark.parametrize("name,s_off,o_off", C5D_SHIM, ids=[f"{n}-stream{s}-out{o}" for n, s, o in C5D_SHIM])
def test_omp_container_stream_and_output_offsets_on_the_cpu_shim(sctx, oracle, name, s_off, o_off):
    check_omp_decompress(sctx, False, oracle, name, s_off, o_off)


# ---- 6. SZ 1.4 (3-D, 2-D, 1-D) through the device-pointer bindings
def check_sz14_compress(ctx, dev, oracle, name, in_off, s_off):
    import sz_amd
    c = P.reference(oracle, name, "sz14")
    x, L = c["x"], len(c["ref"])
    src, dst = _source(dev, c, in_off), P.carve(L, s_off, device=dev)
    rng, med = sz_amd.api.sz14_range(x.min(), x.max(), x.dtype)
    p, n, st = ctx.compress_sz14(src.ptr, True, P.shape3(x), x.dtype, c["eb"], rng, med, c["ref"][:P.meta_len(x)], out_ptr=dst.ptr, out_cap=L)
    what = f"SZ 1.4 {name}, input at +{in_off}, the caller's buffer at +{s_off} with the stream's exact length"
    assert p == dst.ptr and n == L, (what, n, L)
    _same_bytes(dst.get(), c["ref"], what)
    dst.check(what)
    _unchanged(src, x, what)


def check_sz14_decompress(ctx, dev, oracle, name, s_off, o_off):
    c = P.reference(oracle, name, "sz14")
    strm, dst = _stream(dev, c["ref"], s_off), P.carve(c["x"].nbytes, o_off, device=dev)
    _decompress(ctx, strm, dst, c, "decompress_sz14")
    what = f"SZ 1.4 {name}, stream at +{s_off}, output at +{o_off}"
    _same_values(dst, c, what)
    dst.check(what + " (output)")
    strm.check(what + " (stream)")
    _same_bytes(strm.get(), c["ref"], what + ": the stream after the call")


C6 = [(n, a, b) for n in P.SZ14 for a in (0, 4) for b in (0, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,in_off,s_off", C6, ids=[f"{n}-in{a}-stream{b}" for n, a, b in C6])
def test_sz14_compress_offsets_on_the_gpu(gctx, oracle, name, in_off, s_off):
    check_sz14_compress(gctx, True, oracle, name, in_off, s_off)


@pytest.mark.gpu
@pytest.mark.parametrize("name,o_off,s_off", C6, ids=[f"{n}-out{a}-stream{b}" for n, a, b in C6])
def test_sz14_decompress_offsets_on_the_gpu(gctx, oracle, name, o_off, s_off):
    check_sz14_decompress(gctx, True, oracle, name, s_off, o_off)


def test_sz14_bindings_on_the_cpu_shim(sctx, oracle):
    for name in ("plane70x90", "series4097"):
        check_sz14_compress(sctx, False, oracle, name, 4, 3)
        check_sz14_decompress(sctx, False, oracle, name, 3, 4)


def test_sz14_range_is_computed_in_the_datas_type():
    from sz_amd import api
    lo, hi = f32(0.1), f32(0.7)
    rng, med = api.sz14_range(lo, hi, f32)
    assert rng == float(f32(hi - lo)) and med == float(f32(lo + f32(f32(hi - lo) / f32(2))))
    assert api.sz14_range(0.1, 0.7, f64) == (0.7 - 0.1, 0.1 + (0.7 - 0.1) / 2)
    assert rng != 0.7 - 0.1


# ---- 7. szhip_minmax
MINMAX_N = (1, 3, 4, 5, 63, 64, 65, 257, 4099)


def check_minmax(ctx, dev, dtype, n, off):
    x = np.random.default_rng(n).uniform(-1, 1, n).astype(dtype)
    for first, last in ((-3.5, 7.25), (7.25, -3.5)):          # the extremes at the first and at the last element, both ways round
        x[0] = first
        x[-1] = last
        src = P.carve(x.nbytes, off, device=dev).put(x)
        lo, hi = ctx.minmax(src.ptr, True, n, dtype)
        what = f"minmax of {n} {np.dtype(dtype).name} values at +{off}"
        assert (lo, hi) == (float(x.min()), float(x.max())), (what, lo, hi)
        _unchanged(src, x, what)


C7 = [(dt, n, o) for dt in (f32, f64) for n in MINMAX_N for o in ((0, 4, 8, 12) if dt is f32 else (0, 8))]
_id7 = [f"{np.dtype(dt).name}-n{n}-in{o}" for dt, n, o in C7]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n,off", C7, ids=_id7)
def test_minmax_offsets_on_the_gpu(gctx, dtype, n, off):
    check_minmax(gctx, True, dtype, n, off)


@pytest.mark.parametrize("dtype,n,off", C7, ids=_id7)
def test_minmax_offsets_on_the_cpu_shim(sctx, dtype, n, off):
    check_minmax(sctx, False, dtype, n, off)


# ---- 8. element alignment: a pointer to values that is not aligned to its element is SZHIP_ERR_ARG before anything is launched
ENTRIES = ("minmax", "compress", "decompress", "compress_omp", "decompress_omp", "compress_sz14", "decompress_sz14")


def check_misaligned(ctx, dev, oracle, entry, dtype):
    import sz_amd
    name, kind = {"compress_omp": ("omp-s8x8x18-t4", "omp"), "decompress_omp": ("omp-s8x8x18-t4", "omp"), "compress_sz14": ("plane70x90", "sz14"),
                  "decompress_sz14": ("plane70x90", "sz14")}.get(entry, ("s14x19x33", "sz21"))
    c = P.reference(oracle, name, kind)
    x, ref = c["x"].astype(dtype), c["ref"]
    es = x.dtype.itemsize
    for off in sorted({1, 2, es // 2, es - 1}):
        # the array sits at an aligned address; the pointer handed over is `off` bytes behind it: a call that ran would read behind the array or write
        # behind the output
        reg = P.carve(x.nbytes, 0, device=dev).put(x)
        strm = _stream(dev, ref, 3)
        ptr = reg.ptr + off
        what = f"{entry}, {x.dtype.name} pointer at +{off}"
        with pytest.raises(sz_amd.SZError, match=ERR_ARG):
            if entry == "minmax":
                ctx.minmax(ptr, True, x.size, x.dtype)
            elif entry == "compress":
                ctx.compress(ptr, True, P.shape3(x), x.dtype, c["eb"], ref[:P.meta_len(x)])
            elif entry == "compress_omp":
                ctx.compress_omp(ptr, True, x.shape, x.dtype, c["eb"], P.OMP[name], P.OMP_META)
            elif entry == "compress_sz14":
                ctx.compress_sz14(ptr, True, P.shape3(x), x.dtype, c["eb"], 1.0, 0.5, ref[:P.meta_len(x)])
            elif entry == "decompress_omp":
                ctx.decompress_omp(strm.ptr, True, len(ref), len(P.OMP_META), x.shape, x.dtype, ptr, True)
            else:
                getattr(ctx, entry)(strm.ptr, True, len(ref), P.meta_len(c["x"]) + 8, P.shape3(x), x.dtype, ptr, True)
        _unchanged(reg, x, what)
        strm.check(what)
    # a byte pointer takes any alignment, and the context is as usable as before: the 8-byte input of szhip_minmax behind a refused call
    reg = P.carve(x.nbytes, 0, device=dev).put(x)
    assert ctx.minmax(reg.ptr, True, x.size, x.dtype) == (float(x.min()), float(x.max()))


C8 = [(e, dt) for e in ENTRIES for dt in (f32, f64)]
_id8 = [f"{e}-{np.dtype(dt).name}" for e, dt in C8]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,dtype", C8, ids=_id8)
def test_misaligned_value_pointers_are_refused_on_the_gpu(gctx, oracle, entry, dtype):
    check_misaligned(gctx, True, oracle, entry, dtype)


@pytest.mark.parametrize("entry,dtype", C8, ids=_id8)
def test_misaligned_value_pointers_are_refused_on_the_cpu_shim(sctx, oracle, entry, dtype):
    check_misaligned(sctx, False, oracle, entry, dtype)


# ---- the helper itself
@pytest.mark.parametrize("off", (0, 1, 4, 15, 16))
def test_the_carved_region_and_its_guards(off):
    r = P.carve(100, off, pad=64)
    assert (r.ptr - off) % 256 == 0
    r.put(np.arange(100, dtype=np.uint8))
    r.check("untouched")
    assert np.array_equal(r.get(4, 10), np.arange(10, 14, dtype=np.uint8))
    for where in (r.start - 1, r.start + 100, r.start - 256, len(r.whole) - 1):      # the bytes next to the region and the allocation's ends
        r.whole[where] = 0
        with pytest.raises(AssertionError, match="guard bytes"):
            r.check("touched")
        r.whole[where] = P.FILL
    r.check("restored")
