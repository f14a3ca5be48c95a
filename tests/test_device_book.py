"""The Huffman code book built on the device (SZ_HIP_DEV_BOOK=1; sz_amd/csrc/szh_book.h: k_huff_book, k_book_tail, k_book_unpred).

The kernel alone, through szhip_huff_book, against the host builder it stands in for (szhost_huff_build + szhost_huff_tree_write): tree bytes, node count, every
code word and length and the bit total must be EQUAL -- the reference's heap decides which of two equal counts becomes the left child, so histograms full of ties
are the point.  Then whole calls with the switch set: the oracle's stream byte for byte, `book_on_device` in the call's statistics saying who built the book.

GPU (-m gpu): everything.  CPU: the same kernels through the HIP-on-CPU shim for the histograms and the small arrays (logic, not the GPU's memory model), the
binding's structure layout against the header, the record's parse and the switch table (tests/test_host_logic.py reads this file for SZ_HIP_TEST_BOOK_FALLBACK)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import longcode_fields as F  # noqa: E402

f32, f64 = np.float32, np.float64
CAP = 1024                      # SZH_BOOK_CAP: distinct symbols the kernel's heap holds


class _Huff(ctypes.Structure):      # sz_amd/csrc/szhost.h
    _fields_ = [("state_num", ctypes.c_int), ("n_nodes", ctypes.c_int), ("code", ctypes.POINTER(ctypes.c_uint64)),
                ("len", ctypes.POINTER(ctypes.c_uint8)), ("L", ctypes.POINTER(ctypes.c_uint32)), ("R", ctypes.POINTER(ctypes.c_uint32)),
                ("C", ctypes.POINTER(ctypes.c_uint32)), ("t", ctypes.POINTER(ctypes.c_uint8)), ("total_bits", ctypes.c_uint64)]


# ------------------------------------------------------------------------------------------------------------------ the histograms

def _spread(intervals, counts, seed=0):
    """counts at symbols spread over the alphabet (sorted places: the heap sees the leaves in symbol order), uint32[intervals]"""
    rng = np.random.default_rng(seed + len(counts))
    h = np.zeros(intervals, dtype=np.uint32)
    h[np.sort(rng.permutation(intervals)[:len(counts)])] = np.asarray(counts, dtype=np.uint32)
    return h


def _longcode_histogram(L):
    """the code histogram of tests/longcode_fields.py's array for a longest code word of L bits: the chain's counts at 64 + value, the rest of the smallest
    cube's places at 64"""
    c, v = F.chain_counts(L), F.chain_values(L)
    h = np.zeros(F.INTERVALS, dtype=np.uint32)
    for cnt, val in zip(c, v):
        h[F.INTERVALS // 2 + val] = cnt
    h[F.INTERVALS // 2] = F.smallest_cube(L) ** 3 - sum(c)
    return h


def _random_histograms():
    out = []
    rng = np.random.default_rng(2024)
    for i in range(20):
        intervals = (32, 256, 1024, 65536)[i % 4]
        used = int(rng.integers(2, min(intervals, CAP) + 1))
        h = np.zeros(intervals, dtype=np.uint32)
        where = rng.permutation(intervals)[:used]
        # a few magnitudes, many repeated counts (ties), bin 0 sometimes in, sometimes out
        h[where] = np.maximum(1, (rng.pareto(1.2, used) * (1 + i)).astype(np.int64)).clip(1, 2 ** 31).astype(np.uint32)
        if i % 3 == 0:
            h[0] = int(rng.integers(1, 50))
        out.append((f"random{i}-{intervals}", h))
    return out


def _histograms():
    H = [("one-symbol", _spread(64, [7])), ("one-symbol-bin0", np.asarray([5, 0, 0, 0], dtype=np.uint32)), ("two-symbols", _spread(64, [3, 9]))]
    H += [(f"equal-{k}", _spread(256, [4] * k)) for k in (8, 31, 32, 33)]
    H += [("equal-in-pairs", _spread(256, [c for c in (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144) for _ in (0, 1)]))]
    H += [("geometric-30", _spread(1024, [max(1, int(134217728 * 0.55 ** abs(i - 15))) for i in range(30)]))]
    H += [(f"nonzero-{k}", _spread(1024, [1 + (i * 7919) % 97 for i in range(k)])) for k in (255, 256, 257)]
    H += [("capacity-1024", _spread(4096, [1 + (i * 31) % 11 for i in range(CAP)]))]
    H += [(f"longcode-{L}", _longcode_histogram(L)) for L in (31, 32)]
    return H + _random_histograms()


HISTS = _histograms()
DECLINED = [("beyond-capacity-1025", _spread(4096, [1 + (i * 31) % 11 for i in range(CAP + 1)]), 1),
            ("beyond-capacity-all-65536", np.full(65536, 3, dtype=np.uint32), 1),
            ("longcode-33", _longcode_histogram(33), 2)]


def _host_book(L, hist):
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.szhost_huff_build.restype = ctypes.POINTER(_Huff); L.szhost_huff_build.argtypes = [ctypes.c_int, vp, vp, sz]
    L.szhost_huff_tree_size.restype = sz; L.szhost_huff_tree_size.argtypes = [vp]
    L.szhost_huff_tree_write.restype = None; L.szhost_huff_tree_write.argtypes = [vp, vp]
    L.szhost_huff_free.restype = None; L.szhost_huff_free.argtypes = [vp]
    k = hist.size
    h = L.szhost_huff_build(2 * k, hist.ctypes.data, None, k)
    assert h
    try:
        tree = ctypes.create_string_buffer(L.szhost_huff_tree_size(h))
        L.szhost_huff_tree_write(h, tree)
        return dict(n_nodes=int(h.contents.n_nodes), tree=tree.raw, code=np.ctypeslib.as_array(h.contents.code, shape=(2 * k,))[:k].copy(),
                    len=np.ctypeslib.as_array(h.contents.len, shape=(2 * k,))[:k].copy(), total_bits=int(h.contents.total_bits))
    finally:
        L.szhost_huff_free(h)


@pytest.fixture
def shim(built):
    import sim_lib
    from sz_amd import api
    old = api._lib
    api._lib = api._bind(ctypes.CDLL(sim_lib.shim_path()))
    yield
    api._lib = old


@pytest.fixture
def ctx(built):
    import sz_amd
    c = sz_amd.HipContext(0)
    yield c
    c.close()


def _check_book(ctx, name, hist):
    import sz_amd
    want = _host_book(sz_amd.lib(), hist)
    rec, tree, code, ln = ctx.huff_book(hist)
    print(f"{name}: {int(np.count_nonzero(hist))} symbols of {hist.size}, {want['n_nodes']} nodes, longest code word {int(want['len'].max())} bits, status {rec.status}")
    assert rec.status == 0, (name, rec.status)
    assert rec.n_nodes == want["n_nodes"] and rec.tree_bytes == len(want["tree"]), (name, rec.n_nodes, rec.tree_bytes)
    assert tree == want["tree"], (name, "tree bytes differ")
    assert np.array_equal(ln, want["len"]), (name, "code lengths differ")
    assert np.array_equal(code, want["code"]), (name, "code words differ")
    assert rec.total_bits == want["total_bits"] and rec.max_len == int(want["len"].max()) and rec.total_unpred == int(hist[0]), name


def _check_declined(ctx, name, hist, status):
    rec, tree, code, ln = ctx.huff_book(hist)
    print(f"{name}: status {rec.status}")
    assert rec.status == status, (name, rec.status)
    assert rec.n_nodes == 0 and rec.tree_bytes == 0 and rec.total_bits == 0
    # nothing written: the buffers hold what the entry put there before the launch
    assert set(tree) == {0xA5} and np.all(code == 0xA5A5A5A5A5A5A5A5) and np.all(ln == 0xA5), name


@pytest.mark.gpu
@pytest.mark.parametrize("name,hist", HISTS, ids=[h[0] for h in HISTS])
def test_kernel_against_the_host_builder_on_the_gpu(ctx, name, hist):
    _check_book(ctx, name, hist)


@pytest.mark.gpu
@pytest.mark.parametrize("name,hist,status", DECLINED, ids=[h[0] for h in DECLINED])
def test_kernel_declines_on_the_gpu(ctx, name, hist, status):
    _check_declined(ctx, name, hist, status)


@pytest.mark.gpu
def test_kernel_takes_a_device_histogram_and_a_small_tree_buffer_on_the_gpu(ctx):
    import torch
    import sz_amd
    name, hist = HISTS[8]
    want = _host_book(sz_amd.lib(), hist)
    d = torch.from_numpy(hist.view(np.int32)).cuda()
    torch.cuda.synchronize()
    rec, tree, code, ln = ctx.huff_book(d.data_ptr(), on_device=True, intervals=hist.size)
    assert rec.status == 0 and tree == want["tree"] and np.array_equal(code, want["code"]) and np.array_equal(ln, want["len"])
    rec, tree, code, ln = ctx.huff_book(hist, tree_cap=len(want["tree"]) - 1)
    assert rec.status == 4 and np.all(ln == 0xA5)


SHIM_HISTS = [h for h in HISTS if h[0] in ("one-symbol", "one-symbol-bin0", "two-symbols", "equal-8", "equal-33", "equal-in-pairs", "geometric-30", "nonzero-255", "nonzero-256",
                                           "nonzero-257", "capacity-1024", "longcode-32", "random0-32", "random1-256", "random2-1024", "random3-65536")]


@pytest.mark.parametrize("name,hist", SHIM_HISTS, ids=[h[0] for h in SHIM_HISTS])
def test_kernel_against_the_host_builder_on_the_cpu_shim(shim, name, hist):
    import sz_amd
    c = sz_amd.HipContext(0)
    try:
        _check_book(c, name, hist)
    finally:
        c.close()


@pytest.mark.parametrize("name,hist,status", DECLINED[:1] + DECLINED[2:], ids=[DECLINED[0][0], DECLINED[2][0]])
def test_kernel_declines_on_the_cpu_shim(shim, name, hist, status):
    import sz_amd
    c = sz_amd.HipContext(0)
    try:
        _check_declined(c, name, hist, status)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------------------------ whole calls

# name: (shape, dtype, bound, symbols the oracle's book must have: (at least, at most)).  S-fields; the bounds are the ones at which the oracle finds no regression
# block and an alphabet of about 5 (a coarser bound brings regression blocks), about 60 and more than 256 symbols.  6 x 8 x 8 (384 values, one block column) reaches
# 258 symbols only at ABS 1e-7, where the optimiser picks 16384 intervals: a table of that size does not fit k_col_encode's LDS, the array takes the older packing
# passes (packing 0) and with them the host's book -- with or without the switch.  Its "many" is therefore ABS 1e-6 (102 symbols of 1024 intervals), the largest
# alphabet of that array that takes the natural-order passes; the 258-symbol case is pinned as what it is in test_an_alphabet_beyond_the_packing_passes_*.
def _whole_cases():
    out = {}
    for tag, shape, bounds in (("12x16x24", (12, 16, 24), (4e-3, 5e-5, 1e-6)), ("20x24x40", (20, 24, 40), (4e-3, 1e-4, 1e-5)), ("6x8x8", (6, 8, 8), (4e-3, 1e-5, 1e-6))):
        for dt in (f32, f64):
            for cls, eb, want in zip(("few", "sixty", "many"), bounds, ((4, 10), (40, 70), (100, 110) if tag == "6x8x8" else (257, 65536))):
                out[f"{tag}-{np.dtype(dt).name}-{cls}"] = (shape, dt, eb, want)
    return out


WHOLE = _whole_cases()
BEYOND = {"6x8x8-float32-258-symbols": ((6, 8, 8), f32, 1e-7, (257, 65536)), "6x8x8-float64-258-symbols": ((6, 8, 8), f64, 1e-7, (257, 65536))}
_REF = {}        # name -> dict(x, ref, dec): the oracle's stream and what its decoder makes of it, computed once


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _whole(oracle, name):
    if name not in _REF:
        from sz_amd.fields import s_field
        shape, dt, eb, (lo, hi) = (WHOLE.get(name) or BEYOND[name])
        x = s_field(*shape, dt)
        ref, st = oracle.compress(x, oracle.ABS, eb, want_stages=True)
        nsym = int((st["code_len"] > 0).sum())
        print(f"{name}: the oracle's book has {nsym} symbols of {st['intervals']}, longest code word {int(st['code_len'].max())} bits, use_mean {st.get('use_mean')}")
        assert st["reg_count"] == 0 and lo <= nsym <= hi, (name, st["reg_count"], nsym)
        _REF[name] = dict(x=x, eb=eb, ref=ref, dec=oracle.decompress(ref, x.shape, x.dtype))
    return _REF[name]


def _call(x, eb):
    """SZ_compress_args + SZ_decompress under tests/golden/sz_speed.config; returns (stream, decoded, the call's statistics)"""
    import sz_amd
    assert sz_amd.SZ_Init(os.path.join(ROOT, "tests", "golden", "sz_speed.config")) == 0
    try:
        got = sz_amd.SZ_compress_args(x, sz_amd.ABS, eb)
        st = sz_amd.SZ_hip_last_stats()
        stats = (int(st.book_on_device), int(st.packing), int(st.n_unpred))
        return got, sz_amd.SZ_decompress(got, x.shape, x.dtype), stats
    finally:
        sz_amd.SZ_Finalize()


def _check_whole(oracle, monkeypatch, name, switch, want_book, want_packing=1):
    c = _whole(oracle, name)
    for kv in filter(None, switch.split(";")):
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)
    got, dec, (book, packing, n_unpred) = _call(c["x"], c["eb"])
    print(f"{name} [{switch or 'default'}]: {len(got)} bytes, book_on_device {book}, packing {packing}, {n_unpred} unpredictable")
    assert len(got) == len(c["ref"]) and got == c["ref"], (name, switch, len(got), len(c["ref"]))
    assert np.array_equal(_bits(dec), _bits(c["dec"])), (name, switch)
    assert book == want_book and packing == want_packing, (name, switch, book, packing)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WHOLE))
def test_whole_call_with_the_device_book_on_the_gpu(oracle, monkeypatch, name):
    _check_whole(oracle, monkeypatch, name, "SZ_HIP_DEV_BOOK=1", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WHOLE))
def test_whole_call_with_the_switch_unset_on_the_gpu(oracle, monkeypatch, name):
    monkeypatch.delenv("SZ_HIP_DEV_BOOK", raising=False)
    _check_whole(oracle, monkeypatch, name, "", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BEYOND))
def test_an_alphabet_beyond_the_packing_passes_keeps_the_host_book_on_the_gpu(oracle, monkeypatch, name):
    _check_whole(oracle, monkeypatch, name, "SZ_HIP_DEV_BOOK=1", 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["12x16x24-float32-sixty", "20x24x40-float64-many"])
def test_forced_fallback_on_the_gpu(oracle, monkeypatch, name):
    _check_whole(oracle, monkeypatch, name, "SZ_HIP_DEV_BOOK=1;SZ_HIP_TEST_BOOK_FALLBACK=1", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["20x24x40-float32-sixty", "20x24x40-float32-many"])
def test_the_histogram_pass_of_larger_alphabets_and_the_unsliced_form_on_the_gpu(oracle, monkeypatch, name):
    """SZ_HIP_SEGHIST=0: the histogram comes from the second stream's pass (as for alphabets beyond 256 symbols), sliced beside the sweep or, SZ_HIP_SLICES=1, behind it"""
    _check_whole(oracle, monkeypatch, name, "SZ_HIP_DEV_BOOK=1;SZ_HIP_SEGHIST=0", 1)
    _check_whole(oracle, monkeypatch, name, "SZ_HIP_DEV_BOOK=1;SZ_HIP_SEGHIST=0;SZ_HIP_SLICES=1", 1)


def _regression_case(oracle):
    if "reg" not in _REF:
        from sz_amd.fields import reg_beside_lorenzo
        x = reg_beside_lorenzo(24, 40, 32)
        ref, st = oracle.compress(x, oracle.ABS, 1e-4, want_stages=True)
        assert st["reg_count"] > 0
        _REF["reg"] = dict(x=x, eb=1e-4, ref=ref, dec=oracle.decompress(ref, x.shape, x.dtype))
    return _REF["reg"]


def _check_regression_case(oracle, monkeypatch):
    c = _regression_case(oracle)
    monkeypatch.setenv("SZ_HIP_DEV_BOOK", "1")
    got, dec, (book, packing, _) = _call(c["x"], c["eb"])
    assert got == c["ref"] and np.array_equal(_bits(dec), _bits(c["dec"]))
    assert book == 0, "an array with regression blocks keeps the host's book"


@pytest.mark.gpu
def test_regression_blocks_keep_the_host_book_on_the_gpu(oracle, monkeypatch):
    _check_regression_case(oracle, monkeypatch)


@pytest.mark.gpu
def test_a_33_bit_code_word_falls_back_through_the_status_on_the_gpu(oracle, monkeypatch, tmp_path):
    """tests/longcode_fields.py's array for 33 bits: the kernel declines (status 2), the call goes round again with the host's book and the older packing passes"""
    import ref_cases
    import sz_amd
    import test_long_codes as TL
    c = TL._case(oracle, "L33")
    cfg = str(tmp_path / "sz_128.config")
    ref_cases.write_config(cfg, {"quantization_intervals": F.INTERVALS, "max_quant_intervals": F.INTERVALS, "absErrBound": F.BOUND})
    monkeypatch.setenv("SZ_HIP_DEV_BOOK", "1")
    assert sz_amd.SZ_Init(cfg) == 0
    try:
        got = sz_amd.SZ_compress_args(c["x"], sz_amd.ABS, F.BOUND)
        st = sz_amd.SZ_hip_last_stats()
        assert int(st.book_on_device) == 0 and int(st.packing) == 0
        assert len(got) == len(c["ref"]) and got == c["ref"]
    finally:
        sz_amd.SZ_Finalize()


@pytest.mark.gpu
def test_two_arrays_in_a_pool_with_the_switch_set_on_the_gpu(oracle, monkeypatch):
    import torch
    import sz_amd
    monkeypatch.setenv("SZ_HIP_DEV_BOOK", "1")
    work = [_whole(oracle, "20x24x40-float32-sixty"), _whole(oracle, "12x16x24-float64-many")]
    xs = [torch.from_numpy(w["x"]).cuda() for w in work]
    metas = [w["ref"][:4 + (28 if w["x"].dtype == np.float32 else 36)] for w in work]
    outs = [torch.empty(len(w["ref"]) + (1 << 16), dtype=torch.uint8, device="cuda") for w in work]
    torch.cuda.synchronize()
    pool = sz_amd.HipPool(0, 2)
    try:
        for order in ((0, 1), (1, 0)):
            tks = [(i, pool.submit(xs[i].data_ptr(), True, work[i]["x"].shape, work[i]["x"].dtype, work[i]["eb"], metas[i], None, outs[i].data_ptr(), outs[i].numel())) for i in order]
            for i, tk in tks:
                n, st = pool.wait(tk)
                assert n == len(work[i]["ref"]) and bytes(outs[i][:n].cpu().numpy()) == work[i]["ref"], (order, i)
                assert int(st.book_on_device) == 1 and int(st.packing) == 1, (order, i)
    finally:
        pool.close()


# ---- the same calls through the CPU shim (small arrays: the shim runs a lane at a time)
SHIM_WHOLE = ["6x8x8-float32-few", "6x8x8-float64-sixty", "6x8x8-float32-many", "12x16x24-float32-sixty", "12x16x24-float64-many"]


@pytest.mark.parametrize("name", SHIM_WHOLE)
def test_whole_call_with_the_device_book_on_the_cpu_shim(oracle, shim, monkeypatch, name):
    _check_whole(oracle, monkeypatch, name, "SZ_HIP_DEV_BOOK=1", 1)


def test_switch_unset_and_forced_fallback_on_the_cpu_shim(oracle, shim, monkeypatch):
    monkeypatch.delenv("SZ_HIP_DEV_BOOK", raising=False)
    _check_whole(oracle, monkeypatch, "12x16x24-float32-sixty", "", 0)
    _check_whole(oracle, monkeypatch, "12x16x24-float32-sixty", "SZ_HIP_DEV_BOOK=1;SZ_HIP_TEST_BOOK_FALLBACK=1", 0)
    _check_whole(oracle, monkeypatch, "12x16x24-float32-sixty", "SZ_HIP_DEV_BOOK=1;SZ_HIP_TEST_BOOK_FALLBACK=0;SZ_HIP_SEGHIST=0", 1)


def test_regression_blocks_keep_the_host_book_on_the_cpu_shim(oracle, shim, monkeypatch):
    _check_regression_case(oracle, monkeypatch)


def test_an_alphabet_beyond_the_packing_passes_keeps_the_host_book_on_the_cpu_shim(oracle, shim, monkeypatch):
    _check_whole(oracle, monkeypatch, "6x8x8-float32-258-symbols", "SZ_HIP_DEV_BOOK=1", 0, 0)


# ------------------------------------------------------------------------------------------------------------------ CPU: the binding and the record

def test_binding_structures_match_the_header(built, tmp_path):
    """sizeof / offsetof from include/szhip.h (compiled here) against the ctypes mirror: szhip_stats grew at its end only, by `book_on_device`"""
    from sz_amd import api
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "szhip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(szhip_stats), offsetof(szhip_stats, packing), offsetof(szhip_stats, book_on_device),\n'
                   '    sizeof(szhip_book_record), offsetof(szhip_book_record, status), offsetof(szhip_book_record, total_unpred)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    S, R = api.szhip_stats, api.szhip_book_record
    assert got == [ctypes.sizeof(S), S.packing.offset, S.book_on_device.offset, ctypes.sizeof(R), R.status.offset, R.total_unpred.offset], got
    assert S._fields_[-1][0] == "book_on_device" and S._fields_[-2][0] == "packing"
    assert S.book_on_device.offset == S.packing.offset + 4


def test_record_parse():
    from sz_amd import api
    raw = np.asarray([59, 1 + 9 * 59, 12, 0], dtype="<u4").tobytes() + np.asarray([123456789012, 77], dtype="<u8").tobytes()
    assert api.parse_book_record(raw) == dict(n_nodes=59, tree_bytes=532, max_len=12, status=0, total_bits=123456789012, total_unpred=77)
    declined = api.parse_book_record(np.asarray([0, 0, 0, 2], dtype="<u4").tobytes() + bytes(16))
    assert declined["status"] == 2 and declined["n_nodes"] == 0
    assert api.szhip_huff_book_tree_cap() == 1 + 9 * (2 * CAP - 1)
