"""Huffman code words of 31 bits and more in every packing and decoding path.

Every compress call picks its packing kernels by the longest code word of the code book (szhip_sz21.inc `enc_maxlen`, szhip_omp.inc `maxlen`): up to 32 bits
k_col_encode (or k_encode32 with SZ_HIP_SEGENC=0; k_omp_encode_box3 in the OpenMP container), from 33 bits on the block-ordering pass after all, k_chunk_bits and
the general k_encode (k_omp_encode_box); on the way back such words leave the 10-bit look-up window of k_hdec_*.  A code word of L bits needs F(L + 2) values in
the array, so no smooth or noisy field of a few million values reaches either side of that limit: tests/longcode_fields.py builds the arrays that do.

GPU (-m gpu): L = 31, 32 (the fast kernels' limit) and 33 (the first length on the fall-back), stream bytes against the oracle's and decoded bits against the
oracle decoder's; `SZ_hip_last_stats().packing` proves which kernels ran.
CPU: the same list of paths through the HIP-on-CPU shim at L = 20 and 24 -- this does NOT reach 32 bits (the arrays would hold 24 million values, the shim runs a
lane at a time); what it pins on every CPU run is code words of several bytes across the flush boundaries of the packers, in product code.  The host tree builder,
packer and decoder are driven from histograms (only counts: no large array) at depths 31, 32, 33, 48 and 64, and a depth of 65 must be refused.

Before any case runs, the oracle itself is asserted to give the case its code length (never skipped): max(code_len) == L (L + 1 on the SZ 1.4 path, whose first
value is stored exactly and adds symbol 0), no regression block, no unpredictable value, and its decoder returns the input bit for bit."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import longcode_fields as F  # noqa: E402

f32, f64 = np.float32, np.float64
META = bytes(range(1, 33))
SEED = 20


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _cube(L, not_multiple_of=None):
    return (F.smallest_cube(L, not_multiple_of),) * 3


# The arrays.  name: (L, shape, dtype).  Cubes, the smallest that have the places for L bits -- 31: 247^3 and 33: 341^3 (float64) have rows that are no multiple
# of four values, so k_pencil's codes feed the passes; 32: 292^3 and 33: 340^3 (float32) are the smallest cubes with rows of whole 16-byte vectors (the beam).
def _arrays():
    e32 = F.smallest_cube(32)
    while e32 % 4:
        e32 += 1
    return {"L20": (20, _cube(20), f32), "L20-f64": (20, _cube(20), f64), "L24": (24, _cube(24), f32), "L24-f64": (24, _cube(24), f64),
            "L31": (31, _cube(31), f32), "L32": (32, (e32,) * 3, f32), "L33": (33, _cube(33), f32), "L33-f64": (33, _cube(33, 4), f64),
            # more than twice the chain's values: the long code words begin with a 1 (longcode_fields.places_for_leading_one) -- beyond the smallest cubes
            "L20-msb": (20, (F.smallest_cube(20, None, True),) * 3, f32), "L32-msb": (32, (F.smallest_cube(32, None, True),) * 3, f32),
            "L33-msb": (33, (F.smallest_cube(33, None, True),) * 3, f32),
            "1D-L19": (19, (F.places_needed(19) + 5,), f32), "1D-L23-f64": (23, (F.places_needed(23) + 2,), f64),
            "1D-L31": (31, (F.places_needed(31) + 3,), f32), "1D-L32": (32, (F.places_needed(32) + 1,), f32),
            # for the SZ 1.4 path in 3-D, which predicts the first row of the first plane from the two values before (as a box of the OpenMP container): one box
            "sz14-L20": (20, _cube(20), f32, "one box"), "sz14-L24-f64": (24, _cube(24), f64, "one box"),
            "sz14-L31": (31, _cube(31), f32, "one box"), "sz14-L32": (32, _cube(32), f32, "one box")}


# The OpenMP container's arrays: boxes with 32 x 32 faces (the container takes at most 1024 rows a box), one code book over all boxes.  name: (L, shape, box, thread_num, dtype)
OMP_ARRAYS = {"omp-L20": (20, (64, 64, 64), (32, 32, 32), 8, f32), "omp-L24-f64": (24, (64, 64, 128), (32, 32, 64), 8, f64),
              "omp-L32": (32, (256, 256, 384), (32, 32, 48), 512, f32), "omp-L33": (33, (256, 256, 608), (32, 32, 76), 512, f32)}

_X = {}          # name -> array (each built once a module)
_ORACLE = {}     # (name, with_regression) -> dict(x, ref, longest): the oracle's stream; its decode is asserted equal to x and not kept twice


def _array(name):
    if name not in _X:
        t = time.time()
        if name in OMP_ARRAYS:
            L, shape, box, _, dtype = OMP_ARRAYS[name]
            _X[name] = F.longcode_field(L, shape, dtype, SEED, boxes=box)
        else:
            L, shape, dtype = _arrays()[name][:3]
            _X[name] = F.longcode_field(L, shape, dtype, SEED, boxes=shape if len(_arrays()[name]) > 3 else None)
        print(f"{name}: {_X[name].size} values generated in {time.time() - t:.1f} s, max |x| = {float(np.abs(_X[name]).max()):.0f}")
    return _X[name]


def _oracle_params(oracle, with_regression):
    # a fixed interval count is also what the config reader leaves in max_quant_intervals (conf.c:193-197; tests/test_ref_recorded.py)
    return oracle.default_params(with_regression=with_regression, quantization_intervals=F.INTERVALS, max_quant_intervals=F.INTERVALS)


def _case(oracle, name, with_regression=1):
    """The oracle's stream for the array, with the preconditions of the case asserted from the oracle's stages."""
    key = (name, with_regression)
    if key not in _ORACLE:
        x = _array(name)
        L = _arrays()[name][0]
        sz14 = not with_regression or x.ndim == 1
        t = time.time()
        ref, st = oracle.compress(x, oracle.ABS, F.BOUND, params=_oracle_params(oracle, with_regression), want_stages=True)
        longest, nsym = int(st["code_len"].max()), int((st["code_len"] > 0).sum())
        print(f"{name} (withRegression {with_regression}): the oracle's longest code word has {longest} bits, {nsym} symbols, {len(ref)} bytes ({time.time() - t:.1f} s)")
        assert st["intervals"] == F.INTERVALS
        if sz14:
            # SZ 1.4: the first value (1-D: the first two) is stored exactly -- symbol 0, one more leaf at the end of the chain
            assert longest == L + 1 and nsym == L + 2, (name, longest, nsym)
            assert st["exact_count"] == (2 if x.ndim == 1 else 1), (name, st["exact_count"])
        else:
            assert longest == L and nsym == L + 1, (name, longest, nsym)
            assert st["reg_count"] == 0 and st["total_unpred"] == 0, (name, st["reg_count"], st["total_unpred"])
            want_len = F.expected_code_lengths(L)
            assert {int(s): int(st["code_len"][s]) for s in np.flatnonzero(st["code_len"])} == want_len, name
        del st
        dec = oracle.decompress(ref, x.shape, x.dtype)
        assert np.array_equal(_bits(dec), _bits(x)), (name, "the oracle's decoder does not return the input")
        del dec
        if name.endswith("-msb"):
            # the tree's root (node 0) has the chain on its right (bit 1) and the leaf of code 64 on its left
            q = 4 + 28 + 8 + 4 + 4 + 4
            tree_bytes, nodes = int.from_bytes(ref[q:q + 4], "big"), int.from_bytes(ref[q + 4:q + 8], "big")
            tree = ref[q + 8:q + 8 + tree_bytes]
            left, leaf = tree[1], np.frombuffer(tree, np.uint8, nodes, 1 + 2 * nodes + 4 * nodes)
            sym = np.frombuffer(tree, np.uint32, nodes, 1 + 2 * nodes)
            assert x.size >= F.places_for_leading_one(L) and leaf[left] == 1 and sym[left] == F.INTERVALS // 2, (name, "the long code words do not begin with a 1")
        _ORACLE[key] = dict(x=x, ref=ref, longest=longest)
    return _ORACLE[key]


def _tree_code_lengths(tree, nodes):
    """{symbol: depth} of a serialised tree (Huffman.c:443-585: an endian byte, then the arrays L, R, C, t in pre-order)."""
    w = 1 if nodes <= 256 else (2 if nodes <= 65536 else 4)
    it = {1: np.uint8, 2: np.uint16, 4: np.uint32}[w]
    lc, rc = np.frombuffer(tree, it, nodes, 1), np.frombuffer(tree, it, nodes, 1 + w * nodes)
    c, t = np.frombuffer(tree, np.uint32, nodes, 1 + 2 * w * nodes), np.frombuffer(tree, np.uint8, nodes, 1 + 2 * w * nodes + 4 * nodes)
    lens, stack = {}, [(0, 0)]
    while stack:
        n, d = stack.pop()
        if t[n]:
            lens[int(c[n])] = d
        else:
            stack += [(int(lc[n]), d + 1), (int(rc[n]), d + 1)]
    return lens


def _omp_case(oracle, name):
    if (name, "omp") not in _ORACLE:
        L, shape, box, threads, dtype = OMP_ARRAYS[name]
        x = _array(name)
        p = oracle.default_params(); p.quantization_intervals = F.INTERVALS
        t = time.time()
        ref = oracle.omp_compress(x, F.BOUND, threads, META, p)
        q = len(META)
        nb = int.from_bytes(ref[q:q + 4], "big"); q += 4 + x.dtype.itemsize
        intervals, tree_bytes, nodes = (int.from_bytes(ref[q + 4 * i:q + 4 * i + 4], "big") for i in range(3)); q += 12
        lens = _tree_code_lengths(ref[q:q + tree_bytes], nodes); q += tree_bytes
        verbatim = int(np.frombuffer(ref, np.uint32, nb, q).astype(np.int64).sum())
        longest = max(lens.values())
        print(f"{name}: the oracle's longest code word has {longest} bits, {len(lens)} symbols, {nb} boxes, {len(ref)} bytes ({time.time() - t:.1f} s)")
        assert nb == threads and intervals == F.INTERVALS
        assert longest == L and lens == F.expected_code_lengths(L), (name, longest)
        assert verbatim == 0, (name, verbatim)
        dec = oracle.omp_decompress(ref, len(META), x.shape, x.dtype)
        assert np.array_equal(_bits(dec), _bits(x)), (name, "the oracle's decoder does not return the input")
        del dec
        _ORACLE[(name, "omp")] = dict(x=x, ref=ref, longest=longest, threads=threads)
    return _ORACLE[(name, "omp")]


@pytest.fixture(scope="module")
def cfg(tmp_path_factory):
    """tests/golden/sz_speed.config with quantization_intervals = 128"""
    import ref_cases
    path = str(tmp_path_factory.mktemp("longcodes") / "sz_128.config")
    ref_cases.write_config(path, {"quantization_intervals": F.INTERVALS, "max_quant_intervals": F.INTERVALS, "absErrBound": F.BOUND})
    return path


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


def _compress_and_decode(monkeypatch, cfg, c, name, switch, packing, with_regression=1):
    """The library's stream must be the oracle's, byte for byte, and what it decodes from it the input (= the oracle decoder's output), bit for bit."""
    import sz_amd
    _setenv(monkeypatch, switch)
    assert sz_amd.SZ_Init(cfg) == 0
    try:
        sz_amd.conf_params().withRegression = with_regression
        x, ref = c["x"], c["ref"]
        got = sz_amd.SZ_compress_args(x, sz_amd.ABS, F.BOUND)
        st = sz_amd.SZ_hip_last_stats()
        print(f"{name} [{switch or 'default'}]: oracle's longest code word {c['longest']} bits; {len(got)} bytes, intervals {int(st.intervals)}, packing {int(st.packing)}")
        if packing is not None:
            assert int(st.packing) == packing, (name, switch, "packing", int(st.packing), "longest code word", c["longest"])
        assert len(got) == len(ref) and got == ref, (name, switch, len(got), len(ref))
        dec = sz_amd.SZ_decompress(got, x.shape, x.dtype)
        assert np.array_equal(_bits(dec), _bits(x)), (name, switch, "decoded values differ from the reference decoder's")
    finally:
        sz_amd.SZ_Finalize()


def _decode_oracle_stream(monkeypatch, cfg, c, name, switch):
    import sz_amd
    _setenv(monkeypatch, switch)
    assert sz_amd.SZ_Init(cfg) == 0
    try:
        x = c["x"]
        dec = sz_amd.SZ_decompress(c["ref"], x.shape, x.dtype)
        print(f"{name} [decode, {switch or 'default'}]: oracle's longest code word {c['longest']} bits")
        assert np.array_equal(_bits(dec), _bits(x)), (name, switch, "decoded values differ from the reference decoder's")
    finally:
        sz_amd.SZ_Finalize()


def _omp_round(ctx, c, name, fast):
    import sz_amd
    x, ref = c["x"], c["ref"]
    got, n, st = ctx.compress_omp(x.ctypes.data, False, x.shape, x.dtype, F.BOUND, c["threads"], META, sz_amd.api.szhip_params(100, 0.99, 65536, F.INTERVALS))
    print(f"{name}: oracle's longest code word {c['longest']} bits ({'k_omp_encode_box3' if fast else 'k_omp_encode_box'}); {n} bytes")
    assert n == len(ref) and got == ref, name
    out = np.empty_like(x)
    buf = ctypes.create_string_buffer(ref, len(ref))
    ctx.decompress_omp(ctypes.addressof(buf), False, len(ref), len(META), x.shape, x.dtype, out.ctypes.data, False)
    assert np.array_equal(_bits(out), _bits(x)), name


# the paths of a compress call: (switches, value of szhip_stats.packing when the code book fits the fast kernels)
ENCODE_PATHS = [("", 1),                                                  # k_col_encode
                ("SZ_HIP_SEGENC=0", 0),                                   # k_encode32
                ("SZ_HIP_SEGENC=0;SZ_HIP_ENC32=0", 0),                    # k_chunk_bits + k_encode
                ("SZ_HIP_SEG_SEGB=1", 1), ("SZ_HIP_SEG_TILE_KB=4", 1),    # k_col_encode: rounds at their smallest under a window sized for the longest words
                ("SZ_HIP_SEG_SEGB=1;SZ_HIP_SEG_TILE_KB=4", 1)]
DECODE_PATHS = ["", "SZ_HIP_COL_UNPACK=0", "SZ_HIP_TEST_HDEC_FALLBACK=1"]


# ------------------------------------------------------------------------------------------------------------------ CPU: the generator

@pytest.mark.parametrize("name", ["L20", "L20-f64", "L24", "L24-f64"])
def test_generator_gives_the_oracle_a_chain_of_L_bits(oracle, name):
    c = _case(oracle, name)
    assert c["longest"] == _arrays()[name][0]


@pytest.mark.parametrize("name", ["sz14-L20", "sz14-L24-f64", "1D-L19", "1D-L23-f64"])
def test_generator_on_the_sz14_path_gives_L_plus_one_bits(oracle, name):
    c = _case(oracle, name, 0)
    assert c["longest"] == _arrays()[name][0] + 1


def test_generator_balances_the_signs_and_checks_its_conditions():
    for L in (20, 24, 31, 32, 33, 48):
        c, v = F.chain_counts(L), F.chain_values(L)
        assert sorted(abs(a) for a in v) == sorted((j // 2) + 1 for j in range(L)) and len(set(v)) == L
        # the drift of the array is the sum of count x value: with the signs alternating it is a good part of the array's size, balanced a thousandth of it at most
        drift = abs(sum(a * b for a, b in zip(c, v)))
        naive = abs(sum(a * abs(b) * (-1) ** j for j, (a, b) in enumerate(zip(c, v))))
        print(L, "sum of count x value:", drift, "with alternating signs:", naive, "values:", sum(c))
        assert drift * 1000 <= sum(c) and drift * 100 <= naive, (L, drift, naive)
        # a chain: every merged node is lighter than the leaf after next, and the zeros outweigh everything
        for k in range(1, L - 1):
            assert sum(c[:k]) < c[k + 1]
    with pytest.raises(AssertionError, match="needs"):
        F.longcode_field(20, (42, 42, 42), f32, 1)                       # 74088 places, 75001 needed
    assert F.smallest_cube(20) == 43 and F.places_needed(33) > 39_000_000
    with pytest.raises(AssertionError, match="not exact"):               # a float32 array cannot carry what 2^24 does not hold
        import unittest.mock as um
        with um.patch.object(F, "chain_values", lambda L: [(-1) ** j * ((L - 1 - j) // 2 + 1) * 40 for j in range(L)]), um.patch.object(F, "INTERVALS", 4096):
            F.longcode_field(24, (81, 81, 81), f32, 1)


# ------------------------------------------------------------------------------------------------------------------ CPU: the shim, L = 20 and 24

@pytest.mark.parametrize("switch,packing", ENCODE_PATHS)
@pytest.mark.parametrize("name", ["L20", "L24-f64", "L20-msb"])
def test_compress_paths_on_the_cpu_shim(oracle, shim, monkeypatch, cfg, name, switch, packing):
    """(20 and 24 bits: not the 32-bit limit -- code words of three bytes across the packers' flushes, in product code, on every CPU run)"""
    _compress_and_decode(monkeypatch, cfg, _case(oracle, name), name, switch, packing)


@pytest.mark.parametrize("switch", DECODE_PATHS)
@pytest.mark.parametrize("name", ["L20-f64", "L24"])
def test_decode_paths_on_the_cpu_shim(oracle, shim, monkeypatch, cfg, name, switch):
    _decode_oracle_stream(monkeypatch, cfg, _case(oracle, name), name, switch)


@pytest.mark.parametrize("name", ["sz14-L20", "sz14-L24-f64", "1D-L19", "1D-L23-f64"])
def test_sz14_path_on_the_cpu_shim(oracle, shim, monkeypatch, cfg, name):
    _compress_and_decode(monkeypatch, cfg, _case(oracle, name, 0), name, "", None, with_regression=0)


@pytest.mark.parametrize("name", ["omp-L20", "omp-L24-f64"])
def test_omp_container_on_the_cpu_shim(oracle, shim, name):
    import sz_amd
    ctx = sz_amd.HipContext(0)
    try:
        _omp_round(ctx, _omp_case(oracle, name), name, True)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ GPU: L = 31, 32, 33

@pytest.mark.gpu
@pytest.mark.parametrize("name,packing", [("L31", 1), ("L32", 1), ("L33", 0), ("L33-f64", 0), ("L32-msb", 1), ("L33-msb", 0)])
def test_default_configuration_on_the_gpu(oracle, monkeypatch, cfg, name, packing):
    """packing == 1: k_col_encode ran; == 0: the call went back to the block-ordered copy, k_chunk_bits and k_encode -- the switch sits between 32 and 33 bits"""
    _compress_and_decode(monkeypatch, cfg, _case(oracle, name), name, "", packing)


@pytest.mark.gpu
@pytest.mark.parametrize("name,switch", [("L32", "SZ_HIP_SEGENC=0"), ("L32", "SZ_HIP_SEGENC=0;SZ_HIP_ENC32=0"), ("L33", "SZ_HIP_SEGENC=0"), ("L32-msb", "SZ_HIP_SEGENC=0")])
def test_the_older_passes_on_the_gpu(oracle, monkeypatch, cfg, name, switch):
    _compress_and_decode(monkeypatch, cfg, _case(oracle, name), name, switch, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["SZ_HIP_SEG_SEGB=1", "SZ_HIP_SEG_TILE_KB=4", "SZ_HIP_SEG_SEGB=1;SZ_HIP_SEG_TILE_KB=4"])
def test_segment_geometry_at_32_bits_on_the_gpu(oracle, monkeypatch, cfg, switch):
    _compress_and_decode(monkeypatch, cfg, _case(oracle, "L32"), "L32", switch, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", DECODE_PATHS)
@pytest.mark.parametrize("name", ["L32", "L33"])
def test_decoding_the_oracles_streams_on_the_gpu(oracle, monkeypatch, cfg, name, switch):
    _decode_oracle_stream(monkeypatch, cfg, _case(oracle, name), name, switch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sz14-L31", "sz14-L32", "1D-L31", "1D-L32"])
def test_sz14_path_on_the_gpu(oracle, monkeypatch, cfg, name):
    """withRegression = 0 (a 1-D series takes the path anyway): the code books of the L = 31 and 32 arrays come out at 32 and 33 bits there"""
    c = _case(oracle, name, 0)
    assert c["longest"] == {"sz14-L31": 32, "sz14-L32": 33, "1D-L31": 32, "1D-L32": 33}[name]
    _compress_and_decode(monkeypatch, cfg, c, name, "", None, with_regression=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fast", [("omp-L32", True), ("omp-L33", False)])
def test_omp_container_on_the_gpu(oracle, name, fast):
    import sz_amd
    ctx = sz_amd.HipContext(0)
    try:
        _omp_round(ctx, _omp_case(oracle, name), name, fast)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_pool_takes_a_33_bit_array_beside_an_ordinary_field(oracle):
    """The fall-back re-enters the block-ordering pass on a context that had prepared (and, a call earlier, used) the segment path: both arrays through both lanes."""
    import torch
    import sz_amd
    from sz_amd.fields import s_field
    c = _case(oracle, "L33")
    s = s_field(96, 128, 160)
    s_ref, _ = oracle.compress(s, oracle.ABS, 1e-4)
    work = [(c["x"], F.BOUND, c["ref"], sz_amd.api.szhip_params(100, 0.99, F.INTERVALS, F.INTERVALS)), (s, 1e-4, s_ref, None)]
    xs = [torch.from_numpy(w[0]).cuda() for w in work]
    metas = [w[2][:4 + 28] for w in work]
    outs = [torch.empty(len(w[2]) + (1 << 16), dtype=torch.uint8, device="cuda") for w in work]
    pool = sz_amd.HipPool(0, 2)
    try:
        for order in ((0, 1), (1, 0), (0, 1), (1, 0)):              # two calls in flight; the lanes see the arrays in both orders
            tks = [(i, pool.submit(xs[i].data_ptr(), True, work[i][0].shape, work[i][0].dtype, work[i][1], metas[i], work[i][3], outs[i].data_ptr(), outs[i].numel()))
                   for i in order]
            for i, tk in tks:
                n, st = pool.wait(tk)
                assert int(st.packing) == (0 if i == 0 else 1), (order, i, int(st.packing))
                assert n == len(work[i][2]) and bytes(outs[i][:n].cpu().numpy()) == work[i][2], (order, i)
        print(f"pool: oracle's longest code word {c['longest']} bits beside an S-field")
    finally:
        pool.close()


# ------------------------------------------------------------------------------------------------------------------ CPU: the host tree builder, packer and decoder from histograms

class _Huff(ctypes.Structure):      # sz_amd/csrc/szhost.h
    _fields_ = [("state_num", ctypes.c_int), ("n_nodes", ctypes.c_int), ("code", ctypes.POINTER(ctypes.c_uint64)),
                ("len", ctypes.POINTER(ctypes.c_uint8)), ("L", ctypes.POINTER(ctypes.c_uint32)), ("R", ctypes.POINTER(ctypes.c_uint32)),
                ("C", ctypes.POINTER(ctypes.c_uint32)), ("t", ctypes.POINTER(ctypes.c_uint8)), ("total_bits", ctypes.c_uint64)]


class _OHuff(ctypes.Structure):     # oracle/szo.h
    _fields_ = [("state_num", ctypes.c_int), ("n_nodes", ctypes.c_int), ("root", ctypes.c_int), ("freq", ctypes.POINTER(ctypes.c_uint64)),
                ("left", ctypes.POINTER(ctypes.c_int)), ("right", ctypes.POINTER(ctypes.c_int)), ("sym", ctypes.POINTER(ctypes.c_uint)),
                ("leaf", ctypes.POINTER(ctypes.c_ubyte)), ("code", ctypes.POINTER(ctypes.c_uint64)), ("len", ctypes.POINTER(ctypes.c_ubyte)),
                ("used", ctypes.POINTER(ctypes.c_ubyte))]


STATES = 2 * F.INTERVALS


@pytest.fixture(scope="module")
def host(built):
    import sz_amd
    L = sz_amd.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.szhost_huff_build.restype = ctypes.POINTER(_Huff); L.szhost_huff_build.argtypes = [ctypes.c_int, vp, vp, sz]
    L.szhost_huff_from_bytes.restype = ctypes.POINTER(_Huff); L.szhost_huff_from_bytes.argtypes = [ctypes.c_int, vp, ctypes.c_int]
    L.szhost_huff_tree_size.restype = sz; L.szhost_huff_tree_size.argtypes = [vp]
    L.szhost_huff_serial_size.restype = sz; L.szhost_huff_serial_size.argtypes = [ctypes.c_int]
    L.szhost_huff_tree_write.restype = None; L.szhost_huff_tree_write.argtypes = [vp, vp]
    L.szhost_huff_encode_i32.restype = sz; L.szhost_huff_encode_i32.argtypes = [vp, vp, sz, vp]
    L.szhost_huff_decode_i32.restype = ctypes.c_int; L.szhost_huff_decode_i32.argtypes = [vp, vp, sz, sz, vp]
    L.szhost_huff_free.restype = None; L.szhost_huff_free.argtypes = [vp]
    return L


@pytest.fixture(scope="module")
def ohuff(oracle):
    O = oracle.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    O.szo_huff_from_freq.restype = ctypes.POINTER(_OHuff); O.szo_huff_from_freq.argtypes = [ctypes.c_int, vp, sz]
    O.szo_huff_node_count.restype = sz; O.szo_huff_node_count.argtypes = [vp]
    O.szo_huff_tree_to_bytes.restype = sz; O.szo_huff_tree_to_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p)]
    O.szo_huff_encode.restype = sz; O.szo_huff_encode.argtypes = [vp, vp, sz, vp]
    O.szo_huff_free.restype = None; O.szo_huff_free.argtypes = [vp]
    return O


def _chain_histogram(depth, order, seed=1):
    """A histogram (uint64, STATES bins) whose Huffman tree has depth `depth`: the chain's counts and one symbol that outweighs them, at symbols spread over the
    alphabet in the given order of weight ("up", "down" or "mixed": the heap sees the leaves in symbol order)."""
    c = F.chain_counts(depth)
    counts = c + [c[-1] + c[-2] + 1]
    rng = np.random.default_rng(seed + depth)
    syms = np.sort(rng.permutation(STATES)[:len(counts)])
    if order == "down":
        syms = syms[::-1]
    elif order == "mixed":
        syms = rng.permutation(syms)
    h = np.zeros(STATES, dtype=np.uint64)
    h[syms] = np.asarray(counts, dtype=np.uint64)
    return h


def _fibonacci_histogram(terms):
    """exact Fibonacci counts: every merge meets a leaf of its own weight -- the heap's order among equals decides the tree"""
    f = [1, 1]
    while len(f) < terms:
        f.append(f[-1] + f[-2])
    h = np.zeros(STATES, dtype=np.uint64)
    h[np.arange(terms) * 3 + 2] = np.asarray(f, dtype=np.uint64)
    return h


def _oracle_book(O, hist):
    """(lengths, right-aligned code bits as Python ints, tree bytes) of the oracle's Huffman (oracle/szo_huffman.c) for a histogram"""
    h = O.szo_huff_from_freq(STATES, hist.ctypes.data, hist.size)
    assert h
    lens = np.ctypeslib.as_array(h.contents.len, shape=(STATES,)).copy()
    msb = np.ctypeslib.as_array(h.contents.code, shape=(STATES,)).copy()
    codes = [int(msb[s]) >> (64 - int(lens[s])) if lens[s] else 0 for s in range(STATES)]
    out = ctypes.c_void_p()
    n = O.szo_huff_tree_to_bytes(h, ctypes.byref(out))
    tree = ctypes.string_at(out.value, n)
    nodes = int(O.szo_huff_node_count(h))
    O.free(out)
    return h, lens, codes, tree, nodes


HISTOGRAMS = [(f"depth{d}-{o}", d, o) for d in (31, 32, 33, 48, 64) for o in ("up", "down", "mixed")] + [("fibonacci-60", None, "fib")]


@pytest.mark.parametrize("name,depth,order", HISTOGRAMS, ids=[h[0] for h in HISTOGRAMS])
def test_host_tree_builder_from_a_histogram(host, ohuff, name, depth, order):
    """szhost_huff_build, the table write and szhost_huff_serial_size against the oracle's Huffman on the same histogram: code lengths, code bits, tree bytes.
    Only a histogram reaches these depths: an ARRAY with a code word of L bits has F(L + 2) values at least -- 10^10 for 48 bits, 2 x 10^13 for 64."""
    hist = _fibonacci_histogram(60) if order == "fib" else _chain_histogram(depth, order)
    oh, olens, ocodes, otree, onodes = _oracle_book(ohuff, hist)
    try:
        print(name, "oracle's longest code word", int(olens.max()), "bits,", onodes, "nodes")
        if depth is not None:
            assert int(olens.max()) == depth and onodes == 2 * (depth + 1) - 1
        else:
            assert 31 < int(olens.max()) <= 64
        h = host.szhost_huff_build(STATES, None, hist.ctypes.data, hist.size)
        assert h
        try:
            assert h.contents.n_nodes == onodes
            lens = np.ctypeslib.as_array(h.contents.len, shape=(STATES,))
            codes = np.ctypeslib.as_array(h.contents.code, shape=(STATES,))
            assert np.array_equal(lens, olens)
            assert [int(x) for x in codes] == ocodes
            assert h.contents.total_bits == sum(int(hist[s]) * int(olens[s]) for s in range(STATES))
            assert host.szhost_huff_tree_size(h) == host.szhost_huff_serial_size(onodes) == len(otree)
            tree = ctypes.create_string_buffer(len(otree))
            host.szhost_huff_tree_write(h, tree)
            assert tree.raw == otree
            # and back from the bytes: the same table
            h2 = host.szhost_huff_from_bytes(STATES, otree, onodes)
            assert h2
            assert np.array_equal(np.ctypeslib.as_array(h2.contents.len, shape=(STATES,)), olens)
            assert [int(x) for x in np.ctypeslib.as_array(h2.contents.code, shape=(STATES,))] == ocodes
            host.szhost_huff_free(h2)
        finally:
            host.szhost_huff_free(h)
    finally:
        ohuff.szo_huff_free(oh)


def test_host_tree_builder_refuses_a_depth_of_65(host, capfd):
    """code words above 64 bits do not fit the tables: the build fails with a message, it does not return a table"""
    for order in ("up", "down", "mixed"):
        hist = _chain_histogram(65, order)
        h = host.szhost_huff_build(STATES, None, hist.ctypes.data, hist.size)
        assert not h, order
    assert "longer than 64 bits" in capfd.readouterr().err
    hist = _chain_histogram(64, "up")                              # (the depth before it is taken)
    h = host.szhost_huff_build(STATES, None, hist.ctypes.data, hist.size)
    assert h
    host.szhost_huff_free(h)


def _pack_msb_first(words):
    """[(code bits, length)] -> bytes, most significant bit first, zero padded (Huffman.c:205-308)"""
    acc, n = 0, 0
    for bits, ln in words:
        assert 0 < ln <= 64 and bits >> ln == 0
        acc = (acc << ln) | bits
        n += ln
    pad = -n % 8
    return ((acc << pad).to_bytes((n + pad) // 8, "big")) if n else b""


@pytest.mark.parametrize("count", [300, 5000])          # the decoder walks bit by bit below 4096 symbols and looks 12 bits up in a table from there on
@pytest.mark.parametrize("depth", [48, 64])
def test_host_packer_and_decoder_with_long_code_words(host, ohuff, depth, count):
    """szhost_huff_encode_i32 (code words above 32 bits go in as two pieces) and szhost_huff_decode_i32 under tables of depth 48 and 64, against a plain bit packer."""
    hist = _chain_histogram(depth, "mixed")
    oh, olens, ocodes, otree, onodes = _oracle_book(ohuff, hist)
    h = host.szhost_huff_build(STATES, None, hist.ctypes.data, hist.size)
    assert h
    try:
        used = np.flatnonzero(hist)
        by_len = used[np.argsort(olens[used], kind="stable")]
        rng = np.random.default_rng(depth + count)
        # every symbol, the longest words next to one another and beside the shortest, then a random mix weighted towards the long words
        seq = list(by_len) + [by_len[-1]] * 5 + [by_len[0], by_len[-2], by_len[0], by_len[-1], by_len[-2]] * 3
        seq += list(rng.choice(by_len, size=count - len(seq), p=np.arange(1, len(by_len) + 1) / np.arange(1, len(by_len) + 1).sum()))
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        assert seq.size == count and int(olens[seq].max()) == depth
        want = _pack_msb_first([(ocodes[s], int(olens[s])) for s in seq])
        obuf = np.zeros(len(want) + 16, dtype=np.uint8)
        assert ohuff.szo_huff_encode(oh, seq.ctypes.data, seq.size, obuf.ctypes.data) == len(want) and bytes(obuf[:len(want)]) == want
        buf = np.full(len(want) + 16, 0xAA, dtype=np.uint8)
        n = host.szhost_huff_encode_i32(h, seq.ctypes.data, seq.size, buf.ctypes.data)
        assert n == len(want) and bytes(buf[:n]) == want
        assert bytes(buf[n:]) == b"\xaa" * 16                                      # nothing written behind the payload
        for table in (h, host.szhost_huff_from_bytes(STATES, otree, onodes)):      # the encoder's table and the one a decompressor builds from the stream's tree
            assert table
            out = np.full(count, -1, dtype=np.int32)
            assert host.szhost_huff_decode_i32(table, buf.ctypes.data, n, count, out.ctypes.data) == 1
            assert np.array_equal(out, seq)
            # a payload that ends inside the last code word is refused
            assert host.szhost_huff_decode_i32(table, buf.ctypes.data, n - (int(olens[seq[-1]]) + 7) // 8, count, out.ctypes.data) == 0
            if table is not h:
                host.szhost_huff_free(table)
    finally:
        host.szhost_huff_free(h)
        ohuff.szo_huff_free(oh)
