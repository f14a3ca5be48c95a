"""Many small same-shape arrays in one call (include/szhip.h: szhip_compress_omp_batch, szhip_decompress_omp_batch; include/sz.h: SZ_hip_*_openmp_batch).

The bar, with no tolerance: blob[offset_i, offset_i + size_i) is byte for byte oracle.omp_compress of array i alone with its own bound and parameter bytes; the batched
decode writes into out_i bit for bit oracle.omp_decompress of stream i -- NaN payloads and signed zeros included -- and every other byte of every allocation stays what
it was; inputs are never written.  The checker is the oracle on each array alone, never the code under test.  What keeps a loop over single calls from passing: every
item of the shared launches reports batched == 1 and stats.quant_kernel_launches counts ONE sweep launch per form, whatever the number of arrays.  Which items those
are follows from the documented fallback rule and the oracle's own streams (an interval count above 1024, a one-symbol book, boxes of 210 points).

The arrays of a batch differ in content, bound and parameter bytes; a compress case runs with the interval optimiser (quantization_intervals = 0: the arrays end up
with different interval counts, trees and header lengths -- asserted from the oracle's streams) and with a fixed count.  The same groups run on the CPU shim
(tests/sim; its "device" memory is host memory) and, under -m gpu, through the built library; one larger group runs on the GPU only.

A constant array takes the single call's fast packer today (its one-symbol book has a code word of one bit), so the shared COMPRESS launches cover it (batched == 1);
its stream has a one-symbol book, which the look-up-table decoder does not take: the batched DECODE hands it to the single call (batched == 0)."""
import ctypes
import os

import numpy as np
import pytest

import ptr_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = {4: 0x7FC0DEAD, 8: 0x7FF8DEAD0000BEEF}
FIXED_INTERVALS = 256
OK, ERR_ARG, ERR_UNSUP, ERR_STREAM = 0, -2, -3, -4
COL, BOX, ODD = (8, 64, 64), (16, 16, 16), (12, 10, 14)      # thread_num 8: boxes 4 x 32 x 32 (k_omp_col), 8^3 (k_omp_box), 6 x 5 x 7 = 210 points (no multiple of 8)
THREADS = 8
_ARR = {}
_REF = {}            # (array name, intervals) -> (stream, decoded array): the oracle's, computed once, never changed


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _meta(i):
    """32 parameter bytes, different for every item of a batch"""
    return bytes((7 * i + k + 1) & 0xFF for k in range(32))


def _special(shape, dtype):
    """zeros of both signs, a NaN, an infinity, values far outside the quantiser's range, a constant stretch (as tests/test_omp_view.py)"""
    from sz_amd.fields import s_field
    d = s_field(*shape, np.dtype(dtype).type)
    f = d.ravel()
    f[3] = 0.0; f[4] = -0.0; f[5] = 1e30; f[6] = -1e30; f[40:90] = -0.0; f[100:400] = 0.25
    f[f.size // 2] = np.nan; f[f.size // 2 + 7] = np.inf
    return d


def _noisy(shape, dtype):
    """an S-field with one box of noise (as _noisy of tests/test_omp_view.py, the noise small enough for the optimiser to stay at or below 1024 intervals at 1e-4)"""
    from sz_amd.fields import s_field
    d = s_field(*shape, np.dtype(dtype).type, z0=40)
    r0, r1, r2 = shape
    d[:r0 // 2, :r1 // 2, r2 // 2:] = (np.random.default_rng(8).standard_normal((r0 // 2, r1 // 2, r2 - r2 // 2)) * 0.005).astype(dtype)
    return d


def _array(name):
    """name -> (values, eb): `kind-shape-dtype`"""
    if name not in _ARR:
        from sz_amd.fields import m_field, s_field
        kind, shp, dt = name.split("/")
        shape = {"col": COL, "box": BOX, "odd": ODD, "c64": (64, 64, 64)}[shp]
        dtype = np.float32 if dt == "f32" else np.float64
        if kind.startswith("s@"):                                            # an S-field slice starting at plane z0
            a, eb = s_field(*shape, dtype, z0=int(kind[2:])), 1e-4 if shp == "c64" else 1e-3
        elif kind == "noisy":
            a, eb = _noisy(shape, dtype), 1e-4
        elif kind == "special":
            a, eb = _special(shape, dtype), 1e-3
        elif kind == "m":                                                    # most values verbatim
            a, eb = np.ascontiguousarray(m_field(64, dtype)[28:28 + shape[0], :shape[1], :shape[2]]), 1e-6
        elif kind == "tight":                                                # an S-field at a 10 x tighter bound
            a, eb = s_field(*shape, dtype, z0=16), 1e-4
        elif kind == "noise":                                                # noise at a tight bound: the optimiser picks more than 1024 intervals
            a, eb = (np.random.default_rng(3).standard_normal(shape) * 0.05).astype(dtype), 1e-5
        elif kind == "constant":
            a, eb = np.full(shape, 1.5, dtype=dtype), 1e-3
        else:
            raise KeyError(name)
        a = np.ascontiguousarray(a); a.setflags(write=False)
        _ARR[name] = (a, eb)
    return _ARR[name]


def _five(shp, dt):
    return [f"{k}/{shp}/{dt}" for k in ("s@0", "noisy", "special", "m", "tight")]


def _ref(oracle, name, i, intervals):
    """the oracle's stream of array `name` as item i of a batch (its parameter bytes are the item's), and what the oracle decodes from it"""
    key = (name, i, intervals)
    if key not in _REF:
        a, eb = _array(name)
        p = oracle.default_params(); p.quantization_intervals = intervals
        s = oracle.omp_compress(a, eb, THREADS, _meta(i), p)
        dec = oracle.omp_decompress(s, 32, a.shape, a.dtype)
        dec.setflags(write=False)
        _REF[key] = (s, dec)
    return _REF[key]


def _field(stream, esz, which):
    """a header field of an OpenMP-container stream behind 32 parameter bytes: thread_num | eb | intervals | tree_bytes | nodes"""
    at = {"intervals": 36 + esz, "tree_bytes": 40 + esz}[which]
    return int.from_bytes(stream[at:at + 4], "big")


def _n_unpred(stream, esz):
    at = 32 + 4 + esz + 12 + _field(stream, esz, "tree_bytes")
    return int(np.frombuffer(stream[at:at + 4 * THREADS], dtype=np.uint32).sum())


def _form(shape, ptr):
    c = [n // 2 for n in shape]
    if c[1] == 32 and c[2] == 32:
        return 3 if ptr % 16 == 0 else 5
    return 4 if c[2] % 4 == 0 and ptr % 16 == 0 else 5


def _params(iv):
    from sz_amd import api
    return api.szhip_params(100, 0.99, 65536, iv)


def _compress(ctx, oracle, names, device, iv, offs=None, data_dev=True, out_dev=False, expect_batched=None, forms=None, launches=None):
    """one batch compress call of the arrays `names`, item i `offs[i]` bytes behind a 256-byte boundary; everything the bar asks, per item"""
    arrs = [_array(n) for n in names]
    esz = arrs[0][0].dtype.itemsize
    offs = offs or [0] * len(names)
    regs = [ptr_cases.carve(a.nbytes, off, pad=256, device=device and data_dev).put(a) for (a, _), off in zip(arrs, offs)]
    rc, blob, size, items, st = ctx.compress_omp_batch([r.ptr for r in regs], data_dev, arrs[0][0].shape, arrs[0][0].dtype, [eb for _, eb in arrs], THREADS,
                                                       [_meta(i) for i in range(len(names))], _params(iv), out_dev)
    assert rc == OK
    if out_dev:
        blob = ctx.debug_fetch(13, size, np.uint8).tobytes()                 # (the context's blob of the last batch)
    end = 0
    for i, name in enumerate(names):
        what = f"item {i} ({name}), intervals {iv}"
        want, _ = _ref(oracle, name, i, iv)
        it = items[i]
        assert it.rc == OK, what
        assert it.offset >= end and it.offset % 64 == 0 and it.offset + it.size <= size, (what, it.offset, it.size, size)      # offsets increase, streams do not overlap
        end = it.offset + it.size
        got = blob[it.offset:it.offset + it.size]
        assert it.size == len(want) and got == want, f"{what}: the stream differs from the oracle's stream of the array alone ({it.size} / {len(want)} bytes)"
        assert it.intervals == _field(want, esz, "intervals") and (iv == 0 or it.intervals == iv), what
        assert it.n_unpred == _n_unpred(want, esz), what
        # (the fallback rule, from the oracle's stream: an array for which the optimiser picks more than 1024 intervals takes the single call)
        assert it.batched == ((1 if it.intervals <= 1024 else 0) if expect_batched is None else expect_batched[i]), (what, it.batched)
        if it.batched:
            assert it.quant_kernel == (forms[i] if forms else _form(arrs[0][0].shape, regs[i].ptr if data_dev else 0)), (what, it.quant_kernel)
        assert np.array_equal(regs[i].get(), _bits(arrs[i][0]).view(np.uint8)), f"{what}: the input was written"
        regs[i].check(what)
    if launches is not None:
        assert st.quant_kernel_launches == launches, (names, st.quant_kernel_launches)
    return items, st


def _decode(ctx, oracle, names, device, iv=0, offs=None, stream_dev=True, out_dev=True, stream_off=1, expect_batched=None, launches=None, damage=None):
    """one batch decode of the oracle's streams of `names`; damage = (item, how): that stream is damaged and must fail alone"""
    arrs = [_array(n) for n in names]
    a0 = arrs[0][0]
    esz = a0.dtype.itemsize
    offs = offs or [0] * len(names)
    streams = [bytearray(_ref(oracle, n, i, iv)[0]) for i, n in enumerate(names)]
    lens = [len(s) for s in streams]
    if damage:
        k, how = damage
        if how == "truncated":
            lens[k] -= 5
        else:                                                                # one entry of the verbatim-count table raised by one ("moved": and the next one lowered
            at = 32 + 4 + esz + 12 + _field(bytes(streams[k]), esz, "tree_bytes")      # by one -- every table stays where it is, only the device can tell)
            streams[k][at:at + 4] = (int.from_bytes(streams[k][at:at + 4], "little") + 1).to_bytes(4, "little")
            if how == "moved":
                assert int.from_bytes(streams[k][at + 4:at + 8], "little") > 0
                streams[k][at + 4:at + 8] = (int.from_bytes(streams[k][at + 4:at + 8], "little") - 1).to_bytes(4, "little")
    sregs = [ptr_cases.carve(len(s), stream_off, pad=256, device=device and stream_dev).put(bytes(s)) for s in streams]
    before = np.empty(a0.size, dtype=a0.dtype)
    before.view(np.uint32 if esz == 4 else np.uint64)[:] = SENTINEL[esz]
    oregs = [ptr_cases.carve(a0.nbytes, off, pad=256, device=device and out_dev).put(before) for off in offs]
    rc, items, st = ctx.decompress_omp_batch([(r.ptr, n) for r, n in zip(sregs, lens)], stream_dev, 32, a0.shape, a0.dtype, [r.ptr for r in oregs], out_dev,
                                             raise_on_error=False)
    assert rc == (ERR_STREAM if damage else OK), rc
    for i, name in enumerate(names):
        what = f"decode of item {i} ({name})"
        oregs[i].check(what); sregs[i].check(what)
        assert np.array_equal(sregs[i].get(), np.frombuffer(bytes(streams[i]), dtype=np.uint8)), f"{what}: the stream was written"
        if damage and i == damage[0]:
            assert items[i].rc == ERR_STREAM, (what, items[i].rc)
            continue
        assert items[i].rc == OK, (what, items[i].rc)
        want = _ref(oracle, name, i, iv)[1]
        assert np.array_equal(_bits(oregs[i].get().view(a0.dtype)), _bits(want)), f"{what}: the values differ from the oracle's"
        assert items[i].batched == (1 if expect_batched is None else expect_batched[i]), (what, items[i].batched)
        if items[i].batched:
            assert items[i].quant_kernel == _form(a0.shape, oregs[i].ptr if out_dev else 0), (what, items[i].quant_kernel)
    if launches is not None:
        assert st.quant_kernel_launches == launches, (names, st.quant_kernel_launches)
    return items, st


# ------------------------------------------------------------------------------------------------------------------ the groups of cases
def _column(ctx, oracle, device, dt):
    names = _five("col", dt)
    esz = 4 if dt == "f32" else 8
    for count in (1, 2, 5):
        batch = names[:count]
        ivs = {_field(_ref(oracle, n, i, 0)[0], esz, "intervals") for i, n in enumerate(batch)}
        assert count == 1 or len(ivs) > 1, f"the oracle picks one interval count ({ivs}) for all of {batch}: choose other arrays"
        for iv in (0, FIXED_INTERVALS):
            _compress(ctx, oracle, batch, device, iv, launches=1, forms=[3] * count)
            _decode(ctx, oracle, batch, device, iv, launches=1)
    items, _ = _compress(ctx, oracle, names, device, FIXED_INTERVALS, expect_batched=[1] * 5)
    assert items[3].n_unpred > COL[0] * COL[1] * COL[2] // 2                 # the M-field at 1e-6 with 256 intervals: most values verbatim
    assert _field(_ref(oracle, names[3], 3, 0)[0], esz, "intervals") > 1024  # (with the optimiser it is the batch's fallback item: asserted per item above)


def g_column_f32(ctx, oracle, device):
    _column(ctx, oracle, device, "f32")


def g_column_f64(ctx, oracle, device):
    _column(ctx, oracle, device, "f64")


def g_mixed_forms(ctx, oracle, device):
    """the column shape with the middle array 4 bytes past a 16-byte boundary: forms 3, 5, 3 -- two sweep launches"""
    names = ["s@0/col/f32", "noisy/col/f32", "special/col/f32"]
    for iv in (0, FIXED_INTERVALS):
        _compress(ctx, oracle, names, device, iv, offs=[0, 4, 0], forms=[3, 5, 3], launches=2)
    items, _ = _decode(ctx, oracle, names, device, offs=[0, 4, 0], launches=2)
    assert [it.quant_kernel for it in items] == [3, 5, 3]


def g_box_forms(ctx, oracle, device):
    for dt, esz in (("f32", 4), ("f64", 8)):
        names = [f"s@0/box/{dt}", f"s@5/box/{dt}", f"tight/box/{dt}"]
        for offs, forms, launches in (([0, 0, 0], [4, 4, 4], 1), ([0, esz, 16], [4, 5, 4], 2), ([esz, 3 * esz, esz], [5, 5, 5], 1)):
            _compress(ctx, oracle, names, device, 0, offs=offs, forms=forms, launches=launches)
            _compress(ctx, oracle, names, device, FIXED_INTERVALS, offs=offs, forms=forms, launches=launches)
            _decode(ctx, oracle, names, device, offs=offs, launches=launches)


def g_fallback(ctx, oracle, device):
    # more than 1024 intervals after the optimiser: that array through the single call, its batch-mates stay batched
    names = ["s@0/col/f32", "noise/col/f32", "tight/col/f32"]
    assert _field(_ref(oracle, names[1], 1, 0)[0], 4, "intervals") > 1024
    _compress(ctx, oracle, names, device, 0, expect_batched=[1, 0, 1])
    _decode(ctx, oracle, names, device)                                      # (the look-up-table decoder takes any interval count)
    # a constant array: a one-symbol book -- batched by the compress launches (the fast packer takes it), the single call in the decode
    names = ["s@0/box/f32", "constant/box/f32", "special/box/f32"]
    _compress(ctx, oracle, names, device, 0)
    _decode(ctx, oracle, names, device, expect_batched=[1, 0, 1])
    # boxes of 210 points: every array through the single call
    names = ["s@0/odd/f64", "tight/odd/f64"]
    _compress(ctx, oracle, names, device, 0, expect_batched=[0, 0])
    _decode(ctx, oracle, names, device, expect_batched=[0, 0])


def g_host_and_output_kinds(ctx, oracle, device):
    names = ["s@0/col/f32", "m/col/f32", "noise/col/f32"]
    for out_dev in (False, True):
        _compress(ctx, oracle, names, device, 0, data_dev=False, out_dev=out_dev, expect_batched=[1, 0, 0], forms=[3, 3, 3])
        _compress(ctx, oracle, names, device, 0, offs=[0, 4, 8], data_dev=False, out_dev=out_dev, expect_batched=[1, 0, 0], forms=[3, 3, 3])    # (staged at aligned places)
    _compress(ctx, oracle, names, device, 0, data_dev=True, out_dev=True, expect_batched=[1, 0, 0])
    for stream_dev, out_dev in ((False, True), (True, False), (False, False)):
        _decode(ctx, oracle, names, device, stream_dev=stream_dev, out_dev=out_dev, stream_off=3)
    _decode(ctx, oracle, ["s@0/box/f64", "special/box/f64"], device, stream_dev=False, out_dev=False, offs=[8, 0])


def g_damage(ctx, oracle, device):
    names = ["s@0/col/f32", "m/col/f32", "special/col/f32"]
    for how in ("truncated", "count", "moved"):
        for stream_dev in (True, False):
            _decode(ctx, oracle, names, device, stream_dev=stream_dev, damage=(1, how))
    _decode(ctx, oracle, ["s@0/box/f64", "special/box/f64", "tight/box/f64"], device, damage=(1, "count"))


def g_arguments(ctx, oracle, device):
    a, eb = _array("s@0/box/f32")
    s, _ = _ref(oracle, "s@0/box/f32", 0, 0)
    src = ptr_cases.carve(a.nbytes, 0, device=device).put(a)
    mis = ptr_cases.carve(a.nbytes, 2, device=device).put(a)
    out = ptr_cases.carve(a.nbytes, 0, device=device)
    mout = ptr_cases.carve(a.nbytes, 2, device=device)
    sr = ptr_cases.carve(len(s), 1, device=device).put(s)
    regs = (src, mis, out, mout, sr)
    before = [r.get() for r in regs]
    metas = [_meta(0), _meta(1)]
    for ptrs, ms in (([], []), ([src.ptr, None], metas), ([src.ptr, mis.ptr], metas)):
        assert ctx.compress_omp_batch(ptrs, True, a.shape, a.dtype, [eb] * len(ptrs), THREADS, ms, raise_on_error=False)[0] == ERR_ARG
    assert ctx.compress_omp_batch([src.ptr], True, a.shape, a.dtype, [eb], THREADS, metas[:1], out_on_device=2, raise_on_error=False)[0] == ERR_UNSUP
    for streams, outs in (([], []), ([(sr.ptr, len(s)), (None, len(s))], [out.ptr, out.ptr]), ([(sr.ptr, len(s))], [None]), ([(sr.ptr, len(s))], [mout.ptr])):
        assert ctx.decompress_omp_batch(streams, True, 32, a.shape, a.dtype, outs, True, raise_on_error=False)[0] == ERR_ARG
    for r, b in zip(regs, before):
        assert np.array_equal(r.get(), b), "a refused call wrote"
        r.check("refused calls")


def _c_api(L, oracle, device):
    """SZ_hip_compress_openmp_batch / SZ_hip_decompress_openmp_batch against per-array calls of SZ_compress_{float,double}_3D_MDQ_openmp and
    decompressDataSeries_{float,double}_3D_openmp of the same library under the same configuration"""
    from sz_amd import api
    saved = api._lib
    api._lib = api._bind(L)
    sz = ctypes.c_size_t
    L.SZ_compress_float_3D_MDQ_openmp.restype = ctypes.c_void_p
    L.SZ_compress_float_3D_MDQ_openmp.argtypes = [ctypes.c_void_p, sz, sz, sz, ctypes.c_float, ctypes.POINTER(sz)]
    L.SZ_compress_double_3D_MDQ_openmp.restype = ctypes.c_void_p
    L.SZ_compress_double_3D_MDQ_openmp.argtypes = [ctypes.c_void_p, sz, sz, sz, ctypes.c_double, ctypes.POINTER(sz)]
    L.decompressDataSeries_float_3D_openmp.argtypes = [ctypes.POINTER(ctypes.c_void_p), sz, sz, sz, ctypes.c_void_p]
    L.decompressDataSeries_double_3D_openmp.argtypes = [ctypes.POINTER(ctypes.c_void_p), sz, sz, sz, ctypes.c_void_p]
    assert L.SZ_Init(os.path.join(ROOT, "tests", "golden", "sz_speed.config").encode()) == 0
    try:
        L.SZ_hip_set_omp_threads(THREADS)
        for dt in ("f32", "f64"):
            names = [f"s@0/col/{dt}", f"noisy/col/{dt}", f"special/col/{dt}"]
            arrs = [_array(n) for n in names]
            a0 = arrs[0][0]
            single = getattr(L, "SZ_compress_float_3D_MDQ_openmp" if dt == "f32" else "SZ_compress_double_3D_MDQ_openmp")
            inverse = getattr(L, "decompressDataSeries_float_3D_openmp" if dt == "f32" else "decompressDataSeries_double_3D_openmp")
            want, dec = [], []
            for a, eb in arrs:
                n = sz(0)
                p = single(a.ctypes.data, *a.shape, eb, ctypes.byref(n))
                assert p
                want.append(ctypes.string_at(p, n.value)); L.free(p)
                o = ctypes.c_void_p()
                buf = ctypes.create_string_buffer(want[-1][32:], len(want[-1]) - 32)
                inverse(ctypes.byref(o), *a.shape, buf)
                assert o.value
                dec.append(np.ctypeslib.as_array(ctypes.cast(o, ctypes.POINTER(ctypes.c_float if dt == "f32" else ctypes.c_double)), shape=(a.size,)).copy()); L.free(o)
                assert want[-1][32:] == oracle.omp_compress(a, eb, THREADS, want[-1][:32])[32:]
            for on_device in (False, True):
                regs = [ptr_cases.carve(a.nbytes, 0, pad=256, device=device and on_device).put(a) for a, _ in arrs]
                got = api.SZ_hip_compress_openmp_batch([r.ptr for r in regs], on_device, a0.shape, a0.dtype, [eb for _, eb in arrs])
                assert got == want, (dt, on_device)
                fill = np.empty(a0.size, dtype=a0.dtype); fill.view(np.uint32 if dt == "f32" else np.uint64)[:] = SENTINEL[a0.dtype.itemsize]
                outs = [ptr_cases.carve(a0.nbytes, 0, pad=256, device=device and on_device).put(fill) for _ in arrs]
                api.SZ_hip_decompress_openmp_batch(got, [r.ptr for r in outs], on_device, a0.shape, a0.dtype)
                for i, r in enumerate(outs):
                    assert np.array_equal(_bits(r.get().view(a0.dtype)), _bits(dec[i])), (dt, on_device, i)
                    r.check(f"C API decode {dt} {i}"); regs[i].check(f"C API compress {dt} {i}")
            with pytest.raises(api.SZError):                                  # a damaged stream: SZ_NSCS
                api.SZ_hip_decompress_openmp_batch([want[0], want[1][:-5], want[2]], [r.ptr for r in outs], on_device, a0.shape, a0.dtype)
    finally:
        L.SZ_hip_set_omp_threads(0)
        L.SZ_Finalize()
        api._lib = saved


GROUPS = [g_column_f32, g_column_f64, g_mixed_forms, g_box_forms, g_fallback, g_host_and_output_kinds, g_damage, g_arguments]
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
def test_batch_on_cpu_shim(oracle, shim_ctx, group):
    group(shim_ctx, oracle, False)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_hip_batch(oracle, hip_ctx, group):
    group(hip_ctx, oracle, True)


def test_batch_c_api_on_cpu_shim(oracle, built):
    import sim_lib
    _c_api(ctypes.CDLL(sim_lib.shim_path()), oracle, False)


@pytest.mark.gpu
def test_hip_batch_c_api(oracle, built):
    from sz_amd import api
    _c_api(ctypes.CDLL(api.lib_path()), oracle, True)


@pytest.mark.gpu
def test_hip_batch_of_64_cubes(oracle, hip_ctx):
    """64 arrays of 64^3 float32, thread_num 8 (boxes of 32^3), ABS 1e-4, both directions, all in the shared launches"""
    names = [f"s@{3 * i}/c64/f32" for i in range(64)]
    items, st = _compress(hip_ctx, oracle, names, True, 0, launches=1, forms=[3] * 64)
    assert all(it.batched == 1 for it in items) and st.n_blocks == 64 * 8
    items, st = _decode(hip_ctx, oracle, names, True, launches=1)
    assert all(it.batched == 1 for it in items)
