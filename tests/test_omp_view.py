"""Views: a sub-box of a larger array compressed from and decoded into where it lies (include/szhip.h: szhip_compress_omp_view, szhip_decompress_omp_view,
szhip_pack_view, szhip_scatter_view).

The bar, with no tolerance: a stream made from a view is byte for byte oracle.omp_compress of a contiguous copy of the sub-box; decoding into a view writes bit
for bit oracle.omp_decompress -- NaN payloads and signed zeros included -- into the sub-box, and every other byte of the parent and of the guards around it stays
what it was; an input view is never written.  The checker is the oracle on the contiguous copy, never the code under test.

A compress case runs twice: with the interval optimiser (quantization_intervals = 0: the strided sampler) and with a fixed count.  The parent's halo holds 1e30:
a sampler or a predictor that reads one element outside the sub-box changes the interval count or the stream.  A decode case pre-fills the parent with a NaN
bit pattern that no decoded value has.  The same groups run on the CPU shim (tests/sim; its "device" memory is host memory) and, under -m gpu, through the built
library; one larger group runs on the GPU only."""
import ctypes

import numpy as np
import pytest

import ptr_cases

META = bytes(range(1, 33))
HALO = 1e30
SENTINEL = {4: 0x7FC0DEAD, 8: 0x7FF8DEAD0000BEEF}
FIXED_INTERVALS = 256
_REF = {}            # (case, intervals) -> (stream, decoded array): the oracle's, computed once, never changed
_SUB = {}


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _grid(thread_num):
    """the box grid of thread_num (sz/src/sz_omp.c:88-117)"""
    order = thread_num.bit_length() - 1
    bb = order // 3
    nx, ny = [(1 << bb, 1 << bb), (2 << bb, 1 << bb), (2 << bb, 2 << bb)][order % 3]
    return nx, ny, thread_num // (nx * ny)


def _special(shape, dtype):
    """zeros of both signs, a NaN, an infinity, values far outside the quantiser's range, a constant stretch (as tests/test_omp_region.py)"""
    from sz_amd.fields import s_field
    d = s_field(*shape, np.dtype(dtype).type)
    f = d.ravel()
    f[3] = 0.0; f[4] = -0.0; f[5] = 1e30; f[6] = -1e30; f[40:90] = -0.0; f[100:400] = 0.25
    f[f.size // 2] = np.nan; f[f.size // 2 + 7] = np.inf
    return d


def _noisy():
    from sz_amd.fields import s_field
    mix = s_field(8, 64, 128); mix[:, :32, 32:64] = (np.random.default_rng(8).standard_normal((8, 32, 32)) * 3).astype(np.float32)
    return mix


# name -> (the sub-box's values, eb, thread_num, parent shape, lo).  A parent shape of None: `pitches` = (pitch0, pitch1, elements in front of the view) instead.
def _case(name):
    from sz_amd.fields import m_field, s_field
    f64 = np.float64
    return {
        # ---- form-selecting shapes
        "box-scalar": lambda: (s_field(16, 16, 16), 1e-3, 8, (20, 22, 25), (2, 3, 5)),                       # k_omp_box value by value: an odd pitch
        "box-vector": lambda: (s_field(16, 16, 16), 1e-3, 8, (18, 20, 24), (1, 2, 4)),                       # base, rows and planes 16-byte aligned
        "box-pitch26": lambda: (s_field(16, 16, 16), 1e-3, 8, (18, 20, 26), (1, 2, 4)),                      # pitch1 % 4 != 0: a g.vec taken from r2 fails here
        "f64-rows7": lambda: (s_field(12, 10, 14, f64), 1e-3, 8, (15, 13, 19), (2, 1, 3)),                   # boxes 6 x 5 x 7
        "rows18": lambda: (s_field(8, 8, 18), 1e-3, 4, (9, 11, 23), (1, 2, 5)),                              # unaligned code rows
        "col": lambda: (s_field(8, 64, 64), 1e-3, 8, (10, 66, 72), (1, 1, 4)),                               # boxes 4 x 32 x 32: k_omp_col
        "col-f64": lambda: (s_field(8, 64, 64, f64), 1e-5, 8, (10, 66, 72), (1, 1, 4)),
        "col-misaligned": lambda: (s_field(8, 64, 64), 1e-3, 8, (10, 66, 72), (1, 1, 3)),                    # the column shape one element off: packed by the call, same stream
        "col-misaligned-f64": lambda: (s_field(8, 64, 64, f64), 1e-5, 8, (10, 66, 72), (1, 1, 3)),
        "col-pitch0": lambda: (s_field(8, 64, 64), 1e-3, 8, None, (66 * 72 + 4, 72, 8)),                     # pitch0 no multiple of pitch1
        "degenerate": lambda: (s_field(8, 1, 66), 1e-3, 1, (10, 3, 70), (1, 1, 2)),                          # the strided k_sample_walk
        "degenerate-f64": lambda: (s_field(16, 1, 40, f64), 1e-3, 1, (18, 3, 44), (1, 1, 2)),
        "s128": lambda: (s_field(128, 128, 128), 1e-4, 64, (136, 132, 136), (4, 2, 4)),                      # GPU only: 64 boxes of 32^3
        # ---- data-content cases
        "m32": lambda: (np.ascontiguousarray(m_field(32)), 1e-6, 8, (34, 35, 36), (1, 2, 4)),                # most values verbatim
        "noisy": lambda: (_noisy(), 1e-4, 16, (9, 66, 132), (1, 1, 4)),                                      # boxes 2 x 32 x 64, four of them noise
        "special-f32": lambda: (_special((16, 16, 32), np.float32), 1e-3, 8, (18, 19, 36), (1, 2, 4)),
        "special-f64": lambda: (_special((16, 16, 32), f64), 1e-3, 8, (18, 19, 35), (1, 2, 3)),
        "col-special-f32": lambda: (_special((8, 64, 64), np.float32), 1e-3, 8, (10, 66, 72), (1, 1, 4)),
        "col-special-f64": lambda: (_special((8, 64, 64), f64), 1e-3, 8, (10, 66, 72), (1, 1, 4)),
        "constant": lambda: (np.full((16, 16, 16), 1.5, dtype=np.float32), 1e-3, 8, (18, 18, 20), (1, 1, 4)),   # one-symbol book
    }[name]()


def _sub(name):
    if name not in _SUB:
        sub, eb, threads, parent, lo = _case(name)
        sub = np.ascontiguousarray(sub); sub.setflags(write=False)
        if parent is None:
            p0, p1, lead = lo
            total = lead + (sub.shape[0] - 1) * p0 + (sub.shape[1] - 1) * p1 + sub.shape[2] + 5
        else:
            p0, p1 = parent[1] * parent[2], parent[2]
            lead = lo[0] * p0 + lo[1] * p1 + lo[2]
            total = parent[0] * p0
        _SUB[name] = (sub, eb, threads, p0, p1, lead, total)
    return _SUB[name]


def _ref(oracle, name, intervals):
    if (name, intervals) not in _REF:
        sub, eb, threads = _sub(name)[:3]
        p = oracle.default_params(); p.quantization_intervals = intervals
        s = oracle.omp_compress(sub, eb, threads, META, p)
        dec = oracle.omp_decompress(s, len(META), sub.shape, sub.dtype)
        dec.setflags(write=False)
        _REF[(name, intervals)] = (s, dec)
    return _REF[(name, intervals)]


class Parent:
    """`total` values, every one `fill` (a value, or a bit pattern), inside a guarded region `off` bytes behind a 256-byte aligned address; the view of shape `shape`
    starts `lead` elements in, planes p0 and rows p1 elements apart."""

    def __init__(self, shape, dtype, p0, p1, lead, total, fill, off=0, device=False, values=None):
        self.shape, self.dtype, self.p0, self.p1, self.lead = shape, np.dtype(dtype), p0, p1, lead
        esz = self.dtype.itemsize
        flat = np.empty(total, dtype=dtype)
        if isinstance(fill, int):
            flat.view(np.uint32 if esz == 4 else np.uint64)[:] = fill
        else:
            flat[:] = fill
        if values is not None:
            self.window(flat)[...] = values
        self.before = flat
        self.reg = ptr_cases.carve(flat.nbytes, off, pad=256, device=device).put(flat)
        self.ptr = self.reg.ptr + lead * esz

    def window(self, flat):
        esz = self.dtype.itemsize
        return np.lib.stride_tricks.as_strided(flat[self.lead:], shape=self.shape, strides=(self.p0 * esz, self.p1 * esz, esz))

    def now(self):
        return self.reg.get().view(self.dtype)

    def unchanged(self, what):
        assert np.array_equal(_bits(self.now()), _bits(self.before)), f"{what}: the parent was written"
        self.reg.check(what)

    def holds(self, want, what):
        """the sub-box equals `want` bit for bit, every other element still holds what it held, the guards are intact"""
        got = self.now()
        assert np.array_equal(_bits(self.window(got)), _bits(want)), f"{what}: the sub-box differs from the oracle's values"
        expect = self.before.copy()
        self.window(expect)[...] = want
        bad = np.nonzero(_bits(got) != _bits(expect))[0]
        assert bad.size == 0, f"{what}: {bad.size} elements outside the sub-box were written, the first at element {int(bad[0])}"
        self.reg.check(what)


def _parent(name, fill, device, off=0, with_values=True):
    sub, eb, threads, p0, p1, lead, total = _sub(name)
    return Parent(sub.shape, sub.dtype, p0, p1, lead, total, fill, off, device, sub if with_values else None)


def _form(name, ptr):
    """stats.quant_kernel of a device view at `ptr`: 3 k_omp_col, 4 k_omp_box with 16-byte rows, 5 value by value (include/szhip.h).  A view of the column shape that
    misses the 16-byte conditions is packed into the context's aligned buffer by the call itself and takes the column form there; every other shape runs where it lies."""
    sub, eb, threads, p0, p1, lead, total = _sub(name)
    esz = sub.dtype.itemsize
    c = [n // g for n, g in zip(sub.shape, _grid(threads))]
    aligned = ptr % 16 == 0 and p1 * esz % 16 == 0 and p0 * esz % 16 == 0
    if c[1] == 32 and c[2] == 32 and threads % 2 == 0:
        return 3
    return 4 if c[2] % 4 == 0 and aligned else 5


def _params(iv):
    from sz_amd import api
    return api.szhip_params(100, 0.99, 65536, iv)


def _compress(ctx, oracle, name, device, pinned=None, ivs=(0, FIXED_INTERVALS)):
    sub, eb, threads, p0, p1, lead, total = _sub(name)
    for iv in ivs:
        par = _parent(name, HALO, device)
        want, _ = _ref(oracle, name, iv)
        got, n, st = ctx.compress_omp_view(par.ptr, True, sub.shape, (p0, p1), sub.dtype, eb, threads, META, _params(iv))
        what = f"{name}, intervals {iv}"
        assert n == len(want) and got == want, f"{what}: the stream differs from the oracle's stream of the contiguous copy ({n} / {len(want)} bytes)"
        assert st.quant_kernel == _form(name, par.ptr), (what, st.quant_kernel)
        assert pinned is None or st.quant_kernel == pinned, (what, st.quant_kernel, pinned)
        assert st.n_elements == sub.size and st.n_blocks == threads, what
        esz = sub.dtype.itemsize                                             # (the interval count the oracle chose: stream field behind thread_num and the bound)
        assert st.intervals == int.from_bytes(want[len(META) + 4 + esz:len(META) + 8 + esz], "big") and (iv == 0 or st.intervals == iv), what
        par.unchanged(what)
    return st


def _decode(ctx, oracle, name, device, pinned=None, iv=0):
    sub, eb, threads, p0, p1, lead, total = _sub(name)
    s, want = _ref(oracle, name, iv)
    par = _parent(name, SENTINEL[sub.dtype.itemsize], device, with_values=False)
    sr = ptr_cases.carve(len(s), 0, device=device).put(s)
    st = ctx.decompress_omp_view(sr.ptr, True, len(s), len(META), sub.shape, sub.dtype, par.ptr, True, (p0, p1))
    assert st.quant_kernel == _form(name, par.ptr), (name, st.quant_kernel)
    assert pinned is None or st.quant_kernel == pinned, (name, st.quant_kernel, pinned)
    par.holds(want, f"decode of {name}")
    return st


# ------------------------------------------------------------------------------------------------------------------ the groups of cases
def g_box_forms(ctx, oracle, device):
    a = _compress(ctx, oracle, "box-scalar", device, 5); _decode(ctx, oracle, "box-scalar", device, 5)
    b = _compress(ctx, oracle, "box-vector", device, 4); _decode(ctx, oracle, "box-vector", device, 4)
    c = _compress(ctx, oracle, "box-pitch26", device, 5); _decode(ctx, oracle, "box-pitch26", device, 5)
    assert _ref(oracle, "box-scalar", 0)[0] == _ref(oracle, "box-vector", 0)[0] == _ref(oracle, "box-pitch26", 0)[0]     # the same values: the same stream from every form
    assert a.intervals == b.intervals == c.intervals


def g_scalar_rows_f64(ctx, oracle, device):
    _compress(ctx, oracle, "f64-rows7", device, 5); _decode(ctx, oracle, "f64-rows7", device, 5)


def g_unaligned_code_rows(ctx, oracle, device):
    _compress(ctx, oracle, "rows18", device, 5); _decode(ctx, oracle, "rows18", device, 5)


def g_column_form(ctx, oracle, device):
    for name in ("col", "col-f64", "col-pitch0"):
        _compress(ctx, oracle, name, device, 3); _decode(ctx, oracle, name, device, 3)
    for name in ("col-misaligned", "col-misaligned-f64"):                     # never k_omp_col on the view itself: the call packs it (sentinels and halo show that it did)
        _compress(ctx, oracle, name, device, 3); _decode(ctx, oracle, name, device, 3)
    assert _ref(oracle, "col", 0)[0] == _ref(oracle, "col-misaligned", 0)[0] == _ref(oracle, "col-pitch0", 0)[0]


def g_degenerate(ctx, oracle, device):
    for name in ("degenerate", "degenerate-f64"):
        _compress(ctx, oracle, name, device); _decode(ctx, oracle, name, device)


def g_identity(ctx, oracle, device):
    """pitch1 = r2, pitch0 = r1 r2 on the array itself: stream, statistics and form are those of compress_omp / decompress_omp"""
    keys = ("n_elements", "n_blocks", "n_unpred", "intervals", "out_bytes", "quant_kernel", "quant_kernel_launches")
    for name in ("box-vector", "col", "f64-rows7"):
        sub, eb, threads = _sub(name)[:3]
        r0, r1, r2 = sub.shape
        for off in (0, sub.dtype.itemsize):
            src = ptr_cases.carve(sub.nbytes, off, device=device).put(sub)
            a, na, sa = ctx.compress_omp(src.ptr, True, sub.shape, sub.dtype, eb, threads, META)
            b, nb, sb = ctx.compress_omp_view(src.ptr, True, sub.shape, (r1 * r2, r2), sub.dtype, eb, threads, META)
            assert a == b == _ref(oracle, name, 0)[0], (name, off)
            assert [getattr(sa, k) for k in keys] == [getattr(sb, k) for k in keys], (name, off)
            sr = ptr_cases.carve(len(a), 0, device=device).put(a)
            o1, o2 = ptr_cases.carve(sub.nbytes, off, pad=64, device=device), ptr_cases.carve(sub.nbytes, off, pad=64, device=device)
            da = ctx.decompress_omp(sr.ptr, True, len(a), len(META), sub.shape, sub.dtype, o1.ptr, True)
            db = ctx.decompress_omp_view(sr.ptr, True, len(a), len(META), sub.shape, sub.dtype, o2.ptr, True, (r1 * r2, r2))
            assert np.array_equal(o1.get(), o2.get()) and np.array_equal(_bits(o2.get().view(sub.dtype)), _bits(_ref(oracle, name, 0)[1])), (name, off)
            assert [getattr(da, k) for k in keys] == [getattr(db, k) for k in keys], (name, off)
            o2.check(name)


def g_verbatim_values(ctx, oracle, device):
    st = _compress(ctx, oracle, "m32", device); _decode(ctx, oracle, "m32", device)
    assert st.n_unpred > _sub("m32")[0].size // 4                             # the encoders' reads of verbatim values and k_omp_scatter, through the pitches
    st = _compress(ctx, oracle, "noisy", device, 4); _decode(ctx, oracle, "noisy", device, 4)
    assert st.n_unpred > 4000


def g_special_values(ctx, oracle, device):
    for name in ("special-f32", "special-f64", "col-special-f32", "col-special-f64"):
        sub = _sub(name)[0]
        dec = _ref(oracle, name, 0)[1]
        assert np.isnan(dec).any() and np.isinf(dec).any() and (np.signbit(sub) & (sub == 0)).sum() >= 50, name
        _compress(ctx, oracle, name, device); _decode(ctx, oracle, name, device)
        _decode(ctx, oracle, name, device, iv=FIXED_INTERVALS)


def g_constant(ctx, oracle, device):
    """a constant sub-box in a parent of other values: the halo must not leak into the samples (the interval count) or the boxes' first values"""
    st = _compress(ctx, oracle, "constant", device, ivs=(0,)); _decode(ctx, oracle, "constant", device)
    assert st.n_unpred == 0 and st.intervals == 32                            # (every sample predicted exactly: the optimiser's floor)
    _compress(ctx, oracle, "constant", device, ivs=(FIXED_INTERVALS,))


def g_placement(ctx, oracle, device):
    """the view and the stream on the "device" and on the host, all four combinations; the base on a 16-byte boundary and one element behind one"""
    for name in ("box-vector", "col", "col-f64", "rows18"):
        sub, eb, threads, p0, p1, lead, total = _sub(name)
        want, dec = _ref(oracle, name, 0)
        esz = sub.dtype.itemsize
        for view_dev in (False, True):
            for stream_dev in (False, True):
                for off in (0, esz):
                    what = f"{name} view_dev={view_dev} stream_dev={stream_dev} off={off}"
                    par = _parent(name, HALO, device and view_dev, off)
                    got, n, st = ctx.compress_omp_view(par.ptr, view_dev, sub.shape, (p0, p1), sub.dtype, eb, threads, META, None, stream_dev)
                    if stream_dev:
                        got = ctx.debug_fetch(8, n, np.uint8).tobytes()       # (the context's stream buffer)
                    assert got == want, what
                    # (a view on the host is packed into the context's aligned buffer: the form follows the shape alone)
                    assert st.quant_kernel == (_form(name, par.ptr) if view_dev else _form(name, 0)), (what, st.quant_kernel)
                    par.unchanged(what)
                    par = _parent(name, SENTINEL[esz], device and view_dev, off, with_values=False)
                    sr = ptr_cases.carve(len(want), 0, device=device and stream_dev).put(want)
                    st = ctx.decompress_omp_view(sr.ptr, stream_dev, len(want), len(META), sub.shape, sub.dtype, par.ptr, view_dev, (p0, p1))
                    assert st.quant_kernel == (_form(name, par.ptr) if view_dev else _form(name, 0)), (what, st.quant_kernel)
                    par.holds(dec, what)


def _fetch(ctx, ptr, count, dtype, device):
    """`count` values of the context's input buffer (what pack_view returns), through the diagnostic hook"""
    return ctx.debug_fetch(12, count, dtype)


def g_refusals(ctx, oracle, device):
    import sz_amd
    name = "box-scalar"
    sub, eb, threads, p0, p1, lead, total = _sub(name)
    s, dec = _ref(oracle, name, 0)
    r0, r1, r2 = sub.shape
    for view_dev in (False, True):
        for pitches in ((p0, r2 - 1), (r1 * p1 - 1, p1)):
            par = _parent(name, HALO, device and view_dev)
            with pytest.raises(sz_amd.SZError, match="pitch"):
                ctx.compress_omp_view(par.ptr, view_dev, sub.shape, pitches, sub.dtype, eb, threads, META)
            par.unchanged(f"compress, pitches {pitches}")
            par = _parent(name, SENTINEL[4], device and view_dev, with_values=False)
            sr = ptr_cases.carve(len(s), 0, device=device and view_dev).put(s)
            with pytest.raises(sz_amd.SZError, match="pitch"):
                ctx.decompress_omp_view(sr.ptr, view_dev, len(s), len(META), sub.shape, sub.dtype, par.ptr, view_dev, pitches)
            par.unchanged(f"decode, pitches {pitches}")
            with pytest.raises(sz_amd.SZError, match="pitch"):
                ctx.pack_view(par.ptr, view_dev, sub.shape, pitches, sub.dtype)
            with pytest.raises(sz_amd.SZError, match="pitch"):
                ctx.scatter_view(sr.ptr, sub.shape, sub.dtype, par.ptr, view_dev, pitches)
            par.unchanged(f"pack / scatter, pitches {pitches}")
        par = _parent(name, HALO, device and view_dev)                        # a grid that does not divide the sub-box: 2 x 2 x 2 boxes of 15 x 16 x 16
        with pytest.raises(sz_amd.SZError, match="does not divide"):
            ctx.compress_omp_view(par.ptr, view_dev, (15, 16, 16), (p0, p1), sub.dtype, eb, threads, META)
        par.unchanged("uneven grid")
        par = _parent(name, SENTINEL[4], device and view_dev, with_values=False)
        sr = ptr_cases.carve(len(s), 0, device=device and view_dev).put(s)
        with pytest.raises(sz_amd.SZError, match="does not divide"):
            ctx.decompress_omp_view(sr.ptr, view_dev, len(s), len(META), (15, 16, 16), sub.dtype, par.ptr, view_dev, (p0, p1))
        par.unchanged("uneven grid, decode")
        for cut in (len(s) // 2, len(s) - 1):                                 # a truncated stream
            with pytest.raises(sz_amd.SZError, match="truncated"):
                ctx.decompress_omp_view(sr.ptr, view_dev, cut, len(META), sub.shape, sub.dtype, par.ptr, view_dev, (p0, p1))
            par.unchanged(f"stream cut to {cut} bytes")


# ---- pack and scatter
def _pack_scatter(ctx, device, sub, p0, p1, lead, total, two_d=False):
    """pack_view of a view (host and device) equals the contiguous copy; scatter_view of that copy into a sentinel parent writes the sub-box and nothing else"""
    shape3 = sub.shape if not two_d else (1,) + sub.shape
    abi = sub.shape if not two_d else (0,) + sub.shape
    esz = sub.dtype.itemsize
    for view_dev in (False, True):
        for off in (0, esz):
            what = f"{sub.shape} {sub.dtype} pitches ({p0}, {p1}) view_dev={view_dev} off={off}"
            par = Parent(shape3, sub.dtype, p0, p1, lead, total, HALO, off, device and view_dev, sub.reshape(shape3))
            packed = ctx.pack_view(par.ptr, view_dev, abi, (p0, p1), sub.dtype)
            assert packed % 16 == 0
            assert np.array_equal(_bits(_fetch(ctx, packed, sub.size, sub.dtype, device)), _bits(sub)), f"pack_view: {what}"
            par.unchanged(f"pack_view: {what}")
            for src_off in (0, esz):                                           # the contiguous array at a 16-byte boundary and one element behind one
                src = ptr_cases.carve(sub.nbytes, src_off, device=device).put(sub)
                par = Parent(shape3, sub.dtype, p0, p1, lead, total, SENTINEL[esz], off, device and view_dev)
                ctx.scatter_view(src.ptr, abi, sub.dtype, par.ptr, view_dev, (p0, p1))
                par.holds(sub.reshape(shape3), f"scatter_view: {what}, source at +{src_off}")
                src.check(what)


def g_pack_scatter_shapes(ctx, oracle, device):
    for name in ("box-scalar", "box-vector", "f64-rows7", "rows18", "col-pitch0", "degenerate-f64", "special-f32", "special-f64"):
        sub, eb, threads, p0, p1, lead, total = _sub(name)
        _pack_scatter(ctx, device, sub, p0, p1, lead, total)


def g_pack_scatter_rows(ctx, oracle, device):
    """rows of 1, 3, 4 and 5 values (the head and the tail of the 16-byte form), rows of two 16-byte pieces and a tail, and a 2-D view"""
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.float64):
        for r2 in (1, 3, 4, 5, 11):
            sub = rng.standard_normal((3, 5, r2)).astype(dtype)
            for p1 in (r2 + 3, r2 + 4):
                p0 = 7 * p1 + 2
                for lead in (p0 + p1 + 1, p0 + p1 + 4):
                    _pack_scatter(ctx, device, sub, p0, p1, lead, lead + 3 * p0)
        plane = rng.standard_normal((50, 60)).astype(dtype)                   # 50 x 60 inside 64 x 70
        _pack_scatter(ctx, device, plane, 0, 70, 5 * 70 + 6, 64 * 70, two_d=True)


def g_host_view_in_chunks(ctx, oracle, device):
    """host views through the threaded, chunked staging copy: with SZ_HIP_STAGE_CHUNK_KB=1 an array of 4 KiB or more is cut into 1 KiB chunks, which rows of 72 and 112
    bytes do not divide -- chunk boundaries fall inside rows"""
    import os
    saved = os.environ.get("SZ_HIP_STAGE_CHUNK_KB")
    os.environ["SZ_HIP_STAGE_CHUNK_KB"] = "1"
    try:
        for name in ("rows18", "f64-rows7"):
            sub, eb, threads, p0, p1, lead, total = _sub(name)
            assert sub.nbytes >= 4096 and 1024 % (sub.shape[2] * sub.dtype.itemsize) != 0
            want, dec = _ref(oracle, name, 0)
            par = _parent(name, HALO, False, sub.dtype.itemsize)
            got, n, _ = ctx.compress_omp_view(par.ptr, False, sub.shape, (p0, p1), sub.dtype, eb, threads, META)
            assert got == want, name
            par.unchanged(f"{name}: host view in chunks")
            par = _parent(name, SENTINEL[sub.dtype.itemsize], False, sub.dtype.itemsize, with_values=False)
            buf = ctypes.create_string_buffer(want, len(want))
            ctx.decompress_omp_view(ctypes.addressof(buf), False, len(want), len(META), sub.shape, sub.dtype, par.ptr, False, (p0, p1))
            par.holds(dec, f"{name}: decode into a host view in chunks")
            par = _parent(name, HALO, False)
            packed = ctx.pack_view(par.ptr, False, sub.shape, (p0, p1), sub.dtype)
            assert np.array_equal(_bits(_fetch(ctx, packed, sub.size, sub.dtype, device)), _bits(sub)), name
            src = ptr_cases.carve(sub.nbytes, 0, device=device).put(sub)
            par = _parent(name, SENTINEL[sub.dtype.itemsize], False, with_values=False)
            ctx.scatter_view(src.ptr, sub.shape, sub.dtype, par.ptr, False, (p0, p1))
            par.holds(sub, f"{name}: scatter into a host view in chunks")
    finally:
        if saved is None:
            del os.environ["SZ_HIP_STAGE_CHUNK_KB"]
        else:
            os.environ["SZ_HIP_STAGE_CHUNK_KB"] = saved


def g_pack_then_compress(ctx, oracle, device):
    """SZ 2.1 and SZ 1.4 streams from a view: one packing pass, then the contiguous call on the context's buffer"""
    import sz_amd
    for kind, name in (("sz21", "s14x20x36"), ("sz14", "s20x24x40")):
        c = ptr_cases.reference(oracle, name, kind)
        x, eb, ref = c["x"], c["eb"], c["ref"]
        r0, r1, r2 = x.shape
        p1, p0 = r2 + 5, (r1 + 2) * (r2 + 5) + 3
        lead = p0 + 2 * p1 + 3
        for view_dev in (False, True):
            par = Parent(x.shape, x.dtype, p0, p1, lead, lead + r0 * p0, HALO, x.dtype.itemsize, device and view_dev, x)
            packed = ctx.pack_view(par.ptr, view_dev, x.shape, (p0, p1), x.dtype)
            meta = ref[:ptr_cases.meta_len(x)]
            assert ctx.minmax(packed, True, x.size, x.dtype) == (float(x.min()), float(x.max()))
            if kind == "sz21":
                got, n, _ = ctx.compress(packed, True, x.shape, x.dtype, eb, meta)
            else:
                rng, med = sz_amd.api.sz14_range(x.min(), x.max(), x.dtype)
                got, n, _ = ctx.compress_sz14(packed, True, x.shape, x.dtype, eb, rng, med, meta)
            assert got == ref, (kind, view_dev)
            par.unchanged(f"pack_view + {kind}")


GROUPS = [g_box_forms, g_scalar_rows_f64, g_unaligned_code_rows, g_column_form, g_degenerate, g_identity, g_verbatim_values, g_special_values, g_constant,
          g_placement, g_refusals, g_pack_scatter_shapes, g_pack_scatter_rows, g_host_view_in_chunks, g_pack_then_compress]
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
def test_view_on_cpu_shim(oracle, shim_ctx, group):
    group(shim_ctx, oracle, False)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_hip_view(oracle, hip_ctx, group):
    group(hip_ctx, oracle, True)


@pytest.mark.gpu
def test_hip_view_of_128_cubed(oracle, hip_ctx):
    """64 boxes of 32^3 inside a 136 x 132 x 136 parent, the column form: one compress and one decode"""
    st = _compress(hip_ctx, oracle, "s128", True, 3, ivs=(0,))
    assert st.n_blocks == 64
    _decode(hip_ctx, oracle, "s128", True, 3)
