"""An array against its decoded copy, compared where both lie: szhip_compare / szhip_compare_view (include/szhip.h), SZ_hip_compare / SZ_hip_print_quality
(include/sz.h) and their Python mirror.  Kernels: sz_amd/csrc/szh_quality.h.

Every case runs twice: on the device (-m gpu, torch uint8 tensors) and through the HIP-on-CPU shim (tests/sim), where "device" memory is host memory.

Expected values: `reference()` below, a numpy restatement of the loop of the reference's `sz -a` report (example/sz.c:558-620): the difference and its absolute
value in the ARRAY's dtype, everything after that in float64 on exactly converted values.  Points whose ori, dec or error is a NaN are excluded and counted.
  * orderings, indices and counts must be EQUAL;
  * sums are held to the first-order bound that holds for ANY order of summation: |sum - exact| <= (n - 1) 2^-53 sum|term|, times 1.01, computed from the
    data with math.fsum (the exact sum, correctly rounded) -- never a constant;
  * the same input twice, and a view against contiguous copies of its two boxes, must give the same BYTES.

The grid rule the sizes below are chosen for (szh_quality_grid): a lane folds pieces of VW = 16 / itemsize consecutive points, a workgroup has 256 lanes and
is sized for 8 pieces per lane, so grid = clamp(ceil(n / (256 * VW * 8)), 1, 1024).  One sweep of a grid covers grid * 256 * VW points: with grid = 1 that is
1024 points of float32 and 512 of float64 (1023 / 1025, 511 / 513 lie either side); a workgroup's share ends at 8192 / 4096 points (8191 / 8193, 4095 / 4097);
70 001 and 1 000 003 points take 9 / 18 and 123 / 245 workgroups, whose slots the final workgroup merges; 1 052 673 float64 points take 258 slots, more than
the final workgroup has lanes."""
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
import ref_cases  # noqa: E402

f32, f64 = np.float32, np.float64
NO_INDEX = 2 ** 64 - 1
ERR_ARG = -2
U = 2.0 ** -53
BACKENDS = [pytest.param("gpu", marks=pytest.mark.gpu, id="on_the_gpu"), pytest.param("shim", id="on_the_cpu_shim")]


# ------------------------------------------------------------------------------------------------------------------ contexts (as tests/test_device_pointers.py)

@pytest.fixture(scope="module")
def gctx(built):
    import sz_amd
    c = sz_amd.HipContext(0)
    yield c
    c.close()


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


@pytest.fixture(params=BACKENDS)
def env(request):
    """(context, arrays live in device memory): the product library on the GPU, or the same code over the CPU shim"""
    if request.param == "gpu":
        return request.getfixturevalue("gctx"), True
    return request.getfixturevalue("sctx"), False


# ------------------------------------------------------------------------------------------------------------------ the reference's loop, restated

def _bits(a):
    return a.view(np.uint32 if a.dtype == f32 else np.uint64)


def reference(ori, dec, ab=-1.0, pb=-1.0):
    """example/sz.c:558-620 over the points that are not excluded; the terms of every sum are returned too (float64 arrays)"""
    o, d = np.ascontiguousarray(ori).reshape(-1), np.ascontiguousarray(dec).reshape(-1)
    assert o.dtype == d.dtype and o.size == d.size
    with np.errstate(all="ignore"):
        e = np.abs(d - o)                                           # in the array's dtype: `float err = fabs(data[i] - ori_data[i])`
        ex = np.isnan(o) | np.isnan(d) | np.isnan(e)
        idx = np.nonzero(~ex)[0]
        o64, d64, e64 = o[idx].astype(f64), d[idx].astype(f64), e[idx].astype(f64)
        nz = o64 != 0
        rel = np.full(idx.size, np.nan)
        rel[nz] = e64[nz] / np.abs(o64[nz])
        over_abs = e64 > ab if ab >= 0 else np.zeros(idx.size, bool)
        over_pwr = (rel > pb) if pb >= 0 else np.zeros(idx.size, bool)          # (a NaN -- a zero, or inf / inf -- is greater than nothing)
        either = np.nonzero(over_abs | over_pwr)[0]
        r = dict(n=o.size, n_excluded=int(ex.sum()), n_excluded_diff=int((ex & (_bits(o) != _bits(d))).sum()),
                 n_zero_changed=int(((o64 == 0) & (d64 != 0)).sum()), n_over_abs=int(over_abs.sum()), n_over_pwr=int(over_pwr.sum()),
                 n_over_both=int((over_abs & over_pwr).sum()), first_over_idx=int(idx[either[0]]) if either.size else NO_INDEX)
        if idx.size:
            r.update(vmin=float(o64.min()), vmax=float(o64.max()), max_abs_err=float(e64.max()), max_abs_idx=int(idx[int(np.argmax(e64))]),
                     max_pw_rel_err=float(np.fmax.reduce(rel, initial=0.0)))
        else:
            r.update(vmin=math.nan, vmax=math.nan, max_abs_err=0.0, max_abs_idx=NO_INDEX, max_pw_rel_err=0.0)
        r["terms"] = dict(sum_ori=o64, sum_dec=d64, sum_dec_sq=d64 * d64, sum_err_sq=e64 * e64)
        r["o64"], r["d64"] = o64, d64
    return r


EXACT = ("n", "n_excluded", "n_excluded_diff", "n_zero_changed", "n_over_abs", "n_over_pwr", "n_over_both", "max_abs_idx", "first_over_idx",
         "vmin", "vmax", "max_abs_err", "max_pw_rel_err")


def assert_exact(q, r, what):
    for k in EXACT:
        got, want = getattr(q, k), r[k]
        print(f"{what}: {k} = {got!r} (reference {want!r})")
        assert got == want or (isinstance(want, float) and math.isnan(want) and math.isnan(got)), f"{what}: {k} is {got!r}, the reference's loop gives {want!r}"


def sum_tolerance(terms):
    """any order of summation is within (n - 1) 2^-53 sum|term| of the exact sum, to first order; times 1.01"""
    return 1.01 * max(terms.size - 1, 0) * U * math.fsum(np.abs(terms))


def assert_sums(q, r, what, corr):
    terms = dict(r["terms"])
    if corr:
        n = q.n - q.n_excluded
        a, b = r["o64"] - q.sum_ori / n, r["d64"] - q.sum_dec / n       # the means pass 2 is given: the call's own
        terms.update(cov=a * b, var_ori=a * a, var_dec=b * b)
    for k, t in terms.items():
        exact, tol, got = math.fsum(t), sum_tolerance(t), getattr(q, k)
        print(f"{what}: {k} = {got!r}, exact {exact!r}, off by {abs(got - exact):.3e}, tolerance {tol:.3e}")
        assert abs(got - exact) <= tol, f"{what}: {k} = {got!r} is {abs(got - exact):.3e} from the exact sum {exact!r}; any summation order stays within {tol:.3e}"
    if not corr:
        assert q.cov == 0 and q.var_ori == 0 and q.var_dec == 0 and math.isnan(q.ac_eff), f"{what}: centred sums without SZHIP_Q_CORR"


def printed_by(fn):
    """what a call into the C library writes to the process's standard output"""
    import tempfile
    libc = ctypes.CDLL(None)
    sys.stdout.flush(), libc.fflush(None)
    with tempfile.TemporaryFile() as f:
        saved = os.dup(1)
        try:
            os.dup2(f.fileno(), 1)
            fn()
            libc.fflush(None)
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        f.seek(0)
        return f.read().decode()


def put(dev, a, off=0):
    return P.carve(a.nbytes, off, device=dev).put(a)


def unchanged(region, a, what):
    region.check(what)
    assert np.array_equal(region.get(), np.ascontiguousarray(a).reshape(-1).view(np.uint8)), f"{what}: an input was written"


def pair(n, dtype, seed=0):
    """an array with zeros and a copy with errors of about 1e-3, a few exact values, one zero that did not stay zero"""
    rng = np.random.default_rng(seed + n)
    o = (3.0 * rng.standard_normal(n)).astype(dtype)
    o[::17] = 0
    d = (o.astype(f64) + 1e-3 * rng.standard_normal(n)).astype(dtype)
    d[::17] = 0
    d[::5] = o[::5]
    if n > 34:
        d[34] = dtype(1e-4)
    return o, d


def run(env, o, d, ab=-1.0, pb=-1.0, corr=False, offs=(0, 0)):
    """compare on arrays placed `offs` bytes behind an aligned address; the inputs must come back untouched; returns the Quality"""
    ctx, dev = env
    ro, rd = put(dev, o, offs[0]), put(dev, d, offs[1])
    q = ctx.compare(ro.ptr, rd.ptr, True, o.size, o.dtype, ab, pb, corr=corr)
    unchanged(ro, o, "ori"), unchanged(rd, d, "dec")
    return q


# ------------------------------------------------------------------------------------------------------------------ sizes

SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1025, 4095, 4097, 8191, 8193, 70001, 1000003)
SIZE_CASES = [(n, t) for t in (f32, f64) for n in SIZES] + [(1052673, f64)]


@pytest.mark.parametrize("n,dtype", SIZE_CASES, ids=[f"{t.__name__}-{n}" for n, t in SIZE_CASES])
def test_every_field_at_every_size(env, n, dtype):
    o, d = pair(n, dtype)
    ab, pb = 2e-3, 1e-3
    q = run(env, o, d, ab, pb, corr=True)
    r = reference(o, d, ab, pb)
    what = f"{dtype.__name__} n = {n}"
    assert_exact(q, r, what)
    assert_sums(q, r, what, corr=True)
    assert run(env, o, d, ab, pb, corr=True).raw == q.raw, f"{what}: two calls on the same input differ"


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("where", ("first", "last", "twice"))
def test_where_the_largest_error_is(env, dtype, where):
    n = 70001
    o, d = pair(n, dtype, 1)
    at = {"first": (0,), "last": (n - 1,), "twice": (60000, 123)}[where]
    for i in at:
        o[i], d[i] = 1.0, 3.0
    q = run(env, o, d)
    assert_exact(q, reference(o, d), f"{dtype.__name__} maximum {where}")
    assert q.max_abs_err == 2.0 and q.max_abs_idx == min(at)


# ------------------------------------------------------------------------------------------------------------------ pointers

PTR_CASES = [(f32, 4, 12), (f32, 12, 4), (f32, 4, 0), (f64, 8, 0), (f64, 0, 8), (f64, 8, 8)]


@pytest.mark.parametrize("n", (1025, 70001))
@pytest.mark.parametrize("dtype,oo,do", PTR_CASES, ids=[f"{t.__name__}-ori{a}-dec{b}" for t, a, b in PTR_CASES])
def test_pointers_aligned_to_the_element_only(env, dtype, oo, do, n):
    o, d = pair(n, dtype, 2)
    q = run(env, o, d, 2e-3, 1e-3, corr=True, offs=(oo, do))
    r = reference(o, d, 2e-3, 1e-3)
    assert_exact(q, r, f"ori at +{oo}, dec at +{do}")
    assert_sums(q, r, f"ori at +{oo}, dec at +{do}", corr=True)
    assert q.raw == run(env, o, d, 2e-3, 1e-3, corr=True).raw, "the result depends on where the arrays lie"


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
def test_host_arrays_are_staged(env, dtype):
    ctx, dev = env
    o, d = pair(70001, dtype, 3)
    want = run(env, o, d, 2e-3, 1e-3, corr=True)
    o0, d0 = o.copy(), d.copy()
    assert ctx.compare(o.ctypes.data, d.ctypes.data, False, o.size, dtype, 2e-3, 1e-3, corr=True).raw == want.raw
    rd = put(dev, d)
    assert ctx.compare(o.ctypes.data, rd.ptr, (False, True), o.size, dtype, 2e-3, 1e-3, corr=True).raw == want.raw
    assert _bits(o).tobytes() == _bits(o0).tobytes() and _bits(d).tobytes() == _bits(d0).tobytes()


# ------------------------------------------------------------------------------------------------------------------ views

class View:
    """a box of `shape` inside a flat parent of NaNs: first value at element `base`, planes pitch0 and rows pitch1 elements apart"""

    def __init__(self, dev, box, base, pitch0, pitch1, off=0):
        r0, r1, r2 = box.shape
        self.index = base + np.add.outer(np.add.outer(np.arange(r0) * pitch0, np.arange(r1) * pitch1), np.arange(r2))
        self.parent = np.full(int(self.index.max()) + 7, np.nan, dtype=box.dtype)
        self.parent[self.index] = box
        self.region = put(dev, self.parent, off)
        self.ptr, self.pitches = self.region.ptr + base * box.itemsize, (pitch0, pitch1)


VIEW_BOXES = ((1, 1, 1), (2, 3, 5), (7, 9, 33), (16, 16, 64))


def view_layouts(r0, r1, r2, itemsize):
    """(ori base, pitch0, pitch1, byte offset), (dec ...): rows that are no multiple of four elements, pitch1 == r2, a pitch0 that is no multiple of pitch1"""
    yield (3, (r1 + 2) * (r2 + 5), r2 + 5, 0), (1, r1 * r2 + 3, r2, 0)
    yield (0, r1 * r2, r2, 0), (5, (r1 + 1) * (r2 + 3) + 1, r2 + 3, 0)
    yield (4, (r1 + 1) * (r2 + 4), r2 + 4, 0), (8, r1 * (r2 + 8), r2 + 8, 0)         # (float32 16 x 16 x 64: every row of both on a 16-byte boundary)
    yield (2, r1 * (r2 + 1), r2 + 1, itemsize), (0, r1 * r2, r2, 8)                 # (bases one element / 8 bytes behind an aligned address)


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
@pytest.mark.parametrize("shape", VIEW_BOXES, ids=["x".join(map(str, s)) for s in VIEW_BOXES])
def test_views_give_what_contiguous_copies_give(env, dtype, shape):
    ctx, dev = env
    n = int(np.prod(shape))
    o, d = pair(n, dtype, 4)
    o, d = o.reshape(shape), d.reshape(shape)
    want = run(env, o, d, 2e-3, 1e-3, corr=True)
    assert_exact(want, reference(o, d, 2e-3, 1e-3), f"box {shape}")
    assert want.n_excluded == 0
    for lo, ld in view_layouts(*shape, o.itemsize):
        vo, vd = View(dev, o, *lo), View(dev, d, *ld)
        q = ctx.compare_view(vo.ptr, vo.pitches, vd.ptr, vd.pitches, True, shape, dtype, 2e-3, 1e-3, corr=True)
        what = f"box {shape}, ori pitches {vo.pitches}, dec pitches {vd.pitches}"
        assert q.n_excluded == 0, f"{what}: {q.n_excluded} values from outside the box were read (the parents are NaN there)"
        for k in EXACT + ("sum_ori", "sum_dec", "sum_dec_sq", "sum_err_sq", "cov", "var_ori", "var_dec", "psnr", "ac_eff"):
            assert getattr(q, k) == getattr(want, k) or (math.isnan(getattr(q, k)) and math.isnan(getattr(want, k))), f"{what}: {k} is {getattr(q, k)!r}, {getattr(want, k)!r} on contiguous copies"
        assert q.raw == want.raw, what
        unchanged(vo.region, vo.parent, what), unchanged(vd.region, vd.parent, what)
    # a view on the host: its rows are staged
    (lo, ld) = next(view_layouts(*shape, o.itemsize))
    vo, vd = View(False, o, *lo), View(False, d, *ld)
    q = ctx.compare_view(vo.ptr, vo.pitches, vd.ptr, vd.pitches, False, shape, dtype, 2e-3, 1e-3, corr=True)
    assert q.raw == want.raw, f"box {shape}: host views"
    unchanged(vo.region, vo.parent, "host view"), unchanged(vd.region, vd.parent, "host view")


# ------------------------------------------------------------------------------------------------------------------ bounds

@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
def test_an_openmp_container_round_trip_holds_its_bound(env, dtype):
    from sz_amd.fields import s_field
    ctx, dev = env
    x = s_field(32, 32, 64, dtype)
    src = put(dev, x)
    stream, n, _ = ctx.compress_omp(src.ptr, True, x.shape, dtype, 1e-3, 8, P.OMP_META, out_on_device=False)
    out = put(dev, np.zeros_like(x))
    keep = ctypes.create_string_buffer(stream, len(stream))
    ctx.decompress_omp(ctypes.addressof(keep), False, len(stream), len(P.OMP_META), x.shape, dtype, out.ptr, True)
    dec = out.get().view(dtype).reshape(x.shape)
    r = reference(x, dec, 1e-3)
    q = ctx.compare(src.ptr, out.ptr, True, x.size, dtype, 1e-3)
    assert_exact(q, r, "ABS 1e-3")
    assert q.n_over_abs == 0 and q.first_over_idx == NO_INDEX and 0 < q.max_abs_err <= 1e-3
    q0 = ctx.compare(src.ptr, out.ptr, True, x.size, dtype, 0.0)
    assert_exact(q0, reference(x, dec, 0.0), "bound 0")
    assert q0.n_over_abs == int((np.abs(dec - x) > 0).sum()) > x.size // 2
    pushed = dec.copy().reshape(-1)
    at = 12345
    pushed[at] = x.reshape(-1)[at] + dtype(0.5)
    rp = put(dev, pushed)
    q1 = ctx.compare(src.ptr, rp.ptr, True, x.size, dtype, 1e-3)
    assert_exact(q1, reference(x, pushed, 1e-3), "one value pushed out")
    assert q1.n_over_abs == 1 and q1.first_over_idx == at and q1.max_abs_idx == at


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_pw_rel_round_trip_holds_its_bound(request, backend, tmp_path):
    """SZ_compress_args in mode PW_REL (tests/ref_cases.py "pwr-zeros-pos-3D-f32": 18 x 22 x 26 with zeros), checked through SZ_hip_compare on host arrays"""
    request.getfixturevalue("built" if backend == "gpu" else "shim")
    import sz_amd
    c = ref_cases.BY_NAME["pwr-zeros-pos-3D-f32"]
    x = c["data"]()
    cfg = str(tmp_path / "sz.config")
    ref_cases.write_config(cfg, c["conf"])
    assert sz_amd.SZ_Init(cfg) == 0
    try:
        dec = sz_amd.SZ_decompress(sz_amd.SZ_compress_args(x, c["mode"], c["abs"], c["rel"], c["pwr"]), x.shape, x.dtype)
        q = sz_amd.SZ_hip_compare(x, dec, pwRelBound=c["pwr"])
    finally:
        sz_amd.SZ_Finalize()
    assert_exact(q, reference(x, dec, -1.0, c["pwr"]), "PW_REL 1e-2")
    assert int((x == 0).sum()) > 100 and q.n_zero_changed == 0 and q.n_over_pwr == 0 and q.n_over_abs == 0 and 0 < q.max_pw_rel_err <= c["pwr"]


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
def test_points_over_one_bound_the_other_and_both(env, dtype):
    #                 neither  both   abs only  pw_rel only  neither (zero)  abs only (a zero: no relative error)
    o = np.array([2.0, 1.0, 1000.0, 0.001, 0.0, 0.0, 5.0], dtype=dtype)
    e = np.array([0.001, 0.5, 0.5, 0.0005, 0.0, 0.25, 0.0], dtype=dtype)
    d = (o + e).astype(dtype)
    ab, pb = 0.1, 0.01
    q = run(env, o, d, ab, pb)
    assert_exact(q, reference(o, d, ab, pb), "four combinations")
    assert (q.n_over_abs, q.n_over_pwr, q.n_over_both, q.first_over_idx, q.n_zero_changed) == (3, 2, 1, 1, 1)
    # what the combined modes read off: ABS_OR_PW_REL is violated where both are, ABS_AND_PW_REL where either is
    assert q.n_over_abs + q.n_over_pwr - q.n_over_both == 4
    only_abs, only_pwr, none = run(env, o, d, ab, -1.0), run(env, o, d, -1.0, pb), run(env, o, d)
    assert (only_abs.n_over_abs, only_abs.n_over_pwr, only_abs.n_over_both, only_abs.first_over_idx) == (3, 0, 0, 1)
    assert (only_pwr.n_over_abs, only_pwr.n_over_pwr, only_pwr.n_over_both, only_pwr.first_over_idx) == (0, 2, 0, 1)
    assert (none.n_over_abs, none.n_over_pwr, none.n_over_both, none.first_over_idx) == (0, 0, 0, NO_INDEX)


# ------------------------------------------------------------------------------------------------------------------ NaN, infinities

def _nan_with_payload(dtype, payload):
    u = np.array([(0x7fc00000 if dtype == f32 else 0x7ff8000000000000) | payload], dtype=np.uint32 if dtype == f32 else np.uint64)
    return u.view(dtype)[0]


@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
def test_nan_points_are_excluded_and_counted(env, dtype):
    o, d = pair(1025, dtype, 5)
    nan1, nan2, inf = _nan_with_payload(dtype, 1), _nan_with_payload(dtype, 2), dtype(np.inf)
    o[10] = nan1                                    # NaN in ori only
    d[20] = nan1                                    # in dec only
    o[30] = d[30] = nan1                            # in both, the same bits
    o[40], d[40] = nan1, nan2                       # in both, other bits
    o[50] = d[50] = inf                             # inf - inf is a NaN: excluded, the same bits
    o[60], d[60] = inf, -inf                        # the difference is inf: takes part
    o[1024], d[1024] = -inf, -inf
    q = run(env, o, d, 2e-3, 1e-3)
    r = reference(o, d, 2e-3, 1e-3)
    assert_exact(q, r, "NaN and inf")
    assert (q.n_excluded, q.n_excluded_diff) == (6, 3)
    assert q.max_abs_err == math.inf and q.max_abs_idx == 60 and q.vmax == math.inf
    # +inf against a finite value
    o, d = pair(257, dtype, 6)
    d[100] = inf
    q = run(env, o, d, 2e-3, 1e-3)
    assert_exact(q, reference(o, d, 2e-3, 1e-3), "+inf against a finite value")
    assert q.max_abs_err == math.inf and q.max_abs_idx == 100 and q.n_excluded == 0 and q.max_pw_rel_err == math.inf
    # nothing takes part
    o = np.full(300, nan1, dtype=dtype)
    q = run(env, o, o.copy(), 2e-3, 1e-3, corr=True)
    assert_exact(q, reference(o, o, 2e-3, 1e-3), "every point a NaN")
    assert q.n_excluded == 300 and q.n_excluded_diff == 0 and q.max_abs_idx == NO_INDEX and q.sum_ori == 0


# ------------------------------------------------------------------------------------------------------------------ sums

def test_correlation_of_a_field_whose_mean_dwarfs_its_spread(env):
    """1e6 + noise of spread 1 in float64: sum(xy) - n m1 m2 cancels (shown below); the two-pass form of sz.c:595-597 does not"""
    n = 70001
    rng = np.random.default_rng(7)
    o = 1e6 + rng.standard_normal(n)
    d = o + 0.3 * rng.standard_normal(n)
    q = run(env, o, d, corr=True)
    r = reference(o, d)
    assert_sums(q, r, "1e6 + noise", corr=True)
    m1, m2 = q.sum_ori / n, q.sum_dec / n
    a, b = o - m1, d - m2
    cov, v1, v2 = math.fsum(a * b), math.fsum(a * a), math.fsum(b * b)
    two_pass = cov / n / math.sqrt(v1 / n) / math.sqrt(v2 / n)
    # the sums' bounds carried through the quotient (relative: cov once, each variance half), and 8 roundings of the divisions and roots
    bound = 1.01 * abs(two_pass) * (sum_tolerance(a * b) / abs(cov) + 0.5 * sum_tolerance(a * a) / v1 + 0.5 * sum_tolerance(b * b) / v2 + 8 * U)
    one_pass = (float(np.dot(o, d)) - n * m1 * m2) / math.sqrt((float(np.dot(o, o)) - n * m1 * m1) * (float(np.dot(d, d)) - n * m2 * m2))
    print(f"acEff {q.ac_eff!r}, two-pass {two_pass!r}, off by {abs(q.ac_eff - two_pass):.3e}, bound {bound:.3e}; the one-pass form is off by {abs(one_pass - two_pass):.3e}")
    assert abs(q.ac_eff - two_pass) <= bound
    assert not abs(one_pass - two_pass) <= bound, "this field does not tell the two forms apart"


# ------------------------------------------------------------------------------------------------------------------ derived values, the printed report

@pytest.mark.parametrize("backend", BACKENDS)
def test_config1_report(request, backend, c1_data):
    """BASELINE config #1 (testfloat_8_8_128.dat, ABS 1e-4): PSNR 99.114337, and the `Max absolute error` line examples/sz_cli.c prints for the same run
    (tests/test_gpu_parity.py: test_config1_through_a_plain_c_caller pins that line of the tool)"""
    request.getfixturevalue("built" if backend == "gpu" else "shim")
    import sz_amd
    assert sz_amd.SZ_Init(os.path.join(ROOT, "tests", "golden", "sz_speed.config")) == 0
    try:
        stream = sz_amd.SZ_compress_args(c1_data, sz_amd.ABS, 1e-4)
        dec = sz_amd.SZ_decompress(stream, c1_data.shape, c1_data.dtype)
        q = sz_amd.SZ_hip_compare(c1_data, dec, absBound=1e-4, corr=True)
    finally:
        sz_amd.SZ_Finalize()
    assert q.n_over_abs == 0
    out = printed_by(lambda: sz_amd.SZ_hip_print_quality(q, len(stream), False))
    print(out)
    lines = out.splitlines()
    assert "Max absolute error = 0.0000999272" in lines
    assert any(ln.startswith("PSNR = 99.114337, NRMSE= ") for ln in lines)
    r = reference(c1_data, dec)
    rng = float(f32(r["vmax"]) - f32(r["vmin"]))
    assert lines[0] == "Min=%.20G, Max=%.20G, range=%.20G" % (r["vmin"], r["vmax"], rng)
    assert "Max relative error = %f" % (r["max_abs_err"] / rng) in lines and "Max pw relative error = %f" % r["max_pw_rel_err"] in lines
    assert "acEff=%f" % q.ac_eff in lines and "compressionRatio=%f" % (c1_data.nbytes / len(stream)) in lines
    assert abs(q.ac_eff - float(np.corrcoef(c1_data.reshape(-1).astype(f64), dec.reshape(-1).astype(f64))[0, 1])) < 1e-12
    assert q.range == rng and q.norm_err == math.sqrt(q.sum_err_sq) and q.mse == q.sum_err_sq / q.n and q.nrmse == math.sqrt(q.mse) / rng


# ------------------------------------------------------------------------------------------------------------------ refusals

@pytest.mark.parametrize("dtype", (f32, f64), ids=("f32", "f64"))
def test_refusals_leave_the_struct_and_the_context_alone(env, dtype):
    from sz_amd import api
    ctx, dev = env
    L = api.lib()
    o, d = pair(2 * 3 * 8, dtype, 8)
    ro, rd = put(dev, o), put(dev, d)
    code, half = (0 if dtype == f32 else 1), o.itemsize // 2
    q = api.szhip_quality()
    ctypes.memset(ctypes.byref(q), 0x5A, ctypes.sizeof(q))
    before = bytes(q)

    def flat(op, dp, n):
        return L.szhip_compare(ctx._h, code, op, int(dev), dp, int(dev), n, 1e-3, 1e-3, 1, ctypes.byref(q))

    def box(op, opitch, dp, dpitch, shape):
        return L.szhip_compare_view(ctx._h, code, op, int(dev), opitch[0], opitch[1], dp, int(dev), dpitch[0], dpitch[1], *shape, 1e-3, 1e-3, 1, ctypes.byref(q))

    ok = (24, 8)
    refused = {"ori is null": flat(None, rd.ptr, o.size), "dec is null": flat(ro.ptr, None, o.size), "n == 0": flat(ro.ptr, rd.ptr, 0),
               "ori off its element": flat(ro.ptr + half, rd.ptr, o.size - 1), "dec off its element": flat(ro.ptr, rd.ptr + half, o.size - 1),
               "an empty box": box(ro.ptr, ok, rd.ptr, ok, (2, 0, 8)), "no planes": box(ro.ptr, ok, rd.ptr, ok, (0, 3, 8)),
               "pitch1 < r2 (ori)": box(ro.ptr, (24, 7), rd.ptr, ok, (2, 3, 8)), "pitch1 < r2 (dec)": box(ro.ptr, ok, rd.ptr, (24, 7), (2, 3, 8)),
               "pitch0 < r1 * pitch1 (ori)": box(ro.ptr, (23, 8), rd.ptr, ok, (2, 3, 8)), "pitch0 < r1 * pitch1 (dec)": box(ro.ptr, ok, rd.ptr, (23, 8), (2, 3, 8)),
               "a view off its element": box(ro.ptr + half, ok, rd.ptr, ok, (1, 3, 8)),
               "no struct": L.szhip_compare(ctx._h, code, ro.ptr, int(dev), rd.ptr, int(dev), o.size, 1e-3, 1e-3, 1, None)}
    for what, rc in refused.items():
        assert rc == ERR_ARG, f"{what}: returned {rc}"
    assert bytes(q) == before, "a refused call wrote the struct"
    assert box(ro.ptr, ok, rd.ptr, ok, (2, 3, 8)) == 0 and bytes(q) != before
    assert_exact(ctx.compare(ro.ptr, rd.ptr, True, o.size, dtype, 1e-3, 1e-3), reference(o, d, 1e-3, 1e-3), "after the refusals")
    # the reference-style calls: SZ_NSCS and a printed reason
    q2 = api.szhip_quality()
    ctypes.memset(ctypes.byref(q2), 0x5A, ctypes.sizeof(q2))
    dt = api.SZ_FLOAT if dtype == f32 else api.SZ_DOUBLE
    for fn, op, dp in ((L.SZ_hip_compare, o.ctypes.data, d.ctypes.data), (L.SZ_hip_compare_device, ro.ptr, rd.ptr)):
        assert fn(dt, None, dp, 0, 0, 0, 0, o.size, 1e-3, 1e-3, 0, ctypes.byref(q2)) == api.SZ_NSCS
        assert fn(dt, op, None, 0, 0, 0, 0, o.size, 1e-3, 1e-3, 0, ctypes.byref(q2)) == api.SZ_NSCS
        assert fn(dt, op, dp, 0, 0, 0, 0, 0, 1e-3, 1e-3, 0, ctypes.byref(q2)) == api.SZ_NSCS
        assert fn(dt, op + half, dp, 0, 0, 0, 0, o.size - 1, 1e-3, 1e-3, 0, ctypes.byref(q2)) == api.SZ_NSCS
        assert bytes(q2) == before
    if dev:
        import sz_amd
        assert sz_amd.SZ_hip_compare_device(ro.ptr, rd.ptr, (2, 3, 8), dtype, 1e-3, 1e-3).raw == ctx.compare(ro.ptr, rd.ptr, True, o.size, dtype, 1e-3, 1e-3).raw
