"""Many same-shape patches with ghost layers in one call (include/szhip.h: szhip_compress_omp_batch_view, szhip_decompress_omp_batch_view).

The bar, with no tolerance, is the union of the bars of tests/test_omp_batch.py and tests/test_omp_view.py: blob[offset_i, offset_i + size_i) is byte for byte
oracle.omp_compress of a numpy copy of sub-box i alone, with the item's own bound and parameter bytes; the batched decode writes into sub-box i bit for bit
oracle.omp_decompress of stream i and leaves every other byte of every parent -- between rows, between planes, in the ghost layers, in front, behind, in the guard
bytes round the allocation -- what it was; inputs are never written.  The checker is the oracle on each sub-box alone, never the code under test.

Every parent is a padded array: ghosts (g0, g1, g2) on each side of an interior of the common shape, pitch1 = r2 + 2 g2, pitch0 = (r1 + 2 g1) pitch1 (+ `extra0`),
filled outside the interior with garbage (NaNs among it) before a compress call and with a sentinel bit pattern before a decode.  The ghost widths are chosen for the
form they force (szhip.h): the form of every item is asserted from items[i].quant_kernel, items[i].batched, the number of sweep launches (one per form and
addressing that occurs, whatever the count) and stats.packing (the gather / scatter launches: 0 or 1).  What keeps a loop over single view calls from passing:
batched == 1 for every item the documented rule keeps, and launch counts that do not depend on the count.

The same groups run on the CPU shim (tests/sim; its "device" memory is host memory) and, under -m gpu, through the built library; one larger group runs on the GPU only."""
import ctypes

import numpy as np
import pytest

import ptr_cases
from test_omp_batch import (BOX, COL, ERR_ARG, ERR_STREAM, ERR_UNSUP, FIXED_INTERVALS, ODD, OK, SENTINEL, THREADS, _array, _bits, _field, _five, _meta, _n_unpred,
                            _params, _ref)

_LAY = {}


class Layout:
    """the interior of `shape` inside a parent with `ghosts` on each side (far_ghost = False: none behind the interior's last value -- it is the parent's last value)"""

    def __init__(self, shape, ghosts, extra0, far_ghost):
        r0, r1, r2 = shape
        g0, g1, g2 = ghosts
        self.shape = shape
        self.pitch1 = r2 + 2 * g2
        self.pitch0 = (r1 + 2 * g1) * self.pitch1 + extra0
        self.lead = g0 * self.pitch0 + g1 * self.pitch1 + g2                # elements in front of the interior's first value
        last = self.lead + (r0 - 1) * self.pitch0 + (r1 - 1) * self.pitch1 + r2
        self.total = last + (self.lead if far_ghost else 0)
        k, i, j = np.meshgrid(np.arange(r0), np.arange(r1), np.arange(r2), indexing="ij")
        self.idx = (self.lead + k * self.pitch0 + i * self.pitch1 + j).reshape(-1)
        self.outside = np.ones(self.total, dtype=bool)
        self.outside[self.idx] = False
        self.pitches = (self.pitch0, self.pitch1)


def _layout(shape, ghosts, extra0=0, far_ghost=True):
    key = (shape, ghosts, extra0, far_ghost)
    if key not in _LAY:
        _LAY[key] = Layout(shape, ghosts, extra0, far_ghost)
    return _LAY[key]


def _garbage(n, dtype, seed):
    """what stale ghost cells hold: anything, NaNs and huge values among it"""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(n) * 100).astype(dtype)
    g[rng.random(n) < 0.05] = np.nan
    g[rng.random(n) < 0.02] = 1e30
    return g


def _kind(shape, base, pitches, esz):
    """(form, gathered) of a device view by the documented rule (szhip.h), from its own base address and the common pitches"""
    c = [n // 2 for n in shape]
    aligned = base % 16 == 0 and pitches[0] * esz % 16 == 0 and pitches[1] * esz % 16 == 0
    if c[1] == 32 and c[2] == 32:
        if tuple(pitches) == (shape[1] * shape[2], shape[2]):                # the contiguous batch call: nothing is gathered
            return (3 if aligned else 5), False
        return 3, not aligned
    return (4 if c[2] % 4 == 0 and aligned else 5), False


def _check_counts(st, kinds, batched, what):
    """one sweep launch per (form, addressing) among the batched items; one gather / scatter launch when any of them is gathered"""
    kinds = [k for k, b in zip(kinds, batched) if b]
    assert st.quant_kernel_launches == len(set(kinds)), (what, st.quant_kernel_launches, kinds)
    assert st.packing == (1 if any(g for _, g in kinds) else 0), (what, st.packing, kinds)


def _compress(ctx, oracle, names, device, iv, ghosts, offs=None, extra0=0, far_ghost=True, data_dev=True, out_dev=False, want_kinds=None):
    arrs = [_array(n) for n in names]
    a0 = arrs[0][0]
    esz = a0.dtype.itemsize
    lay = _layout(a0.shape, ghosts, extra0, far_ghost)
    offs = offs or [0] * len(names)
    parents = []
    for i, (a, _) in enumerate(arrs):
        p = _garbage(lay.total, a0.dtype, 50 + i)
        p[lay.idx] = a.reshape(-1)
        parents.append(p)
    regs = [ptr_cases.carve(p.nbytes, off, pad=256, device=device and data_dev).put(p) for p, off in zip(parents, offs)]
    bases = [r.ptr + lay.lead * esz for r in regs]
    rc, blob, size, items, st = ctx.compress_omp_batch_view(bases, data_dev, a0.shape, lay.pitches, a0.dtype, [eb for _, eb in arrs], THREADS,
                                                            [_meta(i) for i in range(len(names))], _params(iv), out_dev)
    assert rc == OK
    if out_dev:
        blob = ctx.debug_fetch(13, size, np.uint8).tobytes()
    end, kinds = 0, []
    shared = a0.shape != ODD
    for i, name in enumerate(names):
        what = f"item {i} ({name}), intervals {iv}, ghosts {ghosts}"
        want, _ = _ref(oracle, name, i, iv)
        it = items[i]
        assert it.rc == OK, what
        assert it.offset >= end and it.offset % 64 == 0 and it.offset + it.size <= size, (what, it.offset, it.size, size)
        end = it.offset + it.size
        got = blob[it.offset:it.offset + it.size]
        assert it.size == len(want) and got == want, f"{what}: the stream differs from the oracle's stream of the sub-box alone ({it.size} / {len(want)} bytes)"
        assert it.intervals == _field(want, esz, "intervals") and (iv == 0 or it.intervals == iv), what
        assert it.n_unpred == _n_unpred(want, esz), what
        assert it.batched == (1 if shared and it.intervals <= 1024 else 0), (what, it.batched)
        form, gathered = _kind(a0.shape, bases[i], lay.pitches, esz) if data_dev else _kind(a0.shape, 0, (a0.shape[1] * a0.shape[2], a0.shape[2]), esz)
        assert it.quant_kernel == form, (what, it.quant_kernel, form)
        kinds.append((form, gathered))
        assert np.array_equal(regs[i].get(), parents[i].view(np.uint8)), f"{what}: the input parent was written"
        regs[i].check(what)
    _check_counts(st, kinds, [it.batched for it in items[:len(names)]], (names, ghosts, iv))
    if want_kinds is not None:
        assert kinds == want_kinds, (kinds, want_kinds)
    return items, st


def _decode(ctx, oracle, names, device, ghosts, iv=0, offs=None, extra0=0, far_ghost=True, stream_dev=True, out_dev=True, expect_batched=None, damage=None,
            want_kinds=None):
    """one batched decode of the oracle's streams into sentinel-filled parents; damage = (item, how): that stream is damaged and must fail alone"""
    arrs = [_array(n) for n in names]
    a0 = arrs[0][0]
    esz = a0.dtype.itemsize
    lay = _layout(a0.shape, ghosts, extra0, far_ghost)
    offs = offs or [0] * len(names)
    streams = [bytearray(_ref(oracle, n, i, iv)[0]) for i, n in enumerate(names)]
    lens = [len(s) for s in streams]
    if damage:
        k, how = damage
        if how == "truncated":
            lens[k] -= 5
        else:                                                                # one entry of the verbatim-count table raised by one: only the device can tell
            at = 32 + 4 + esz + 12 + _field(bytes(streams[k]), esz, "tree_bytes")
            streams[k][at:at + 4] = (int.from_bytes(streams[k][at:at + 4], "little") + 1).to_bytes(4, "little")
    sregs = [ptr_cases.carve(len(s), 1, pad=256, device=device and stream_dev).put(bytes(s)) for s in streams]
    before = np.empty(lay.total, dtype=a0.dtype)
    before.view(np.uint32 if esz == 4 else np.uint64)[:] = SENTINEL[esz]
    oregs = [ptr_cases.carve(before.nbytes, off, pad=256, device=device and out_dev).put(before) for off in offs]
    bases = [r.ptr + lay.lead * esz for r in oregs]
    rc, items, st = ctx.decompress_omp_batch_view([(r.ptr, n) for r, n in zip(sregs, lens)], stream_dev, 32, a0.shape, a0.dtype, bases, out_dev, lay.pitches,
                                                  raise_on_error=False)
    assert rc == (ERR_STREAM if damage else OK), rc
    kinds = []
    for i, name in enumerate(names):
        what = f"decode of item {i} ({name}), ghosts {ghosts}"
        kinds.append(_kind(a0.shape, bases[i], lay.pitches, esz) if out_dev else _kind(a0.shape, 0, (a0.shape[1] * a0.shape[2], a0.shape[2]), esz))
        oregs[i].check(what); sregs[i].check(what)
        assert np.array_equal(sregs[i].get(), np.frombuffer(bytes(streams[i]), dtype=np.uint8)), f"{what}: the stream was written"
        got = oregs[i].get().view(a0.dtype)
        assert np.array_equal(_bits(got[lay.outside]), _bits(before[lay.outside])), f"{what}: bytes of the parent outside the sub-box were written"
        if damage and i == damage[0]:
            assert items[i].rc == ERR_STREAM, (what, items[i].rc)
            if not out_dev:
                assert np.array_equal(_bits(got), _bits(before)), f"{what}: a damaged stream reached the host parent"
            continue
        assert items[i].rc == OK, (what, items[i].rc)
        want = _ref(oracle, name, i, iv)[1]
        assert np.array_equal(_bits(got[lay.idx]), _bits(want)), f"{what}: the values differ from the oracle's"
        assert items[i].batched == (1 if expect_batched is None else expect_batched[i]), (what, items[i].batched)
        assert items[i].quant_kernel == kinds[i][0], (what, items[i].quant_kernel, kinds[i])
    if not damage:
        _check_counts(st, kinds, [it.batched for it in items[:len(names)]], (names, ghosts))
    if want_kinds is not None:
        assert kinds == want_kinds, (kinds, want_kinds)
    return items, st


# ------------------------------------------------------------------------------------------------------------------ the groups of cases
def _counts(ctx, oracle, device, dt, ghosts, col_kind, box_kind):
    """the column shape at counts 1, 2, 5 with the optimiser and a fixed interval count, both directions; the launch counts of 2 and 5 items are equal; the box shape"""
    names = _five("col", dt)
    esz = 4 if dt == "f32" else 8
    seen = {}
    for count in (1, 2, 5):
        batch = names[:count]
        ivs = {_field(_ref(oracle, n, i, 0)[0], esz, "intervals") for i, n in enumerate(batch)}
        assert count == 1 or len(ivs) > 1, f"the oracle picks one interval count ({ivs}) for all of {batch}: choose other arrays"
        for iv in (0, FIXED_INTERVALS):
            _, st = _compress(ctx, oracle, batch, device, iv, ghosts)
            _, sd = _decode(ctx, oracle, batch, device, ghosts, iv)
            seen[(count, iv)] = (st.quant_kernel_launches, st.packing, sd.quant_kernel_launches, sd.packing)
    for iv in (0, FIXED_INTERVALS):
        assert seen[(2, iv)] == seen[(5, iv)], f"launch counts grow with the count: {seen}"
    items, _ = _compress(ctx, oracle, names, device, FIXED_INTERVALS, ghosts, want_kinds=[col_kind] * 5)
    assert items[3].n_unpred > COL[0] * COL[1] * COL[2] // 2                 # the M-field at 1e-6 with 256 intervals: most values verbatim, read through the geometry
    _decode(ctx, oracle, names, device, ghosts, FIXED_INTERVALS, want_kinds=[col_kind] * 5)
    box = [f"s@0/box/{dt}", f"s@5/box/{dt}", f"tight/box/{dt}"]
    for iv in (0, FIXED_INTERVALS):
        _compress(ctx, oracle, box, device, iv, ghosts, want_kinds=[box_kind] * 3)
    _decode(ctx, oracle, box, device, ghosts, want_kinds=[box_kind] * 3)


def g_ghosts_111_f32(ctx, oracle, device):
    """base and pitch1 both miss 16 bytes: the column shape is gathered and reports 3, the box shape runs form 5 in place"""
    _counts(ctx, oracle, device, "f32", (1, 1, 1), (3, True), (5, False))


def g_ghosts_234_f32(ctx, oracle, device):
    """everything on 16 bytes: the column form and the vector box form directly on the parent"""
    _counts(ctx, oracle, device, "f32", (2, 3, 4), (3, False), (4, False))


def g_ghosts_002_f32(ctx, oracle, device):
    """the pitches are fine, only the base is off by 8 bytes: the column shape is gathered"""
    names = _five("col", "f32")[:3]
    for iv in (0, FIXED_INTERVALS):
        _compress(ctx, oracle, names, device, iv, (0, 0, 2), want_kinds=[(3, True)] * 3)
    _decode(ctx, oracle, names, device, (0, 0, 2), want_kinds=[(3, True)] * 3)


def g_f64(ctx, oracle, device):
    for ghosts, col_kind, box_kind in (((1, 1, 1), (3, True), (5, False)), ((2, 2, 2), (3, False), (4, False))):
        col = _five("col", "f64")[:3]
        box = ["s@0/box/f64", "special/box/f64", "tight/box/f64"]
        for iv in (0, FIXED_INTERVALS):
            _compress(ctx, oracle, col, device, iv, ghosts, want_kinds=[col_kind] * 3)
            _compress(ctx, oracle, box, device, iv, ghosts, want_kinds=[box_kind] * 3)
        _decode(ctx, oracle, col, device, ghosts, want_kinds=[col_kind] * 3)
        _decode(ctx, oracle, box, device, ghosts, want_kinds=[box_kind] * 3)


def g_odd_pitch0(ctx, oracle, device):
    """pitch0 = (r1 + 2 g1) pitch1 + 5: no multiple of pitch1, and the planes leave the 16-byte grid"""
    col, box = _five("col", "f32")[:3], ["s@0/box/f32", "s@5/box/f32", "tight/box/f32"]
    for iv in (0, FIXED_INTERVALS):
        _compress(ctx, oracle, col, device, iv, (2, 3, 4), extra0=5, want_kinds=[(3, True)] * 3)
        _compress(ctx, oracle, box, device, iv, (2, 3, 4), extra0=5, want_kinds=[(5, False)] * 3)
    _decode(ctx, oracle, col, device, (2, 3, 4), extra0=5, want_kinds=[(3, True)] * 3)
    _decode(ctx, oracle, box, device, (2, 3, 4), extra0=5, want_kinds=[(5, False)] * 3)


def g_mixed_offsets(ctx, oracle, device):
    """parents 0, 4, 8 bytes behind a 256-byte boundary: one call holds items of different forms and addressing, one sweep launch for each that occurs"""
    col, box = _five("col", "f32")[:3], ["s@0/box/f32", "s@5/box/f32", "tight/box/f32"]
    for iv in (0, FIXED_INTERVALS):
        _, st = _compress(ctx, oracle, col, device, iv, (2, 3, 4), offs=[0, 4, 8], want_kinds=[(3, False), (3, True), (3, True)])
        assert st.quant_kernel_launches == 2 and st.packing == 1
        _, st = _compress(ctx, oracle, box, device, iv, (2, 3, 4), offs=[0, 4, 8], want_kinds=[(4, False), (5, False), (5, False)])
        assert st.quant_kernel_launches == 2 and st.packing == 0
    _, st = _decode(ctx, oracle, col, device, (2, 3, 4), offs=[0, 4, 8], want_kinds=[(3, False), (3, True), (3, True)])
    assert st.quant_kernel_launches == 2 and st.packing == 1
    _, st = _decode(ctx, oracle, box, device, (2, 3, 4), offs=[0, 4, 8], want_kinds=[(4, False), (5, False), (5, False)])
    assert st.quant_kernel_launches == 2 and st.packing == 0


def g_contiguous_is_the_batch_call(ctx, oracle, device):
    """pitch1 == r2 with pitch0 == r1 r2: the contiguous batch call's streams, offsets and item fields"""
    for names, offs in ((_five("col", "f32")[:3], [0, 4, 0]), (["s@0/box/f64", "special/box/f64"], [8, 0])):
        arrs = [_array(n) for n in names]
        a0 = arrs[0][0]
        regs = [ptr_cases.carve(a.nbytes, off, pad=256, device=device).put(a) for (a, _), off in zip(arrs, offs)]
        args = ([eb for _, eb in arrs], THREADS, [_meta(i) for i in range(len(names))], _params(0))
        rc1, blob1, size1, it1, st1 = ctx.compress_omp_batch([r.ptr for r in regs], True, a0.shape, a0.dtype, *args)
        rc2, blob2, size2, it2, st2 = ctx.compress_omp_batch_view([r.ptr for r in regs], True, a0.shape, (a0.shape[1] * a0.shape[2], a0.shape[2]), a0.dtype, *args)
        assert rc1 == OK and rc2 == OK and size1 == size2
        assert st1.quant_kernel_launches == st2.quant_kernel_launches and st2.packing == 0
        for i in range(len(names)):
            for f in ("offset", "size", "rc", "intervals", "n_unpred", "quant_kernel", "batched"):
                assert getattr(it1[i], f) == getattr(it2[i], f), (names[i], f)
            assert blob1[it1[i].offset:it1[i].offset + it1[i].size] == blob2[it2[i].offset:it2[i].offset + it2[i].size] == _ref(oracle, names[i], i, 0)[0]
        _decode(ctx, oracle, names, device, (0, 0, 0), offs=offs)


def g_far_end(ctx, oracle, device):
    """no ghost behind the interior: its last row ends at the parent's last byte, guard bytes behind -- the 16-byte gather and scatter must stop there"""
    for ghosts in ((1, 1, 1), (2, 3, 4)):
        for offs in ([0, 4], [8, 12]):
            names = _five("col", "f32")[:2]
            _compress(ctx, oracle, names, device, FIXED_INTERVALS, ghosts, offs=offs, far_ghost=False)
            _decode(ctx, oracle, names, device, ghosts, FIXED_INTERVALS, offs=offs, far_ghost=False)
    _compress(ctx, oracle, ["s@0/box/f64", "tight/box/f64"], device, 0, (1, 1, 1), far_ghost=False)
    _decode(ctx, oracle, ["s@0/box/f64", "tight/box/f64"], device, (1, 1, 1), far_ghost=False)


def g_fallback(ctx, oracle, device):
    # boxes of 210 points: the whole batch through single view calls
    names = ["s@0/odd/f64", "tight/odd/f64"]
    items, st = _compress(ctx, oracle, names, device, 0, (1, 1, 1))
    assert [it.batched for it in items] == [0, 0] and st.quant_kernel_launches == 0
    _decode(ctx, oracle, names, device, (1, 1, 1), expect_batched=[0, 0])
    # more than 1024 intervals after the optimiser: that item through the single view call (gathered by it), its batch-mates stay batched
    names = ["s@0/col/f32", "noise/col/f32", "tight/col/f32"]
    assert _field(_ref(oracle, names[1], 1, 0)[0], 4, "intervals") > 1024
    items, _ = _compress(ctx, oracle, names, device, 0, (1, 1, 1))
    assert [it.batched for it in items] == [1, 0, 1]
    _decode(ctx, oracle, names, device, (1, 1, 1))
    # a constant sub-box: a one-symbol book, the single view call in the decode
    names = ["s@0/box/f32", "constant/box/f32", "special/box/f32"]
    _compress(ctx, oracle, names, device, 0, (1, 1, 1))
    _decode(ctx, oracle, names, device, (1, 1, 1), expect_batched=[1, 0, 1])


def g_host_views(ctx, oracle, device):
    """parents on the host: only the rows of the sub-boxes cross the bus, staged packed at aligned places"""
    names = _five("col", "f32")[:3]
    for out_dev in (False, True):
        _compress(ctx, oracle, names, device, 0, (1, 1, 1), offs=[0, 4, 8], data_dev=False, out_dev=out_dev, want_kinds=[(3, False)] * 3)
    _compress(ctx, oracle, ["s@0/box/f64", "special/box/f64"], device, FIXED_INTERVALS, (1, 1, 1), data_dev=False, extra0=5)
    for stream_dev in (False, True):
        _decode(ctx, oracle, names, device, (1, 1, 1), offs=[0, 4, 8], stream_dev=stream_dev, out_dev=False)
    _decode(ctx, oracle, ["s@0/box/f64", "special/box/f64"], device, (1, 1, 1), extra0=5, stream_dev=False, out_dev=False)
    for how in ("truncated", "count"):                                       # of a damaged stream nothing reaches its host parent
        _decode(ctx, oracle, names, device, (1, 1, 1), out_dev=False, damage=(1, how))


def g_damage(ctx, oracle, device):
    """one damaged stream in a batch of five: SZHIP_ERR_STREAM for that item, the other four bit for bit; nothing outside any sub-box written"""
    names = _five("col", "f32")
    for ghosts in ((1, 1, 1), (2, 3, 4)):
        for how in ("truncated", "count"):
            _decode(ctx, oracle, names, device, ghosts, FIXED_INTERVALS, damage=(2, how))
    _decode(ctx, oracle, ["s@0/box/f64", "special/box/f64", "tight/box/f64"], device, (1, 1, 1), damage=(1, "count"))


def g_arguments(ctx, oracle, device):
    a, eb = _array("s@0/box/f32")
    s, _ = _ref(oracle, "s@0/box/f32", 0, 0)
    lay = _layout(a.shape, (1, 1, 1))
    parent = _garbage(lay.total, a.dtype, 1)
    parent[lay.idx] = a.reshape(-1)
    src = ptr_cases.carve(parent.nbytes, 0, device=device).put(parent)
    out = ptr_cases.carve(parent.nbytes, 0, device=device).put(parent)
    sr = ptr_cases.carve(len(s), 1, device=device).put(s)
    regs = (src, out, sr)
    before = [r.get() for r in regs]
    base, obase = src.ptr + lay.lead * 4, out.ptr + lay.lead * 4
    metas = [_meta(0), _meta(1)]
    ok, r1r2 = lay.pitches, (a.shape[1] * a.shape[2], a.shape[2])

    def comp(ptrs, pitches, bounds=None, ms=metas, **kw):
        return ctx.compress_omp_batch_view(ptrs, True, a.shape, pitches, a.dtype, bounds or [eb] * len(ptrs), THREADS, ms[:max(len(ptrs), 1)], raise_on_error=False, **kw)[0]

    def dec(streams, outs, pitches):
        return ctx.decompress_omp_batch_view(streams, True, 32, a.shape, a.dtype, outs, True, pitches, raise_on_error=False)[0]

    one = [(sr.ptr, len(s))]
    for pitches in ((ok[0], a.shape[2] - 1), (a.shape[1] * ok[1] - 1, ok[1]), (r1r2[0], r1r2[1] + 1)):      # pitch1 < r2; pitch0 < r1 pitch1 (twice)
        assert comp([base], pitches) == ERR_ARG, pitches
        assert dec(one, [obase], pitches) == ERR_ARG, pitches
    assert comp([], ok) == ERR_ARG                                           # count < 1
    assert comp([base, None], ok) == ERR_ARG                                 # a null item pointer
    assert comp([base, base + 2], ok) == ERR_ARG                             # a misaligned value pointer
    assert comp([base, base], ok, bounds=[eb, 0.0]) == ERR_ARG               # a bound that is not positive
    assert comp([base, base], ok, bounds=[eb, -1.0]) == ERR_ARG
    assert comp([base], ok, out_on_device=2) == ERR_UNSUP                    # a caller's buffer
    assert dec([], [], ok) == ERR_ARG
    assert dec(one + [(None, len(s))], [obase, obase], ok) == ERR_ARG
    assert dec(one, [None], ok) == ERR_ARG
    assert dec(one, [obase + 2], ok) == ERR_ARG
    for r, b in zip(regs, before):
        assert np.array_equal(r.get(), b), "a refused call wrote"
        r.check("refused calls")


GROUPS = [g_ghosts_111_f32, g_ghosts_234_f32, g_ghosts_002_f32, g_f64, g_odd_pitch0, g_mixed_offsets, g_contiguous_is_the_batch_call, g_far_end, g_fallback,
          g_host_views, g_damage, g_arguments]
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
def test_batch_view_on_cpu_shim(oracle, shim_ctx, group):
    group(shim_ctx, oracle, False)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_hip_batch_view(oracle, hip_ctx, group):
    group(hip_ctx, oracle, True)


@pytest.mark.gpu
def test_hip_batch_view_of_40_patches(oracle, hip_ctx):
    """40 patches of the column shape, float32, ghosts (1, 1, 1) -- all gathered by one launch -- and ghosts (2, 3, 4) -- all direct --, both directions"""
    names = [f"s@{3 * i}/col/f32" for i in range(40)]
    for ghosts, kind in (((1, 1, 1), (3, True)), ((2, 3, 4), (3, False))):
        items, st = _compress(hip_ctx, oracle, names, True, 0, ghosts, want_kinds=[kind] * 40)
        assert all(it.batched == 1 for it in items) and st.n_blocks == 40 * 8 and st.quant_kernel_launches == 1
        items, st = _decode(hip_ctx, oracle, names, True, ghosts, want_kinds=[kind] * 40)
        assert all(it.batched == 1 for it in items) and st.quant_kernel_launches == 1
