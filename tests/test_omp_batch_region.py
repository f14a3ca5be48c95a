"""Sub-boxes of many OpenMP-container streams in one call: szhip_decompress_omp_batch_region (include/szhip.h).

The bar: every destination sub-box holds bit for bit oracle.omp_decompress(stream)[lo0:hi0, lo1:hi1, lo2:hi2] -- NaN payloads and signed zeros included --, for streams
made by oracle.omp_compress, and every other byte of every destination allocation keeps its fill.  No tolerance.  The same groups of cases run on the CPU shim
(tests/sim) and, under -m gpu, through the built library; one group of patches with ghost layers runs on the GPU only.  The streams and small arrays are those of
tests/test_omp_region.py."""
import ctypes

import numpy as np
import pytest

import ptr_cases
from test_omp_region import META, _STREAMS, _bits, _covered, _crop, _grid, _stream, _tables, hip_ctx, shim_ctx  # noqa: F401  (the two fixtures)

ERR_ARG, ERR_STREAM = -2, -4
F32 = ("box", "rows18", "col", "m32", "noisy", "special-f32", "constant", "wide-codes-one-box", "wide-codes-big-box")
F64 = ("f64-rows7", "col-f64", "special-f64")
# the items the shared launches do not cover, by the rules of szhip.h: a one-symbol book; boxes of 6 x 5 x 7 = 210 points, no multiple of 8; a covered payload that
# does not fit a workgroup's LDS beside the look-up table (g_mixed_batch works the sum out from the stream's tables, for this stream and for wide-codes-one-box)
FALLBACK = ("constant", "f64-rows7", "wide-codes-big-box")
_stream_of_region_tests = _stream


def _stream(oracle, name):
    """the streams of tests/test_omp_region.py and one more: ONE box of 32 x 32 x 64 values with a wide book, whose payload is beyond the decoder's LDS"""
    if name == "wide-codes-big-box" and name not in _STREAMS:
        d = (np.random.default_rng(6).standard_normal((32, 32, 64)) * 50).astype(np.float32)
        p = oracle.default_params(); p.quantization_intervals = 65536
        s = oracle.omp_compress(d, 1e-3, 1, META, p)
        want = oracle.omp_decompress(s, len(META), d.shape, d.dtype)
        want.setflags(write=False)
        _STREAMS[name] = (d, s, want)
    return _stream_of_region_tests(oracle, name)


def _decoder_lds(oracle, name):
    """bytes of LDS the look-up-table decoder needs for the largest box of a stream: the payload's stage (szh_omp.h: omp_hdec_lut_body) and the 20 KiB look-up
    table; a node table above 13 KiB stays in global memory"""
    d, s, _ = _stream(oracle, name)
    nb, _, off_sizes, _ = _tables(s, d.dtype)
    largest = int(np.frombuffer(s, dtype=np.uint64, count=nb, offset=off_sizes).max())
    words = (((largest + 30 + 15) // 16 * 16 + 16) + 16) // 4
    nodes = int.from_bytes(s[len(META) + 12 + d.dtype.itemsize:len(META) + 16 + d.dtype.itemsize], "big")
    return ((words + (words >> 5)) * 4 + 15) // 16 * 16 + 1024 * 20 + (nodes * 8 if nodes * 8 <= 13 * 1024 else 0)


class Item:
    """one item of a call: the region [lo, hi) of stream `name` into a destination `off` bytes behind a 256-byte boundary, contiguous or with `pitches`"""

    def __init__(self, name, lo, hi, pitches=None, off=0):
        self.name, self.lo, self.hi, self.pitches, self.off = name, tuple(lo), tuple(hi), pitches, off
        self.ext = tuple(h - l for l, h in zip(lo, hi))
        self.p0, self.p1 = pitches if pitches else (self.ext[1] * self.ext[2], self.ext[2])

    def span(self):
        """values from the destination's first to its last"""
        return (self.ext[0] - 1) * self.p0 + (self.ext[1] - 1) * self.p1 + self.ext[2]

    def mask(self):
        """which values of the span belong to the sub-box"""
        m = np.zeros(self.span(), dtype=bool)
        k, i = np.meshgrid(np.arange(self.ext[0]), np.arange(self.ext[1]), indexing="ij")
        for s in (k * self.p0 + i * self.p1).ravel():
            m[s:s + self.ext[2]] = True
        return m


def _call(ctx, oracle, items, stream_dev=False, out_dev=False, device=False, streams=None, raise_on_error=True, dests=None):
    """one call over `items` -> (rc, c_items, c_regions, stats, dests).  Items of one name share ONE copy of the stream (and so its header work).
    streams: name -> bytes, where a test wants other bytes than the oracle's."""
    dtype = _stream(oracle, items[0].name)[0].dtype
    esz = dtype.itemsize
    placed = {}
    for it in items:
        if it.name not in placed:
            s = (streams or {}).get(it.name) or _stream(oracle, it.name)[1]
            placed[it.name] = (ptr_cases.carve(len(s), 0, device=device and stream_dev).put(s), len(s))
    if dests is None:
        dests = [ptr_cases.carve(it.span() * esz, it.off, pad=64, device=device and out_dev) for it in items]
    rc, c_items, c_regions, st = ctx.decompress_omp_batch_region(
        [(placed[it.name][0].ptr, placed[it.name][1]) for it in items], stream_dev, len(META), [_stream(oracle, it.name)[0].shape for it in items], dtype,
        [(it.lo, it.hi, it.pitches) for it in items], [d.ptr for d in dests], out_dev, raise_on_error=raise_on_error)
    return rc, c_items, c_regions, st, dests


def _untouched(dest, what):
    assert (dest.get() == ptr_cases.FILL).all(), f"{what}: the destination of an item that was not delivered was written"
    dest.check(what)


def _delivered(oracle, it, dest, what):
    """the sub-box holds the oracle's crop, every other byte of the allocation its fill"""
    d, _, want = _stream(oracle, it.name)
    got = dest.get().view(d.dtype)
    m = it.mask()
    crop = np.ascontiguousarray(_crop(want, it.lo, it.hi))
    assert np.array_equal(_bits(got[m]), _bits(crop.ravel())), f"{what}: values differ from the oracle's crop"
    assert (got[~m].view(np.uint8) == ptr_cases.FILL).all(), f"{what}: bytes between the rows or planes of the sub-box were written"
    dest.check(what)


def _check_items(oracle, items, c_items, c_regions, dests, what=""):
    first = {}
    for i, it in enumerate(items):
        w = f"{what} item {i} ({it.name} {it.lo}-{it.hi} pitches={it.pitches} off={it.off})"
        assert c_items[i].rc == 0, w
        _delivered(oracle, it, dests[i], w)
        d, s, _ = _stream(oracle, it.name)
        nb, ucount, _, _ = _tables(s, d.dtype)
        boxes = _covered(d.shape, nb, it.lo, it.hi)
        assert c_regions[i].n_boxes == len(boxes) and c_items[i].n_unpred == int(ucount[boxes].sum()), w
        assert c_items[i].batched == (0 if it.name in FALLBACK else 1), w
        assert c_regions[i].shares == first.setdefault(it.name, i), w
        if c_items[i].batched:                                 # the single region call's rule on the covered sub-grid
            grid = _grid(nb)
            col = d.shape[1] // grid[1] == 32 and d.shape[2] // grid[2] == 32 and len(boxes) % 2 == 0
            assert (c_items[i].quant_kernel == 3) == col and c_items[i].quant_kernel in (3, 4, 5), w


def _totals(oracle, items):
    n = boxes = unpred = 0
    for it in items:
        d, s, _ = _stream(oracle, it.name)
        nb, ucount, _, _ = _tables(s, d.dtype)
        b = _covered(d.shape, nb, it.lo, it.hi)
        n += int(np.prod(it.ext)); boxes += len(b); unpred += int(ucount[b].sum())
    return n, boxes, unpred


def _faces(shape, width):
    """the six faces of `width` values of an array of `shape`"""
    out = []
    for d in range(3):
        for side in (0, 1):
            lo, hi = [0, 0, 0], list(shape)
            if side == 0: hi[d] = width
            else: lo[d] = shape[d] - width
            out.append((tuple(lo), tuple(hi)))
    return out


# ------------------------------------------------------------------------------------------------------------------ the groups of cases
def _mixed_items(names):
    items = []
    if "col" in names:
        items += [Item("col", lo, hi) for lo, hi in _faces((8, 64, 64), 2)]                   # six faces, one stream
        items += [Item("col", (0, 0, 0), (8, 64, 64)), Item("col", (3, 33, 40), (4, 34, 41)),  # the whole array; one value
                  Item("col", (4, 32, 0), (8, 64, 32)),                                        # on box boundaries
                  Item("col", (1, 5, 2), (3, 30, 31), (31 * 40 + 5, 40), 4),                   # an odd covered-box count: a box form
                  Item("col", (0, 0, 20), (4, 32, 40), (32 * 24, 24))]                          # an even one: the column form
    for name in names:
        shape = {"box": (16, 16, 16), "rows18": (8, 8, 18), "m32": (32, 32, 32), "noisy": (8, 64, 128), "special-f32": (16, 16, 32), "constant": (16, 16, 16),
                 "wide-codes-one-box": (32, 32, 32), "wide-codes-big-box": (32, 32, 64), "f64-rows7": (12, 10, 14), "col-f64": (8, 64, 64), "special-f64": (16, 16, 32), "col": None}[name]
        if shape is None:
            continue
        lo = tuple(min(n - 1, k) for n, k in zip(shape, (1, 2, 3)))
        hi = tuple(max(l + 1, n - k) for l, n, k in zip(lo, shape, (2, 1, 3)))
        items += [Item(name, lo, hi), Item(name, (0, 0, 0), (9 if shape[0] > 9 else shape[0], 3, shape[2] - 1), ((3 + 1) * (shape[2] + 3) + 1, shape[2] + 3), 0)]
    items += [Item("col-f64", lo, hi) for lo, hi in (((0, 0, 20), (4, 32, 40)), ((1, 5, 2), (3, 30, 31)))] if "col-f64" in names else []
    return items


def g_mixed_batch(ctx, oracle):
    # (wide-codes-one-box: 24 264 bytes of payload, 45 584 bytes of LDS -- within a workgroup's 64 KiB, so it runs in the shared launches; the big box does not)
    assert _decoder_lds(oracle, "wide-codes-one-box") <= 64 * 1024 < _decoder_lds(oracle, "wide-codes-big-box")
    for names in (F32, F64):
        items = _mixed_items(names)
        rc, c_items, c_regions, st, dests = _call(ctx, oracle, items)
        assert rc == 0
        _check_items(oracle, items, c_items, c_regions, dests, names[0])
        assert (st.n_elements, st.n_blocks, st.n_unpred) == _totals(oracle, items)
        if names is F32:
            assert [c_regions[i].shares for i in range(6)] == [0] * 6 and st.packing == 1
            special = [it for it in items if it.name == "special-f32"]                  # (the NaN and the -0 stretch are inside what is asked for)
            want = _stream(oracle, "special-f32")[2]
            assert any(np.isnan(_crop(want, it.lo, it.hi)).any() for it in special)


def g_placement(ctx, oracle, device=False):
    """contiguous destinations and views; the base 0 and one element behind a 16-byte boundary; pitches that are multiples and non-multiples of 16 bytes; rows of
    1, 3, 4, 5, 9 float32 and 1, 2, 3 float64 values (the head and tail cases of the 16-byte pieces); stream and destination on the host and on the device"""
    for name, lens in (("box", (1, 3, 4, 5, 9)), ("special-f64", (1, 2, 3))):
        esz = _stream(oracle, name)[0].dtype.itemsize
        per16 = 16 // esz
        items = []
        for e2 in lens:
            for off in (0, esz):
                lo, hi = (1, 2, 3), (5, 7, 3 + e2)
                aligned = (e2 + per16 - 1) // per16 * per16 + per16                        # a row pitch of a multiple of 16 bytes ...
                for pitches in (None, (aligned * 6, aligned), (aligned * 5 + per16 * 2, aligned), ((aligned + 1) * 5 + 3, aligned + 1)):     # ... and one that is none
                    items.append(Item(name, lo, hi, pitches, off))
        if name == "box":                                      # fallback items beside them: the single region call from inside, a view placed behind it
            items += [Item("constant", (2, 3, 4), (15, 9, 13), (6 * 11 + 2, 11), 4), Item("constant", (0, 0, 0), (3, 3, 3)), Item("wide-codes-big-box", (5, 6, 7), (9, 29, 28), (23 * 24, 24))]
        for stream_dev in (False, True):
            for out_dev in (False, True):
                rc, c_items, c_regions, st, dests = _call(ctx, oracle, items, stream_dev, out_dev, device)
                assert rc == 0
                _check_items(oracle, items, c_items, c_regions, dests, f"{name} stream_dev={stream_dev} out_dev={out_dev}")
                assert st.packing == 1


def _payloads(oracle, name):
    d, s, _ = _stream(oracle, name)
    nb, _, off_sizes, off_pay = _tables(s, d.dtype)
    sizes = np.frombuffer(s, dtype=np.uint64, count=nb, offset=off_sizes)
    return s, sizes, off_pay + np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)


def g_errors(ctx, oracle):
    s, sizes, starts = _payloads(oracle, "box")
    bad = bytearray(s)
    bad[int(starts[5]):int(starts[5] + sizes[5])] = b"\xff" * int(sizes[5])       # box 5 = (1, 0, 1): rows 8.., columns 8.. of dim 2
    in5, in0 = Item("box", (9, 1, 9), (14, 6, 15), (7 * 9, 9)), Item("box", (1, 2, 3), (5, 7, 6), (6 * 5 + 1, 5), 4)
    other = Item("m32", (9, 9, 9), (23, 23, 23))
    items = [in0, in5, other, Item("box", (0, 0, 0), (8, 8, 8))]
    rc, c_items, c_regions, st, dests = _call(ctx, oracle, items, streams={"box": bytes(bad)}, raise_on_error=False)
    assert rc == ERR_STREAM and [c_items[i].rc for i in range(4)] == [0, ERR_STREAM, 0, 0]
    _untouched(dests[1], "a damaged payload in a covered box")
    for i in (0, 2, 3):
        _delivered(oracle, items[i], dests[i], f"beside a damaged item: item {i}")
    # damage in a box that no region touches is not noticed
    rc, c_items, c_regions, st, dests = _call(ctx, oracle, [in0, other], streams={"box": bytes(bad)})
    assert rc == 0
    _check_items(oracle, [in0, other], c_items, c_regions, dests, "damage elsewhere")
    # a truncated stream and a wrong thread_num fail per item
    seven = bytearray(s); seven[len(META):len(META) + 4] = (7).to_bytes(4, "big")
    for what, broken in (("truncated", s[:len(s) // 2]), ("thread_num 7", bytes(seven))):
        rc, c_items, c_regions, st, dests = _call(ctx, oracle, [other, in0, in5], streams={"box": broken}, raise_on_error=False)
        assert rc != 0 and c_items[0].rc == 0 and c_items[1].rc != 0 and c_items[2].rc != 0, what
        _delivered(oracle, other, dests[0], what)
        _untouched(dests[1], what); _untouched(dests[2], what)


def g_refusals(ctx, oracle):
    d, s, _ = _stream(oracle, "box")
    buf = ctypes.create_string_buffer(s, len(s))
    good = ((1, 2, 3), (5, 7, 6), None)
    outs = [np.full(4 * 5 * 3 + 8, 7.0, dtype=np.float32) for _ in range(2)]

    def call(streams=None, shapes=True, regions=(good, good), out_ptrs=None, count=2):
        streams = [(ctypes.addressof(buf), len(s))] * 2 if streams is None else streams
        out_ptrs = [o.ctypes.data for o in outs] if out_ptrs is None else out_ptrs
        rc, _, _, _ = ctx.decompress_omp_batch_region(streams[:count], False, len(META), [d.shape] * count if shapes else None, d.dtype,
                                                      list(regions)[:count] if regions is not None else None, out_ptrs[:count], False, raise_on_error=False)
        assert rc == ERR_ARG
        assert all((o == 7.0).all() for o in outs)

    call(count=0)
    call(shapes=False)
    call(regions=None)
    call(streams=[(ctypes.addressof(buf), len(s)), (None, len(s))])
    call(out_ptrs=[outs[0].ctypes.data, None])
    call(out_ptrs=[outs[0].ctypes.data, outs[1].ctypes.data + 2])                                  # misaligned
    for lo, hi in (((2, 2, 2), (2, 5, 5)), ((0, 0, 9), (1, 1, 9)), ((0, 0, 0), (17, 16, 16)), ((0, 0, 3), (16, 16, 17)), ((5, 0, 0), (4, 16, 16))):
        call(regions=(good, (lo, hi, None)))
    for pitches in ((15, 2), (14, 3), (0, 3), (15, 0)):                                            # pitch1 < e2; pitch0 < e1 * pitch1; one of the two zero
        call(regions=(good, (good[0], good[1], pitches)))


def g_launch_counts(ctx, oracle, device=False):
    items = _mixed_items(F32)
    rc1, _, _, st1, _ = _call(ctx, oracle, items, out_dev=True, device=device)
    rc2, c_items, c_regions, st2, dests = _call(ctx, oracle, items + items, out_dev=True, device=device)
    assert rc1 == 0 and rc2 == 0
    assert st2.quant_kernel_launches == st1.quant_kernel_launches > 0 and st2.packing == st1.packing == 1
    assert st2.n_blocks == 2 * st1.n_blocks and st2.n_elements == 2 * st1.n_elements
    for i, it in enumerate(items + items):
        _delivered(oracle, it, dests[i], f"given twice: item {i}")


def g_fuzz(ctx, oracle):
    rng = np.random.default_rng(23)
    names = ("box", "col", "m32")
    items = []
    for k in range(40):
        shape = _stream(oracle, names[k % 3])[0].shape
        lo = [int(rng.integers(0, n)) for n in shape]
        hi = [int(rng.integers(l + 1, n + 1)) for l, n in zip(lo, shape)]
        e = [h - l for l, h in zip(lo, hi)]
        p1 = e[2] + int(rng.integers(0, 6))
        pitches = None if k % 4 == 0 else (p1 * e[1] + int(rng.integers(0, 9)), p1)
        items.append(Item(names[k % 3], lo, hi, pitches, 4 * int(rng.integers(0, 4))))
    rc, c_items, c_regions, st, dests = _call(ctx, oracle, items)
    assert rc == 0
    _check_items(oracle, items, c_items, c_regions, dests, "fuzz")
    assert (st.n_elements, st.n_blocks, st.n_unpred) == _totals(oracle, items)


GROUPS = [g_mixed_batch, g_placement, g_errors, g_refusals, g_launch_counts, g_fuzz]
IDS = [g.__name__[2:] for g in GROUPS]


@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_batch_region_on_cpu_shim(oracle, shim_ctx, group):
    group(shim_ctx, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_hip_batch_region(oracle, hip_ctx, group):
    if group in (g_placement, g_launch_counts):
        group(hip_ctx, oracle, device=True)
    else:
        group(hip_ctx, oracle)


@pytest.mark.gpu
def test_hip_batch_region_fills_ghost_layers(oracle, hip_ctx):
    """8 patches of 64^3 float32 at thread_num 8 (boxes of 32^3), device-resident; the six faces of width 3 of every patch's neighbour into the ghost layers of its
    70^3 device parent: 48 items in one call.  Every face is the oracle's crop, every other byte of every parent is unchanged, and every item takes the form the
    rule gives it (four covered boxes with 32 x 32 faces: the column form)."""
    import torch
    from sz_amd.fields import s_field
    n, w, P = 64, 3, 70
    base = s_field(n, n, n)
    wants, streams = [], []
    for k in range(8):
        x = np.ascontiguousarray(base * np.float32(1 + 0.125 * k) + np.float32(0.01 * k))
        s = oracle.omp_compress(x, 1e-4, 8, META, oracle.default_params())
        wants.append(oracle.omp_decompress(s, len(META), x.shape, x.dtype))
        streams.append(ptr_cases.carve(len(s), 0, device=True).put(s))
    fill = np.float32(-7.5)
    parents = [torch.full((P, P, P), float(fill), dtype=torch.float32, device="cuda") for _ in range(8)]
    expect = [np.full((P, P, P), fill, dtype=np.float32) for _ in range(8)]
    torch.cuda.synchronize()
    srcs, shapes, regions, outs = [], [], [], []
    for k in range(8):
        nb = (k + 1) % 8                                                            # whose faces fill patch k's ghost layers
        for d in range(3):
            for side in (0, 1):
                lo, hi = [0, 0, 0], [n, n, n]                                        # in the neighbour: its far face for the low ghost layer, its near one for the high
                glo = [w, w, w]                                                      # in the parent
                if side == 0: lo[d], glo[d] = n - w, 0
                else: hi[d], glo[d] = w, w + n
                srcs.append((streams[nb].ptr, streams[nb].nbytes)); shapes.append((n, n, n))
                regions.append((lo, hi, (P * P, P)))
                outs.append(parents[k].data_ptr() + 4 * ((glo[0] * P + glo[1]) * P + glo[2]))
                e = [h - l for l, h in zip(lo, hi)]
                expect[k][glo[0]:glo[0] + e[0], glo[1]:glo[1] + e[1], glo[2]:glo[2] + e[2]] = wants[nb][lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    rc, c_items, c_regions, st = hip_ctx.decompress_omp_batch_region(srcs, True, len(META), shapes, np.float32, regions, outs, True)
    assert rc == 0 and st.packing == 1 and st.quant_kernel_launches == 1 and st.n_blocks == 48 * 4 and st.n_elements == 48 * w * n * n
    for i in range(48):
        assert c_items[i].rc == 0 and c_items[i].batched == 1 and c_regions[i].n_boxes == 4 and c_items[i].quant_kernel == 3, i
    assert [c_regions[i].shares for i in range(48)] == [next(j for j in range(48) if srcs[j] == srcs[i]) for i in range(48)]
    for k in range(8):
        got = parents[k].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), expect[k].view(np.uint32)), f"parent {k}: a face differs from the oracle's crop, or a byte outside the ghost layers was written"
