"""Arrays of DIFFERENT shapes in one call (include/szhip.h: szhip_compress_omp_batch_shapes, szhip_decompress_omp_batch_shapes).

The bar is that of tests/test_omp_batch.py, per item and with no tolerance: blob[offset_i, offset_i + size_i) is byte for byte oracle.omp_compress of array i alone with
ITS shape, thread_num, bound and parameter bytes; the batched decode writes into out_i bit for bit oracle.omp_decompress of stream i, and every other byte of every
allocation stays what it was (guarded regions, tests/ptr_cases.py); inputs are never written.  The checker is the oracle on each array alone, never the code under test.
What keeps a loop over single calls from passing: items[i].batched follows the documented rule per item, and stats.quant_kernel_launches is at most the number of
distinct (sweep form, box c0 x c1 x c2) among the batched items -- and the same when every item of the batch is given a second time.

The items (shape / thread_num -> boxes), the smallest at which the per-item geometry can still go wrong:
  c2    (4, 32, 32) / 2      2 boxes of 2 x 32 x 32, column form: ONE workgroup beside larger items -- the surplus workgroups of its row of the grid return
  c8    (8, 64, 64) / 8      8 of 4 x 32 x 32, column form: the same-shape tests' COL
  c64   (16, 128, 128) / 64  64 of 4 x 32 x 32, column form: 32 workgroups in the launch of the 1-workgroup item
  b8    (16, 16, 16) / 8     8^3 boxes, form 4, a face of 64 rows: the same-shape tests' BOX
  b48   (8, 24, 16) / 8      4 x 12 x 8, form 4, a face of 48 rows: a second block size and LDS size among the box forms
  s6    (12, 12, 12) / 8     6^3 = 216 points, form 5, a face of 36 rows: the value-by-value form
  p210  (12, 10, 14) / 8     boxes of 210 points: no multiple of 8 -- fallback of that item alone
  e1    (1, 16, 64) / 1      an extent of 1 in dim 0: fallback of that item alone in the compress call (the sampler's walk); the decode batches it
  o105  (3, 5, 7) / 1        105 values, fallback; stands IN FRONT of batched items: an odd length must not shift the next item's work arrays off their boundary
(The grid of thread_num 2 is 2 x 1 x 1 and does not divide an extent of 1 in dim 0, so the single call refuses (1, 16, 64) / 2: that shape is the REFUSED item of
g_refused_item below -- its rc alone, the others proceed -- and the extent-1 fallback is pinned with thread_num 1.)
Every item has its own content, bound and 32 parameter bytes; every batched kind occurs with two contents.  The compress groups run with the interval optimiser, so that
the items end with different interval counts, trees and header lengths (asserted from the oracle's streams), and with 256 fixed intervals.  The same groups run on the
CPU shim (tests/sim; its "device" memory is host memory) and, under -m gpu, through the built library."""
import ctypes
import os

import numpy as np
import pytest

import ptr_cases
from test_omp_batch import FIXED_INTERVALS, SENTINEL, _bits, _field, _meta, _params, _special

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUP, ERR_STREAM = 0, -2, -3, -4
KINDS = {"c2": ((4, 32, 32), 2), "c8": ((8, 64, 64), 8), "c64": ((16, 128, 128), 64), "b8": ((16, 16, 16), 8), "b48": ((8, 24, 16), 8), "s6": ((12, 12, 12), 8),
         "p210": ((12, 10, 14), 8), "e1": ((1, 16, 64), 1), "o105": ((3, 5, 7), 1), "c8t1": ((8, 64, 64), 1), "refused": ((1, 16, 64), 2)}
# group (a): a large item in front of a small one and the reverse, the odd-length fallback in front of batched items, two contents of every batched kind
NINE = ["o105/a", "c64/a", "c2/a", "b8/a", "e1/a", "c8/a", "b48/a", "p210/a", "s6/a", "c2/b", "s6/b", "c8/b", "b48/b", "b8/16"]
_ARR = {}
_REF = {}            # (item name, dtype, place in the batch, intervals) -> (stream, decoded array): the oracle's, computed once, never changed


def grid(shape, threads):
    """omp_box_grid of include/szhip.h's container: (boxes along each dim, points of a box along each dim), or None when the grid does not divide the shape"""
    order = threads.bit_length() - 1
    bb = order // 3
    nx, ny = [(1 << bb, 1 << bb), (1 << (bb + 1), 1 << bb), (1 << (bb + 1), 1 << (bb + 1))][order % 3]
    nz = threads // (nx * ny)
    if shape[0] % nx or shape[1] % ny or shape[2] % nz:
        return None
    return (nx, ny, nz), (shape[0] // nx, shape[1] // ny, shape[2] // nz)


def form(shape, threads, ptr):
    """the documented sweep form of an item at address ptr: 3 boxes with 32 x 32 faces at 16 bytes, 4 rows of a multiple of four values at 16 bytes, else 5"""
    (nx, ny, nz), c = grid(shape, threads)
    if c[1] == 32 and c[2] == 32 and (nx * ny * nz) % 2 == 0 and ptr % 16 == 0:
        return 3
    return 4 if c[2] % 4 == 0 and shape[2] % 4 == 0 and ptr % 16 == 0 else 5


def shared(shape, threads, compress):
    """the per-item rule of the header: boxes of a multiple of 8 points; the compress call also wants extents above 1 in dim 0 and dim 1"""
    _, c = grid(shape, threads)
    return (c[0] * c[1] * c[2]) % 8 == 0 and (not compress or (shape[0] > 1 and shape[1] > 1))


def array(name, dt):
    """`kind/content` -> (values, bound): content a an S-field slice at 1e-3, b another slice at a 10 x tighter bound, with zeros of both signs, a NaN, an infinity and
    values far outside the quantiser's range where the array is large enough to hold them"""
    key = (name, dt)
    if key not in _ARR:
        from sz_amd.fields import s_field
        kind, content = name.split("/")
        shape = KINDS[kind][0]
        dtype = np.float32 if dt == "f32" else np.float64
        if content == "a":
            a, eb = s_field(*shape, dtype), 1e-3
        elif content == "b":
            a, eb = (_special(shape, dtype) if np.prod(shape) > 1000 else s_field(*shape, dtype, z0=16)), 1e-4
        else:
            a, eb = s_field(*shape, dtype, z0=int(content)), 1e-3
        a = np.ascontiguousarray(a); a.setflags(write=False)
        _ARR[key] = (a, eb)
    return _ARR[key]


def ref(oracle, name, dt, i, iv):
    key = (name, dt, i, iv)
    if key not in _REF:
        a, eb = array(name, dt)
        p = oracle.default_params(); p.quantization_intervals = iv
        s = oracle.omp_compress(a, eb, KINDS[name.split("/")[0]][1], _meta(i), p)
        dec = oracle.omp_decompress(s, 32, a.shape, a.dtype)
        dec.setflags(write=False)
        _REF[key] = (s, dec)
    return _REF[key]


def n_unpred(stream, esz, boxes):
    at = 32 + 4 + esz + 12 + _field(stream, esz, "tree_bytes")
    return int(np.frombuffer(stream[at:at + 4 * boxes], dtype=np.uint32).sum())


def most_launches(batch, forms):
    """the bound of the header: distinct (form, box extents) among the batched items"""
    return len({(f, grid(*KINDS[n.split("/")[0]])[1]) for n, f in zip(batch, forms) if f})


def compress(ctx, oracle, batch, device, iv, dt="f32", offs=None, data_dev=True, out_dev=False):
    """one call on the items `batch`, item i `offs[i]` bytes behind a 256-byte boundary; everything the bar asks, per item.  Returns (items, stats, streams)"""
    arrs = [array(n, dt) for n in batch]
    kinds = [KINDS[n.split("/")[0]] for n in batch]
    esz = arrs[0][0].dtype.itemsize
    offs = offs or [0] * len(batch)
    regs = [ptr_cases.carve(a.nbytes, off, pad=256, device=device and data_dev).put(a) for (a, _), off in zip(arrs, offs)]
    rc, blob, size, items, st = ctx.compress_omp_batch_shapes([r.ptr for r in regs], data_dev, [s + (t,) for s, t in kinds], arrs[0][0].dtype, [eb for _, eb in arrs],
                                                              [_meta(i) for i in range(len(batch))], _params(iv), out_dev)
    assert rc == OK
    if out_dev:
        blob = ctx.debug_fetch(13, size, np.uint8).tobytes()                 # (the context's blob of the last batch)
    end, forms, streams = 0, [], []
    for i, name in enumerate(batch):
        what = f"item {i} ({name} {dt}), intervals {iv}"
        want, _ = ref(oracle, name, dt, i, iv)
        it, (shape, threads) = items[i], kinds[i]
        assert it.rc == OK, what
        assert it.offset >= end and it.offset % 64 == 0 and it.offset + it.size <= size, (what, it.offset, it.size, size)
        end = it.offset + it.size
        got = blob[it.offset:it.offset + it.size]
        assert it.size == len(want) and got == want, f"{what}: the stream differs from the oracle's stream of the array alone ({it.size} / {len(want)} bytes)"
        assert it.intervals == _field(want, esz, "intervals") and (iv == 0 or it.intervals == iv), what
        assert it.n_unpred == n_unpred(want, esz, threads), what
        # the documented rule, per item: its own geometry, and (from the oracle's stream) at most 1024 intervals
        want_batched = 1 if shared(shape, threads, True) and it.intervals <= 1024 else 0
        assert it.batched == want_batched, (what, it.batched)
        forms.append(form(shape, threads, regs[i].ptr if data_dev else 0) if want_batched else 0)
        if want_batched:
            assert it.quant_kernel == forms[i], (what, it.quant_kernel, forms[i])
        assert np.array_equal(regs[i].get(), _bits(arrs[i][0]).view(np.uint8)), f"{what}: the input was written"
        regs[i].check(what)
        streams.append(got)
    assert 1 <= st.quant_kernel_launches <= most_launches(batch, forms) or not any(forms), (batch, forms, st.quant_kernel_launches)
    return items, st, streams


def decode(ctx, oracle, batch, device, iv=0, dt="f32", offs=None, stream_dev=True, out_dev=True, stream_off=1, damage=()):
    """one decode of the oracle's streams of `batch`; damage: (item, how) pairs -- those streams are damaged and must fail alone"""
    arrs = [array(n, dt) for n in batch]
    kinds = [KINDS[n.split("/")[0]] for n in batch]
    esz = arrs[0][0].dtype.itemsize
    offs = offs or [0] * len(batch)
    streams = [bytearray(ref(oracle, n, dt, i, iv)[0]) for i, n in enumerate(batch)]
    lens = [len(s) for s in streams]
    for k, how in damage:
        if how == "truncated":
            lens[k] -= 5
        else:                                                                # one entry of the verbatim-count table raised by one: only the device can tell
            at = 32 + 4 + esz + 12 + _field(bytes(streams[k]), esz, "tree_bytes")
            streams[k][at:at + 4] = (int.from_bytes(streams[k][at:at + 4], "little") + 1).to_bytes(4, "little")
    sregs = [ptr_cases.carve(len(s), stream_off, pad=256, device=device and stream_dev).put(bytes(s)) for s in streams]
    oregs = []
    for (a, _), off in zip(arrs, offs):
        before = np.empty(a.size, dtype=a.dtype)
        before.view(np.uint32 if esz == 4 else np.uint64)[:] = SENTINEL[esz]
        oregs.append(ptr_cases.carve(a.nbytes, off, pad=256, device=device and out_dev).put(before))
    rc, items, st = ctx.decompress_omp_batch_shapes([(r.ptr, n) for r, n in zip(sregs, lens)], stream_dev, 32, [s for s, _ in kinds], arrs[0][0].dtype,
                                                    [r.ptr for r in oregs], out_dev, raise_on_error=False)
    assert rc == (ERR_STREAM if damage else OK), rc
    bad, forms = {k for k, _ in damage}, []
    for i, name in enumerate(batch):
        what = f"decode of item {i} ({name} {dt})"
        shape, threads = kinds[i]
        oregs[i].check(what); sregs[i].check(what)
        assert np.array_equal(sregs[i].get(), np.frombuffer(bytes(streams[i]), dtype=np.uint8)), f"{what}: the stream was written"
        if i in bad:
            assert items[i].rc == ERR_STREAM, (what, items[i].rc)
            forms.append(0)
            continue
        assert items[i].rc == OK, (what, items[i].rc)
        want = ref(oracle, name, dt, i, iv)[1]
        assert np.array_equal(_bits(oregs[i].get().view(arrs[i][0].dtype)), _bits(want)), f"{what}: the values differ from the oracle's"
        want_batched = 1 if shared(shape, threads, False) else 0               # (a stream is batched when the grid of ITS thread_num divides ITS shape)
        assert items[i].batched == want_batched, (what, items[i].batched)
        forms.append(form(shape, threads, oregs[i].ptr if out_dev else 0) if want_batched else 0)
        if want_batched:
            assert items[i].quant_kernel == forms[i], (what, items[i].quant_kernel, forms[i])
    assert st.quant_kernel_launches <= most_launches(batch, forms), (batch, forms, st.quant_kernel_launches)
    return items, st


# ------------------------------------------------------------------------------------------------------------------ the groups of cases
def g_all_kinds(ctx, oracle, device):
    """(a): all nine kinds interleaved, compress and decode"""
    ivs = {_field(ref(oracle, n, "f32", i, 0)[0], 4, "intervals") for i, n in enumerate(NINE) if shared(*KINDS[n.split("/")[0]], True)}
    hdr = {_field(ref(oracle, n, "f32", i, 0)[0], 4, "tree_bytes") for i, n in enumerate(NINE)}
    assert len(ivs) > 1 and len(hdr) > 2, f"the oracle picks one interval count ({ivs}) or one tree ({hdr}) for all items: choose other arrays"
    for iv in (0, FIXED_INTERVALS):
        items, st, _ = compress(ctx, oracle, NINE, device, iv)
        assert [it.batched for it in items] == [0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1]
        assert [it.quant_kernel for it in items if it.batched] == [3, 3, 4, 3, 4, 5, 3, 5, 3, 4, 4]
        assert st.quant_kernel_launches <= 4                                 # one column launch, b8, b48, s6
    items, st = decode(ctx, oracle, NINE, device)
    assert [it.batched for it in items] == [0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
    assert st.quant_kernel_launches <= 5                                     # one column launch, b8, b48, e1's 1 x 16 x 64, s6


def g_twice_over(ctx, oracle, device):
    """(a): the sweep launches do not grow with the number of items -- the batch of all kinds, and the same batch with every item given a second time"""
    batch = [n for n in NINE if not n.startswith("c64")]                     # (every kind of (form, box) of the nine; the largest item adds none)
    _, once, _ = compress(ctx, oracle, batch, device, 0)
    _, twice, _ = compress(ctx, oracle, batch + batch, device, 0)
    assert twice.quant_kernel_launches == once.quant_kernel_launches, (once.quant_kernel_launches, twice.quant_kernel_launches)
    _, once = decode(ctx, oracle, batch, device)
    _, twice = decode(ctx, oracle, batch + batch, device)
    assert twice.quant_kernel_launches == once.quant_kernel_launches, (once.quant_kernel_launches, twice.quant_kernel_launches)


def g_off_boundary_and_f64(ctx, oracle, device):
    """(b): every column-form base 4 bytes off a 16-byte boundary (form 5 where it lies; float64: 8 bytes off), and float64 (without the largest item)"""
    offs = [4 if n.startswith("c") else 0 for n in NINE]
    items, _, _ = compress(ctx, oracle, NINE, device, 0, offs=offs)
    assert [it.quant_kernel for it in items if it.batched] == [5, 5, 4, 5, 4, 5, 5, 5, 5, 4, 4]
    items, _ = decode(ctx, oracle, NINE, device, offs=offs)
    assert 3 not in [it.quant_kernel for it in items if it.batched]
    small = [n for n in NINE if not n.startswith("c64")]
    offs = [8 if n.startswith("c") else 0 for n in small]
    for iv in (0, FIXED_INTERVALS):
        items, _, _ = compress(ctx, oracle, small, device, iv, dt="f64", offs=offs)
        assert [it.quant_kernel for it in items if it.batched] == [5, 4, 5, 4, 5, 5, 5, 5, 4, 4]
    decode(ctx, oracle, small, device, dt="f64", offs=offs)
    items, _, _ = compress(ctx, oracle, small, device, 0, dt="f64")
    assert [it.quant_kernel for it in items if it.batched] == [3, 4, 3, 4, 5, 3, 5, 3, 4, 4]
    decode(ctx, oracle, small, device, dt="f64")


def g_host_and_output_kinds(ctx, oracle, device):
    """(c): host arrays in (staged one behind the other at their own lengths), host blob and device blob out; the decode's four pointer-kind combinations"""
    batch = ["o105/a", "c8/a", "c2/a", "b48/a", "p210/a", "s6/a", "c2/b"]
    for out_dev in (False, True):
        compress(ctx, oracle, batch, device, 0, offs=[0, 4, 8, 0, 4, 8, 12], data_dev=False, out_dev=out_dev)
    compress(ctx, oracle, batch, device, 0, data_dev=True, out_dev=True)
    for stream_dev, out_dev in ((False, True), (True, False), (False, False), (True, True)):
        decode(ctx, oracle, batch, device, stream_dev=stream_dev, out_dev=out_dev, stream_off=3)
    decode(ctx, oracle, batch, device, dt="f64", stream_dev=False, out_dev=False, offs=[8, 0, 8, 0, 8, 0, 8])


def g_damage(ctx, oracle, device):
    """(d): one damaged stream, one truncated stream and one stream with another thread_num among good ones: the others decode exactly"""
    batch = ["c8/a", "b48/a", "c8t1/a", "c2/a", "s6/a", "b8/a", "c8/b"]      # (c8t1: the shape of c8 in ONE box of 8 x 64 x 64 -- its own grid, form 4)
    for stream_dev in (True, False):
        items, _ = decode(ctx, oracle, batch, device, stream_dev=stream_dev, damage=((1, "count"), (5, "truncated")))
        assert items[2].batched == 1 and items[2].quant_kernel == 4
    decode(ctx, oracle, batch, device, dt="f64", damage=((0, "count"),))


def g_every_shape_once(ctx, oracle, device):
    """(e): a batch in which every shape occurs once (a kind with a single member still runs in the shared launches), and a batch of one item"""
    once = ["c2/a", "c8/a", "b8/a", "b48/a", "s6/a", "p210/a", "e1/a", "o105/a"]
    items, st, _ = compress(ctx, oracle, once, device, 0)
    assert [it.batched for it in items] == [1, 1, 1, 1, 1, 0, 0, 0] and st.quant_kernel_launches == 4
    decode(ctx, oracle, once, device)
    for name in ("c2/a", "s6/b", "o105/a"):
        compress(ctx, oracle, [name], device, 0)
        decode(ctx, oracle, [name], device)


def g_refused_item(ctx, oracle, device):
    """an item whose shape the single call refuses (the grid of thread_num 2 does not divide (1, 16, 64)) gets that rc; the rest proceed"""
    batch = ["c2/a", "refused/a", "b48/a"]
    arrs = [array(n, "f32") for n in batch]
    regs = [ptr_cases.carve(a.nbytes, 0, pad=256, device=device).put(a) for a, _ in arrs]
    shapes = [KINDS[n.split("/")[0]][0] + (KINDS[n.split("/")[0]][1],) for n in batch]
    rc, blob, size, items, st = ctx.compress_omp_batch_shapes([r.ptr for r in regs], True, shapes, np.float32, [eb for _, eb in arrs], [_meta(i) for i in range(3)], _params(0),
                                                              raise_on_error=False)
    assert rc == ERR_UNSUP and items[1].rc == ERR_UNSUP and items[1].size == 0
    for i in (0, 2):
        assert items[i].rc == OK and items[i].batched == 1
        assert blob[items[i].offset:items[i].offset + items[i].size] == ref(oracle, batch[i], "f32", i, 0)[0]
    for r in regs:
        r.check("refused item")


def g_arguments(ctx, oracle, device):
    """(f): the refusals, before anything is launched or written"""
    a, eb = array("b8/a", "f32")
    s, _ = ref(oracle, "b8/a", "f32", 0, 0)
    shp = KINDS["b8"][0] + (8,)
    src = ptr_cases.carve(a.nbytes, 0, device=device).put(a)
    mis = ptr_cases.carve(a.nbytes, 2, device=device).put(a)
    out = ptr_cases.carve(a.nbytes, 0, device=device)
    mout = ptr_cases.carve(a.nbytes, 2, device=device)
    sr = ptr_cases.carve(len(s), 1, device=device).put(s)
    regs = (src, mis, out, mout, sr)
    before = [r.get() for r in regs]
    metas = [_meta(0), _meta(1)]
    for ptrs, shapes, bounds in (([], [], []), ([src.ptr, src.ptr], None, [eb, eb]), ([src.ptr, None], [shp, shp], [eb, eb]), ([src.ptr, mis.ptr], [shp, shp], [eb, eb]),
                                 ([src.ptr, src.ptr], [shp, shp], [eb, 0.0]), ([src.ptr, src.ptr], [shp, shp], [eb, -1.0]), ([src.ptr, src.ptr], [shp, (0, 16, 16, 8)], [eb, eb]),
                                 ([src.ptr, src.ptr], [shp, (16, 16, 16, 0)], [eb, eb])):
        assert ctx.compress_omp_batch_shapes(ptrs, True, shapes, a.dtype, bounds, metas[:len(ptrs)], raise_on_error=False)[0] == ERR_ARG, (ptrs, shapes, bounds)
    assert ctx.compress_omp_batch_shapes([src.ptr], True, [shp], a.dtype, [eb], metas[:1], out_on_device=2, raise_on_error=False)[0] == ERR_UNSUP
    for streams, outs, shapes in (([], [], []), ([(sr.ptr, len(s))], [out.ptr], None), ([(sr.ptr, len(s)), (None, len(s))], [out.ptr, out.ptr], [shp, shp]),
                                  ([(sr.ptr, len(s))], [None], [shp]), ([(sr.ptr, len(s))], [mout.ptr], [shp]), ([(sr.ptr, len(s))], [out.ptr], [(16, 0, 16)])):
        assert ctx.decompress_omp_batch_shapes(streams, True, 32, shapes, a.dtype, outs, True, raise_on_error=False)[0] == ERR_ARG, (streams, shapes)
    for r, b in zip(regs, before):
        assert np.array_equal(r.get(), b), "a refused call wrote"
        r.check("refused calls")
    # more than 65535 items: 65 536 arrays of (2, 2, 2) / 1, every one of them allocated (2 MiB)
    many = 65536
    tiny = ptr_cases.carve(many * 32, 0, device=device).put(np.zeros(many * 8, dtype=np.float32))
    rc = ctx.compress_omp_batch_shapes([tiny.ptr + 32 * i for i in range(many)], True, [(2, 2, 2, 1)] * many, np.float32, [1e-3] * many, [_meta(0)] * many, raise_on_error=False)[0]
    assert rc == ERR_UNSUP
    tiny.check("65536 items")


def g_box_total(ctx, oracle, device):
    """(f), on the CPU shim only: more than 2^22 boxes in all -- 65 arrays of (64, 32, 32) in 65 536 boxes of one point each, every array allocated (16 MiB)"""
    n = 65
    whole = ptr_cases.carve(n * 65536 * 4, 0, device=device).put(np.zeros(n * 65536, dtype=np.float32))
    rc = ctx.compress_omp_batch_shapes([whole.ptr + 65536 * 4 * i for i in range(n)], True, [(64, 32, 32, 65536)] * n, np.float32, [1e-3] * n, [_meta(0)] * n, raise_on_error=False)[0]
    assert rc == ERR_UNSUP
    whole.check("2^22 boxes")


def g_same_shape_call(ctx, oracle, device):
    """(g): the same-shape call and the new call on the same equal-shape batch give identical blobs"""
    for kind in ("c8", "b48", "s6"):
        shape, threads = KINDS[kind]
        names = [f"{kind}/a", f"{kind}/b", f"{kind}/7"]
        arrs = [array(n, "f32") for n in names]
        regs = [ptr_cases.carve(a.nbytes, 0, pad=256, device=device).put(a) for a, _ in arrs]
        metas = [_meta(i) for i in range(3)]
        for iv in (0, FIXED_INTERVALS):
            old = ctx.compress_omp_batch([r.ptr for r in regs], True, shape, np.float32, [eb for _, eb in arrs], threads, metas, _params(iv))
            new = ctx.compress_omp_batch_shapes([r.ptr for r in regs], True, [shape + (threads,)] * 3, np.float32, [eb for _, eb in arrs], metas, _params(iv))
            assert old[0] == new[0] == OK and old[2] == new[2]
            for i in range(3):
                o, n = old[3][i], new[3][i]
                assert (o.offset, o.size, o.intervals, o.n_unpred, o.quant_kernel, o.batched) == (n.offset, n.size, n.intervals, n.n_unpred, n.quant_kernel, n.batched)
                assert old[1][o.offset:o.offset + o.size] == new[1][n.offset:n.offset + n.size] == ref(oracle, names[i], "f32", i, iv)[0]
            assert old[4].quant_kernel_launches == new[4].quant_kernel_launches == 1


def g_minmax_lens(ctx, oracle, device):
    """szhip_minmax_batch_lens: lengths 1 .. 70 001 in one call, bases at every element offset from a 16-byte boundary, NaN and zeros of both signs inside;
    against numpy with the NaNs skipped and against szhip_minmax of each array"""
    lens = [1, 3, 4, 5, 1023, 4096, 70001]
    rng = np.random.default_rng(5)
    for dtype in (np.float32, np.float64):
        esz = np.dtype(dtype).itemsize
        for shift in range(16 // esz):
            arrs = []
            for k, n in enumerate(lens):
                a = (rng.standard_normal(n) * 10 ** (k - 3)).astype(dtype)
                if n > 4:
                    a[1] = np.nan; a[2] = -0.0; a[n - 1] = 0.0; a[n // 2] = np.nan
                arrs.append(a)
            arrs.append(np.array([np.nan, -0.0, 0.0, np.nan, -0.0], dtype=dtype))      # (its range is -0 .. +0 in the ordering: the signs are checked below)
            regs = [ptr_cases.carve(a.nbytes, ((shift + k) % (16 // esz)) * esz, pad=256, device=device).put(a) for k, a in enumerate(arrs)]
            rc, pairs, st = ctx.minmax_batch_lens([r.ptr for r in regs], True, [a.size for a in arrs], dtype)
            assert rc == OK and st.quant_kernel_launches == 1
            for k, (a, r) in enumerate(zip(arrs, regs)):
                lo, hi = pairs[k]
                with np.errstate(all="ignore"):
                    assert lo == float(np.nanmin(a)) and hi == float(np.nanmax(a)), (dtype, shift, k, lo, hi)
                one = ctx.minmax(r.ptr, True, a.size, dtype)
                assert np.array([lo, hi]).tobytes() == np.array(one[:2], dtype=np.float64).tobytes(), (dtype, shift, k, (lo, hi), one)
                r.check("minmax_batch_lens")
            rc, pairs, _ = ctx.minmax_batch_lens([a.ctypes.data for a in arrs], False, [a.size for a in arrs], dtype)      # host arrays, staged at their own lengths
            for k, a in enumerate(arrs):
                with np.errstate(all="ignore"):
                    assert pairs[k] == (float(np.nanmin(a)), float(np.nanmax(a)))
    a = np.zeros(8, dtype=np.float32)
    assert ctx.minmax_batch_lens([a.ctypes.data], False, [0], np.float32, raise_on_error=False)[0] == ERR_ARG
    assert ctx.minmax_batch_lens([], False, [], np.float32, raise_on_error=False)[0] == ERR_ARG


GROUPS = [g_all_kinds, g_twice_over, g_off_boundary_and_f64, g_host_and_output_kinds, g_damage, g_every_shape_once, g_refused_item, g_arguments, g_same_shape_call, g_minmax_lens]
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


@pytest.mark.parametrize("group", GROUPS + [g_box_total], ids=IDS + ["box_total"])
def test_batch_shapes_on_cpu_shim(oracle, shim_ctx, group):
    group(shim_ctx, oracle, False)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_hip_batch_shapes(oracle, hip_ctx, group):
    group(hip_ctx, oracle, True)
