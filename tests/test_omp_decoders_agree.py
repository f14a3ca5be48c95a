"""The four decoders of the OpenMP container refuse the same damaged streams with the same code: szhip_decompress_omp, szhip_decompress_omp_batch,
szhip_decompress_omp_batch_shapes and szhip_decompress_omp_batch_region read a stream's header, tree and per-box tables by ONE copy of the container's rules
(sz_amd/csrc/szhip_omprules.inc: omp_stream), and this file pins what that means.

One oracle stream per small shape of tests/test_omp_batch.py (COL: k_omp_col boxes, BOX: 8^3 boxes, ODD: boxes of 210 points), float32 and float64, thread_num 8,
takes the damage tests/test_container_errors.py applies to such streams: a cut at every header field, the header fields the decoder refuses, a count of verbatim values
above the box size, a payload size that runs past the end.  Every damaged stream goes to (a) the single call, and as item 1 of three -- the other two good -- to (b) the
same-shape batch, (c) the different-shapes batch and (d) the region batch with a region inside one box; all of the damage lies in the header or the tables, which the
region call reads whole.  Asserted: the damaged item's rc is the same nonzero code in all four; the good items decode bit for bit to the oracle's arrays (the region
items to the oracle's array cropped); the damaged item's output keeps its sentinel fill.  The checker is the oracle and the sentinel, never another path of the code
under test.  Streams are handed over as host and as device pointers; the same cases run on the CPU shim and, under -m gpu, through the built library (every listed
damage is refused by the host-side walk before a kernel reads the stream)."""
import numpy as np
import pytest

import ptr_cases
from test_omp_batch import BOX, COL, ERR_STREAM, ODD, OK, SENTINEL, THREADS, _array, _bits, _ref, hip_ctx, shim_ctx  # noqa: F401  (the two fixtures)

SHAPES = {"col": COL, "box": BOX, "odd": ODD}
KINDS = ("s@0", "tight", "special")          # items 0, 1, 2 of every batch; item 1 is the damaged one
BAD = 1
BODY = 32


def _damages(stream, esz, shape):
    """[(what, damaged stream bytes)] of one good stream behind 32 parameter bytes"""
    b = BODY
    nb = int.from_bytes(stream[b:b + 4], "big"); tree_bytes = int.from_bytes(stream[b + 8 + esz:b + 12 + esz], "big")
    fixed = b + 4 + esz + 12
    off_ucount = fixed + tree_bytes; off_first = off_ucount + nb * 4; off_unpred = off_first + nb * esz
    E = int(np.frombuffer(stream[off_ucount:off_first], dtype="<u4").sum())
    off_sizes = off_unpred + E * esz; off_pay = off_sizes + nb * 8
    assert nb == THREADS and off_pay < len(stream)
    bel = shape[0] * shape[1] * shape[2] // nb
    out = [(f"cut behind {k} ({cut} bytes)", stream[:cut]) for k, cut in (
        ("thread_num", b + 4), ("eb", b + 4 + esz), ("intervals", b + 8 + esz), ("tree_bytes", b + 12 + esz), ("fixed", fixed), ("inside the tree", fixed + tree_bytes // 2),
        ("the tree", off_ucount), ("the counts of verbatim values", off_first), ("the first values", off_unpred), ("the verbatim values", off_sizes),
        ("the payload sizes", off_pay), ("one byte short of the last payload", len(stream) - 1))]
    for what, at, value, n, order in (("intervals = 2", b + 4 + esz, 2, 4, "big"), ("intervals = 131072", b + 4 + esz, 131072, 4, "big"), ("node_count = 0", b + 12 + esz, 0, 4, "big"),
                                      ("thread_num = 7", b, 7, 4, "big"), ("count of verbatim values of box 0 = bel + 1", off_ucount, bel + 1, 4, "little"),
                                      ("payload size of box 0 = stream length + 1", off_sizes, len(stream) + 1, 8, "little"),
                                      ("payload size of the last box = all payload bytes", off_sizes + (nb - 1) * 8, len(stream) - off_pay, 8, "little")):
        bad = bytearray(stream); bad[at:at + n] = int(value).to_bytes(n, order)
        out.append((what, bytes(bad)))
    return out


def _sentinel(n, dtype):
    a = np.empty(n, dtype=dtype)
    a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)[:] = SENTINEL[a.dtype.itemsize]
    return a


def _agree(ctx, oracle, device, shp, dt, stream_dev):
    from sz_amd import api
    shape = SHAPES[shp]
    names = [f"{k}/{shp}/{dt}" for k in KINDS]
    dtype = _array(names[0])[0].dtype
    esz = dtype.itemsize
    good = [_ref(oracle, n, i, 0) for i, n in enumerate(names)]             # (stream, decoded array): the oracle's
    n = shape[0] * shape[1] * shape[2]
    # a region inside box (1, 0, 1) of the 2 x 2 x 2 grid, one value away from each of its faces
    c = [s // 2 for s in shape]
    lo = [c[0] + 1, 1, c[2] + 1]; hi = [2 * c[0] - 1, c[1] - 1, 2 * c[2] - 1]
    ext = [h - l for l, h in zip(lo, hi)]
    crop = [np.ascontiguousarray(d.reshape(shape)[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]) for _, d in good]
    fill, fill_r = _sentinel(n, dtype), _sentinel(ext[0] * ext[1] * ext[2], dtype)
    dev = device and stream_dev
    gregs = [ptr_cases.carve(len(s), 1, pad=256, device=dev).put(s) for s, _ in good]
    for what, bad in _damages(good[BAD][0], esz, shape):
        what = f"{shp}/{dt}, {'device' if stream_dev else 'host'} streams, {what}"
        breg = ptr_cases.carve(len(bad) + 1, 1, pad=256, device=dev).put(bad)
        streams = [(breg.ptr, len(bad)) if i == BAD else (gregs[i].ptr, len(good[i][0])) for i in range(3)]
        # (a) the single call
        o = ptr_cases.carve(n * esz, 0, pad=256, device=dev).put(fill)
        rc_single = api.lib().szhip_decompress_omp(ctx._h, 0 if esz == 4 else 1, breg.ptr, int(stream_dev), len(bad), BODY, *shape, o.ptr, int(stream_dev), None)
        assert rc_single != OK, what
        assert np.array_equal(o.get(), fill.view(np.uint8)), f"{what}: the single call wrote"
        o.check(what)
        # (b), (c), (d): item 1 of three
        for call in ("batch", "shapes", "region"):
            region = call == "region"
            outs = [ptr_cases.carve((fill_r if region else fill).nbytes, 0, pad=256, device=dev).put(fill_r if region else fill) for _ in range(3)]
            ptrs = [r.ptr for r in outs]
            if call == "batch":
                rc, items, _ = ctx.decompress_omp_batch(streams, stream_dev, BODY, shape, dtype, ptrs, stream_dev, raise_on_error=False)
            elif call == "shapes":
                rc, items, _ = ctx.decompress_omp_batch_shapes(streams, stream_dev, BODY, [shape] * 3, dtype, ptrs, stream_dev, raise_on_error=False)
            else:
                rc, items, _, _ = ctx.decompress_omp_batch_region(streams, stream_dev, BODY, [shape] * 3, dtype, [(lo, hi)] * 3, ptrs, stream_dev, raise_on_error=False)
            assert rc == rc_single and items[BAD].rc == rc_single, (what, call, rc, items[BAD].rc, rc_single)
            for i, r in enumerate(outs):
                r.check(f"{what}, {call}, item {i}")
                if i == BAD:
                    assert np.array_equal(r.get(), (fill_r if region else fill).view(np.uint8)), f"{what}: {call} wrote the damaged item's output"
                    continue
                assert items[i].rc == OK, (what, call, i, items[i].rc)
                want = crop[i] if region else good[i][1]
                assert np.array_equal(_bits(r.get().view(dtype)), _bits(want)), f"{what}: {call}, item {i} differs from the oracle's"
        assert rc_single == ERR_STREAM, (what, rc_single)


CASES = [(shp, dt, sd) for shp in SHAPES for dt in ("f32", "f64") for sd in (False, True)]
IDS = [f"{shp}-{dt}-{'device' if sd else 'host'}" for shp, dt, sd in CASES]


@pytest.mark.slow          # (the shim runs a workgroup at a time: every good item's decode costs it a quarter of a second, 20 s a case; the GPU cases take well under a second each)
@pytest.mark.parametrize("shp,dt,stream_dev", CASES, ids=IDS)
def test_decoders_agree_on_cpu_shim(oracle, shim_ctx, shp, dt, stream_dev):
    _agree(shim_ctx, oracle, False, shp, dt, stream_dev)


@pytest.mark.gpu
@pytest.mark.parametrize("shp,dt,stream_dev", CASES, ids=IDS)
def test_hip_decoders_agree(oracle, hip_ctx, shp, dt, stream_dev):
    _agree(hip_ctx, oracle, True, shp, dt, stream_dev)
