#!/usr/bin/env python3
"""What compressing from and decoding into a view costs beside the contiguous calls (GPU box; writes profiles/r13_view_timing.json).

The bench's 512^3 float32 S-field at ABS 1e-4, thread_num 4096 (boxes of 32^3); arrays, views and streams device-resident; device events around whole calls, taken
in turn in one loop after a warm-up so that they share whatever else the machine is doing.
  (a) contiguous   compress_omp / decompress_omp on the contiguous array: the code of the parent commit
  (b) aligned      the same values as the interior of a 520^3 parent, 4 ghost values a side: rows and planes 16-byte aligned, the column form runs.
                   compress_omp_view / decompress_omp_view (direct) against pack_view + compress_omp and decompress_omp + scatter_view
  (c) unaligned    the interior of a 516^3 parent, 2 ghost values: the base is not 16-byte aligned.  The view call packs such a view of 32 x 32 box faces itself
                   and runs the column form on the copy (value by value on the view it took 3.73 / 3.41 ms).  Both ways as in (b)
  (d) SZ 2.1       pack_view + szhip_compress against szhip_compress on the contiguous array
Nothing is asserted about the times; streams and decoded values are compared before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_view_timing.json"))
    args = ap.parse_args()
    import torch
    import sz_amd
    from sz_amd.fields import s_field
    if not torch.cuda.is_available():
        raise SystemExit("view_timing.py measures on the GPU; there is none here")
    n, eb, f32 = args.edge, 1e-4, np.float32
    boxes = (n // 32) ** 3
    x = torch.from_numpy(s_field(n, n, n, f32)).cuda()
    parents, views, targets, tviews = {}, {}, {}, {}                          # (decode goes into parents of its own: the views compressed keep the field's values)
    for kind, ghost in (("aligned", 4), ("unaligned", 2)):
        p = torch.full((n + 2 * ghost,) * 3, 1e30, dtype=torch.float32, device="cuda")
        p[ghost:-ghost, ghost:-ghost, ghost:-ghost] = x
        m = n + 2 * ghost
        parents[kind] = p
        views[kind] = (p.data_ptr() + 4 * (ghost * m * m + ghost * m + ghost), (m * m, m), ghost)
        targets[kind] = torch.full_like(p, 1e30)
        tviews[kind] = (targets[kind].data_ptr() + 4 * (ghost * m * m + ghost * m + ghost), (m * m, m), ghost)
    ctx = sz_amd.HipContext(0)
    meta = sz_amd.make_meta(f32, err_mode=sz_amd.ABS, abs_bound=eb)
    meta_omp = bytes([meta[0], meta[1], meta[2], 0xC0]) + bytes(meta[4:])
    shape = (n, n, n)
    blob, osize, st0 = ctx.compress_omp(x.data_ptr(), True, shape, f32, eb, boxes, meta_omp)
    stream = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    full = torch.empty_like(x)
    torch.cuda.synchronize()
    ctx.decompress_omp(stream.data_ptr(), True, osize, len(meta_omp), shape, f32, full.data_ptr(), True)
    torch.cuda.synchronize()
    forms = {"contiguous": int(st0.quant_kernel)}
    for kind, (ptr, pitches, ghost) in views.items():                         # the bar, before any timing
        b2, _, st = ctx.compress_omp_view(ptr, True, shape, pitches, f32, eb, boxes, meta_omp)
        assert b2 == blob, kind
        forms[kind] = int(st.quant_kernel)
        ctx.decompress_omp_view(stream.data_ptr(), True, osize, len(meta_omp), shape, f32, tviews[kind][0], True, pitches)
        torch.cuda.synchronize()
        assert torch.equal(targets[kind][ghost:-ghost, ghost:-ghost, ghost:-ghost].contiguous().view(torch.int32), full.view(torch.int32)), kind
        assert float(targets[kind][0, 0, 0]) == float(np.float32(1e30)) and float(targets[kind][-1, -1, -1]) == float(np.float32(1e30))
    sz21_ref, sz21_n, _ = ctx.compress(x.data_ptr(), True, shape, f32, eb, meta)
    packed = ctx.pack_view(views["aligned"][0], True, shape, views["aligned"][1], f32)
    sz21_view, _, _ = ctx.compress(packed, True, shape, f32, eb, meta)
    assert sz21_view == sz21_ref

    def c_direct(kind):
        ptr, pitches, _ = views[kind]
        ctx.compress_omp_view(ptr, True, shape, pitches, f32, eb, boxes, meta_omp, None, True)

    def c_packed(kind):
        ptr, pitches, _ = views[kind]
        ctx.compress_omp(ctx.pack_view(ptr, True, shape, pitches, f32), True, shape, f32, eb, boxes, meta_omp, None, True)

    def d_direct(kind):
        ptr, pitches, _ = tviews[kind]
        ctx.decompress_omp_view(stream.data_ptr(), True, osize, len(meta_omp), shape, f32, ptr, True, pitches)

    def d_scatter(kind):
        ptr, pitches, _ = tviews[kind]
        ctx.decompress_omp(stream.data_ptr(), True, osize, len(meta_omp), shape, f32, full.data_ptr(), True)
        ctx.scatter_view(full.data_ptr(), shape, f32, ptr, True, pitches)

    calls = {"a_compress": lambda: ctx.compress_omp(x.data_ptr(), True, shape, f32, eb, boxes, meta_omp, None, True),
             "a_decompress": lambda: ctx.decompress_omp(stream.data_ptr(), True, osize, len(meta_omp), shape, f32, full.data_ptr(), True),
             "d_sz21_contiguous": lambda: ctx.compress(x.data_ptr(), True, shape, f32, eb, meta, None, True),
             "d_sz21_pack_then_compress": lambda: ctx.compress(ctx.pack_view(views["aligned"][0], True, shape, views["aligned"][1], f32), True, shape, f32, eb, meta, None, True)}
    for tag, kind in (("b", "aligned"), ("c", "unaligned")):
        calls[f"{tag}_compress_view"] = lambda k=kind: c_direct(k)
        calls[f"{tag}_pack_then_compress"] = lambda k=kind: c_packed(k)
        calls[f"{tag}_decompress_view"] = lambda k=kind: d_direct(k)
        calls[f"{tag}_decompress_then_scatter"] = lambda k=kind: d_scatter(k)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in calls}
    for r in range(args.warmup + args.rounds):
        for k, f in calls.items():
            torch.cuda.synchronize()
            ev0.record(); f(); ev1.record()                                   # (every call of the library ends in a synchronisation of its own stream)
            torch.cuda.synchronize()
            if r >= args.warmup:
                ms[k].append(ev0.elapsed_time(ev1))
    med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    res = {"what": f"{n}^3 float32 S-field, ABS {eb}, thread_num {boxes}; arrays, views and streams on the device; device events around whole calls, {args.rounds} rounds of all "
                   f"calls in turn after {args.warmup} warm-up rounds; medians in ms (min .. max beside them).  aligned: interior of a {n + 8}^3 parent (4 ghost values a side); "
                   f"unaligned: interior of a {n + 4}^3 parent (2 ghost values)",
           "device": torch.cuda.get_device_name(0), "stream_bytes": int(osize), "quant_kernel": forms,
           "median_ms": med, "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "ratios": {"b_compress_view / a_compress": round(med["b_compress_view"] / med["a_compress"], 4),
                      "b_decompress_view / a_decompress": round(med["b_decompress_view"] / med["a_decompress"], 4),
                      "b_compress_view / b_pack_then_compress": round(med["b_compress_view"] / med["b_pack_then_compress"], 4),
                      "b_decompress_view / b_decompress_then_scatter": round(med["b_decompress_view"] / med["b_decompress_then_scatter"], 4),
                      "c_compress_view / c_pack_then_compress": round(med["c_compress_view"] / med["c_pack_then_compress"], 4),
                      "c_decompress_view / c_decompress_then_scatter": round(med["c_decompress_view"] / med["c_decompress_then_scatter"], 4),
                      "d_sz21_pack_then_compress / d_sz21_contiguous": round(med["d_sz21_pack_then_compress"] / med["d_sz21_contiguous"], 4)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
