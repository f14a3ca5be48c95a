#!/usr/bin/env python3
"""What filling the ghost layers of many patches from their neighbours' compressed streams costs one region call at a time and in one batched region call (GPU box;
writes profiles/r20_batch_region_timing.json).

`count` (64) device-resident streams of float32 S-field patches of 64^3 (z0 varied from patch to patch), ABS 1e-4, the interval optimiser on, thread_num 8 (boxes of
32^3).  Patch k's six ghost layers of `width` (4) cells -- inside a padded device parent of (64 + 2 width)^3 values -- are filled with the six faces of patch k + 1:
6 x count = 384 items, each of which meets 4 of its stream's 8 boxes.  Taken in turn in one loop so that all share whatever else the machine is doing:
  batch_region  one szhip_decompress_omp_batch_region call over the 384 items
  loop          384 x (szhip_decompress_omp_region into a contiguous device array + szhip_scatter_view into the ghost layer): the calls that existed before
  whole_batch   one szhip_decompress_omp_batch of the `count` whole patches into contiguous arrays (no ghost layer is filled: what decoding everything costs)
The loop and the whole-patch batch run code the batched region call's change does not touch.  Time: the host's clock around the calls (every call ends in a
synchronisation of its stream); median and min .. max over the repetitions after warm-up.  Of the batched region call also the launch counts (stats.quant_kernel_launches:
sweeps; stats.packing: placing launches), the distinct streams, and the library's own split.  Before anything is timed the parents of the two ways are compared bit for
bit.  Nothing is asserted about the times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=64)
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_batch_region_timing.json"))
    args = ap.parse_args()
    import torch
    import sz_amd
    from sz_amd.fields import s_field
    if not torch.cuda.is_available():
        raise SystemExit("batch_region_timing.py measures on the GPU; there is none here")
    n, count, w, eb, f32, threads = args.edge, args.count, args.width, 1e-4, np.float32, 8
    shape, m = (n, n, n), n + 2 * args.width
    ctx = sz_amd.HipContext(0)
    meta = sz_amd.make_meta(f32, err_mode=sz_amd.ABS, abs_bound=eb)
    meta = bytes([meta[0], meta[1], meta[2], 0xC0]) + bytes(meta[4:])
    med = lambda v: round(float(np.median(v)), 4)                            # noqa: E731
    span = lambda v: [round(float(min(v)), 4), round(float(max(v)), 4)]      # noqa: E731
    patches = [torch.from_numpy(s_field(n, n, n, f32, z0=(37 * i) % 509)).cuda() for i in range(count)]
    torch.cuda.synchronize()
    rc, blob, size, items, _ = ctx.compress_omp_batch([p.data_ptr() for p in patches], True, shape, f32, [eb] * count, threads, [meta] * count, None, False)
    assert rc == 0
    streams = [torch.frombuffer(bytearray(blob[it.offset:it.offset + it.size]), dtype=torch.uint8).cuda() for it in items[:count]]
    parents = [[torch.full((m, m, m), 1e30, dtype=torch.float32, device="cuda") for _ in range(count)] for _ in range(2)]
    flat = [torch.empty(shape, dtype=torch.float32, device="cuda") for _ in range(count)]
    face = torch.empty(w * n * n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    srcs, regions, outs, whole = [], [], [[], []], [(s.data_ptr(), s.numel()) for s in streams]
    for k in range(count):
        nb = (k + 1) % count
        for d in range(3):
            for side in (0, 1):
                lo, hi, glo = [0, 0, 0], [n, n, n], [w, w, w]
                if side == 0:
                    lo[d], glo[d] = n - w, 0
                else:
                    hi[d], glo[d] = w, w + n
                srcs.append(whole[nb]); regions.append((lo, hi, (m * m, m)))
                for way in (0, 1):
                    outs[way].append(parents[way][k].data_ptr() + 4 * ((glo[0] * m + glo[1]) * m + glo[2]))
    n_items = len(srcs)

    def batch_region():
        return ctx.decompress_omp_batch_region(srcs, True, len(meta), [shape] * n_items, f32, regions, outs[0], True)

    def loop():
        for (p, ln), (lo, hi, pitches), o in zip(srcs, regions, outs[1]):
            ctx.decompress_omp_region(p, True, ln, len(meta), shape, f32, lo, hi, face.data_ptr(), True)
            ctx.scatter_view(face.data_ptr(), [h - l for l, h in zip(lo, hi)], f32, o, True, pitches)

    def whole_batch():
        return ctx.decompress_omp_batch(whole, True, len(meta), shape, f32, [q.data_ptr() for q in flat], True)

    rc, c_items, c_regions, st = batch_region()
    loop()
    torch.cuda.synchronize()
    assert rc == 0 and all(c_items[i].batched == 1 for i in range(n_items))
    for a, b in zip(*parents):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the batched call and the loop of single calls fill the ghost layers differently"
    launches = {"sweeps": int(st.quant_kernel_launches), "placing": int(st.packing), "forms": sorted({int(c_items[i].quant_kernel) for i in range(n_items)}),
                "distinct_streams": len({int(c_regions[i].shares) for i in range(n_items)}), "boxes_decoded": int(st.n_blocks), "values_delivered": int(st.n_elements)}
    calls = {"batch_region": batch_region, "loop": loop, "whole_batch": whole_batch}
    wall = {k: [] for k in calls}
    split = {"quant": [], "entropy": [], "host": []}
    for r in range(args.warmup + args.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            got = f()
            ms = (time.perf_counter() - t0) * 1e3
            if r < args.warmup:
                continue
            wall[k].append(ms)
            if k == "batch_region":
                s = got[-1]
                for key, v in (("quant", s.ms_quant), ("entropy", s.ms_entropy), ("host", s.ms_host)):
                    split[key].append(v)
    res = {"what": f"{count} device-resident streams of {n}^3 float32 patches (S-field slices), ABS {eb}, interval optimiser on, thread_num {threads}; the six faces of width {w} of "
                   f"every patch's neighbour into the ghost layers of its {m}^3 device parent: {n_items} items; wall ms, median [min, max] over {args.reps} repetitions after "
                   f"{args.warmup} warm-up rounds, the three ways taken in turn",
           "device": torch.cuda.get_device_name(0), "items": n_items, "bytes_delivered": n_items * w * n * n * 4, "bytes_streams": int(sum(s.numel() for s in streams)),
           "launches": launches}
    for k in calls:
        res[k] = {"ms": med(wall[k]), "min_max": span(wall[k])}
    res["batch_region"]["batch_split"] = {key: med(v) for key, v in split.items()}
    res["loop_over_batch_region"] = round(res["loop"]["ms"] / res["batch_region"]["ms"], 3)
    res["whole_batch_over_batch_region"] = round(res["whole_batch"]["ms"] / res["batch_region"]["ms"], 3)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
