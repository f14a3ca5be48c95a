#!/usr/bin/env python3
"""What many patches with ghost layers cost one view call at a time, packed by the caller, and in one batched view call (GPU box; writes
profiles/r18_batch_view_timing.json).

`count` (64) device-resident patches: float32 S-field slices of 64^3 (z0 varied from patch to patch), each the interior of a padded parent with `ghost` cells a side
-- ghost 2: the interior starts 8 bytes off a 16-byte boundary, the batched call gathers it; ghost 4: everything on 16 bytes, the column form runs on the parent --,
ABS 1e-4, the interval optimiser on, thread_num 8 (boxes of 32^3); streams and decode targets device-resident.  Per ghost width and direction, taken in turn in one
loop so that all share whatever else the machine is doing:
  batch_view   one szhip_compress_omp_batch_view / szhip_decompress_omp_batch_view call
  (a) loop     `count` calls of szhip_compress_omp_view / szhip_decompress_omp_view
  (b) packed   compress: `count` x (szhip_pack_view + a copy of the packed patch out of the context's input buffer, which every pack_view call reuses -- made
               with szhip_scatter_view onto a contiguous array), then szhip_compress_omp_batch on the copies; decode: szhip_decompress_omp_batch into contiguous
               arrays, then `count` x szhip_scatter_view
Both baselines run code the batched view calls' change does not touch.  Time: the host's clock around the calls (every call ends in a synchronisation of its
stream; (b) ends in a device synchronisation); median and min .. max over the repetitions after warm-up.  Of the batched view calls also the launch counts
(stats.quant_kernel_launches: sweeps; stats.packing: gather / scatter launches) and the library's own split.  Before anything is timed the three ways' streams and
decoded parents are compared.  Nothing is asserted about the times."""
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
    ap.add_argument("--ghosts", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_batch_view_timing.json"))
    args = ap.parse_args()
    import torch
    import sz_amd
    from sz_amd.fields import s_field
    if not torch.cuda.is_available():
        raise SystemExit("batch_view_timing.py measures on the GPU; there is none here")
    n, count, eb, f32, threads = args.edge, args.count, 1e-4, np.float32, 8
    shape = (n, n, n)
    ctx = sz_amd.HipContext(0)
    meta = sz_amd.make_meta(f32, err_mode=sz_amd.ABS, abs_bound=eb)
    meta = bytes([meta[0], meta[1], meta[2], 0xC0]) + bytes(meta[4:])
    med = lambda v: round(float(np.median(v)), 4)                            # noqa: E731
    span = lambda v: [round(float(min(v)), 4), round(float(max(v)), 4)]      # noqa: E731
    res = {"what": f"{count} device-resident patches of {n}^3 float32 (S-field slices) inside parents with `ghost` cells a side, ABS {eb}, interval optimiser on, thread_num "
                   f"{threads}; wall ms, median [min, max] over {args.reps} repetitions after {args.warmup} warm-up rounds, the three ways taken in turn",
           "device": torch.cuda.get_device_name(0), "cases": []}
    fields = [torch.from_numpy(s_field(n, n, n, f32, z0=(37 * i) % 509)) for i in range(count)]
    for ghost in args.ghosts:
        m = n + 2 * ghost
        first = 4 * (ghost * m * m + ghost * m + ghost)
        pitches = (m * m, m)
        parents, targets = [], [[], [], []]
        for i in range(count):
            p = torch.full((m, m, m), 1e30, dtype=torch.float32, device="cuda")
            p[ghost:-ghost, ghost:-ghost, ghost:-ghost] = fields[i].cuda()
            parents.append(p)
            for t in targets:
                t.append(torch.full((m, m, m), 1e30, dtype=torch.float32, device="cuda"))
        packed = [torch.empty(shape, dtype=torch.float32, device="cuda") for _ in range(count)]
        flat = [torch.empty(shape, dtype=torch.float32, device="cuda") for _ in range(count)]
        torch.cuda.synchronize()
        views = [p.data_ptr() + first for p in parents]
        tviews = [[t.data_ptr() + first for t in ts] for ts in targets]

        def batch_compress(out_dev=True):
            return ctx.compress_omp_batch_view(views, True, shape, pitches, f32, [eb] * count, threads, [meta] * count, None, out_dev)

        def loop_compress(out_dev=True):
            return [ctx.compress_omp_view(v, True, shape, pitches, f32, eb, threads, meta, None, out_dev) for v in views]

        def packed_compress(out_dev=True):
            for v, q in zip(views, packed):
                d = ctx.pack_view(v, True, shape, pitches, f32)
                ctx.scatter_view(d, shape, f32, q.data_ptr(), True, (n * n, n))
            torch.cuda.synchronize()
            return ctx.compress_omp_batch([q.data_ptr() for q in packed], True, shape, f32, [eb] * count, threads, [meta] * count, None, out_dev)

        # ---- the same streams three ways
        singles = [s[0] for s in loop_compress(False)]
        rc, blob, size, items, st = batch_compress(False)
        assert rc == 0 and all(blob[it.offset:it.offset + it.size] == s for it, s in zip(items[:count], singles)), ghost
        assert all(it.batched == 1 for it in items[:count]), ghost
        launches = {"compress": {"sweeps": int(st.quant_kernel_launches), "gathers": int(st.packing), "forms": sorted({int(it.quant_kernel) for it in items[:count]})}}
        rc, blob, size, items, _ = packed_compress(False)
        assert rc == 0 and all(blob[it.offset:it.offset + it.size] == s for it, s in zip(items[:count], singles)), ghost
        streams = [torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda() for s in singles]
        torch.cuda.synchronize()
        srcs = [(s.data_ptr(), s.numel()) for s in streams]

        def batch_decompress():
            return ctx.decompress_omp_batch_view(srcs, True, len(meta), shape, f32, tviews[0], True, pitches)

        def loop_decompress():
            return [ctx.decompress_omp_view(p, True, ln, len(meta), shape, f32, t, True, pitches) for (p, ln), t in zip(srcs, tviews[1])]

        def packed_decompress():
            got = ctx.decompress_omp_batch(srcs, True, len(meta), shape, f32, [q.data_ptr() for q in flat], True)
            for q, t in zip(flat, tviews[2]):
                ctx.scatter_view(q.data_ptr(), shape, f32, t, True, pitches)
            torch.cuda.synchronize()
            return got

        rc, items, st = batch_decompress()
        loop_decompress(); packed_decompress()
        torch.cuda.synchronize()
        assert rc == 0 and all(it.batched == 1 for it in items[:count]), ghost
        launches["decompress"] = {"sweeps": int(st.quant_kernel_launches), "scatters": int(st.packing), "forms": sorted({int(it.quant_kernel) for it in items[:count]})}
        for a, b, c in zip(*targets):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32)), ghost
        calls = {"compress_batch_view": batch_compress, "compress_loop": loop_compress, "compress_packed": packed_compress,
                 "decompress_batch_view": batch_decompress, "decompress_loop": loop_decompress, "decompress_packed": packed_decompress}
        wall = {k: [] for k in calls}
        split = {k: {"prequant": [], "quant": [], "entropy": [], "host": []} for k in ("compress_batch_view", "decompress_batch_view")}
        for r in range(args.warmup + args.reps):
            for k, f in calls.items():
                t0 = time.perf_counter()
                got = f()
                ms = (time.perf_counter() - t0) * 1e3
                if r < args.warmup:
                    continue
                wall[k].append(ms)
                if k in split:
                    s = got[-1]
                    for key, v in (("prequant", s.ms_prequant), ("quant", s.ms_quant), ("entropy", s.ms_entropy), ("host", s.ms_host)):
                        split[k][key].append(v)
        case = {"ghost": ghost, "first_value_offset_mod_16": first % 16, "count": count, "edge": n, "bytes_in": count * n ** 3 * 4,
                "bytes_streams": int(sum(len(s) for s in singles)), "launches": launches}
        for k in calls:
            case[k] = {"ms": med(wall[k]), "min_max": span(wall[k])}
        for k in split:
            case[k]["batch_split"] = {key: med(v) for key, v in split[k].items()}
        for d in ("compress", "decompress"):
            case[d + "_loop_over_batch_view"] = round(case[d + "_loop"]["ms"] / case[d + "_batch_view"]["ms"], 3)
            case[d + "_packed_over_batch_view"] = round(case[d + "_packed"]["ms"] / case[d + "_batch_view"]["ms"], 3)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del parents, targets, packed, flat, streams
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
