#!/usr/bin/env python3
"""What a batch of arrays of DIFFERENT shapes costs three ways (GPU box; writes profiles/r19_batch_shapes_timing.json), in the manner of tools/batch_timing.py.

float32 S-field slices (z0 varied from array to array), arrays, streams and outputs device-resident, ABS 1e-4, the interval optimiser on.  Per batch, taken in turn in
one loop so that all share whatever else the machine is doing:
  loop     one szhip_compress_omp / szhip_decompress_omp call per array
  by_shape one szhip_compress_omp_batch / szhip_decompress_omp_batch call per distinct (shape, thread_num): the best a caller of the same-shape calls can do
  shapes   ONE szhip_compress_omp_batch_shapes / szhip_decompress_omp_batch_shapes call
The batches:
  acceptance  64 arrays, 16 each of 32^3, 64^3, 32 x 64 x 64 and 48^3 (thread_num 8), interleaved
  distinct    64 arrays of 64 distinct shapes (r0 from 8 .. 64 planes, r1 and r2 from {32, 48, 64}; thread_num 8): by_shape degenerates to one batch call per array
  skewed      one 16 x 128 x 128 array in 64 boxes beside 63 of 4 x 32 x 32 in 2 boxes: what the returning workgroups cost
Time: the host's clock around the blocking calls; median and min .. max over the repetitions after warm-up.  Of the new call also the library's own split
(szhip_stats).  Before anything is timed the streams of the three alternatives are compared, and the decoded arrays.  Nothing is asserted about the times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batches():
    four = [(32, 32, 32), (64, 64, 64), (32, 64, 64), (48, 48, 48)]
    planes = [8, 16, 24, 32, 40, 48, 56, 64]                                 # (thread_num 8 halves every extent: box faces of at most 32 x 32 rows)
    distinct = [(r0, r1, r2) for r0 in planes for r1 in (32, 48, 64) for r2 in (32, 48, 64)][:64]
    return {"acceptance": [(four[i % 4], 8) for i in range(64)],
            "distinct": [(s, 8) for s in distinct],
            "skewed": [((16, 128, 128), 64)] + [((4, 32, 32), 2)] * 63}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", nargs="+", default=["acceptance", "distinct", "skewed"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_batch_shapes_timing.json"))
    args = ap.parse_args()
    import torch
    import sz_amd
    from sz_amd.fields import s_field
    if not torch.cuda.is_available():
        raise SystemExit("batch_shapes_timing.py measures on the GPU; there is none here")
    eb = 1e-4
    f32 = np.float32
    ctx = sz_amd.HipContext(0)
    meta = sz_amd.make_meta(f32, err_mode=sz_amd.ABS, abs_bound=eb)
    meta = bytes([meta[0], meta[1], meta[2], 0xC0]) + bytes(meta[4:])
    med = lambda v: round(float(np.median(v)), 4)                            # noqa: E731
    span = lambda v: [round(float(min(v)), 4), round(float(max(v)), 4)]      # noqa: E731
    res = {"what": f"float32 S-field slices, ABS {eb}, interval optimiser on, everything device-resident; wall ms of one single call per array (loop), one same-shape "
                   f"batch call per distinct shape (by_shape) and ONE call on all shapes (shapes), median [min, max] over {args.reps} repetitions after {args.warmup} "
                   "warm-up rounds, the three taken in turn; split: medians of the new call's szhip_stats (device events; host: the code books and headers)",
           "device": torch.cuda.get_device_name(0), "cases": []}
    for name in args.batches:
        items = batches()[name]
        count = len(items)
        arrays = [torch.from_numpy(s_field(*s, f32, z0=(37 * i) % 509)).cuda() for i, (s, _) in enumerate(items)]
        outs = [[torch.empty_like(a) for a in arrays] for _ in range(3)]
        torch.cuda.synchronize()
        ptrs = [a.data_ptr() for a in arrays]
        shapes4 = [s + (t,) for s, t in items]
        groups = {}
        for i, key in enumerate(items):
            groups.setdefault(key, []).append(i)

        def c_loop():
            return [ctx.compress_omp(p, True, s, f32, eb, t, meta, None, True) for p, (s, t) in zip(ptrs, items)]

        def c_by_shape(on_device=True):
            return [ctx.compress_omp_batch([ptrs[i] for i in idx], True, s, f32, [eb] * len(idx), t, [meta] * len(idx), None, on_device) for (s, t), idx in groups.items()]

        def c_shapes(on_device=True):
            return ctx.compress_omp_batch_shapes(ptrs, True, shapes4, f32, [eb] * count, [meta] * count, None, on_device)

        # ---- the same streams three ways
        singles = [ctx.compress_omp(p, True, s, f32, eb, t, meta)[0] for p, (s, t) in zip(ptrs, items)]
        rc, blob, size, its, st = c_shapes(False)
        assert rc == 0 and all(blob[it.offset:it.offset + it.size] == s for it, s in zip(its[:count], singles)), name
        n_batched = sum(it.batched for it in its[:count])
        launches = st.quant_kernel_launches
        for (rc, blob, size, its, _), idx in zip(c_by_shape(False), groups.values()):
            assert rc == 0 and all(blob[it.offset:it.offset + it.size] == singles[i] for it, i in zip(its[:len(idx)], idx)), name
        streams = [torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda() for s in singles]
        torch.cuda.synchronize()
        srcs = [(s.data_ptr(), s.numel()) for s in streams]

        def d_loop():
            return [ctx.decompress_omp(p, True, ln, len(meta), s, f32, o.data_ptr(), True) for (p, ln), (s, _), o in zip(srcs, items, outs[0])]

        def d_by_shape():
            return [ctx.decompress_omp_batch([srcs[i] for i in idx], True, len(meta), s, f32, [outs[1][i].data_ptr() for i in idx], True) for (s, _), idx in groups.items()]

        def d_shapes():
            return ctx.decompress_omp_batch_shapes(srcs, True, len(meta), [s for s, _ in items], f32, [o.data_ptr() for o in outs[2]], True)

        d_loop(); d_by_shape(); rc, its, st = d_shapes()
        torch.cuda.synchronize()
        assert rc == 0, name
        d_batched = sum(it.batched for it in its[:count])
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32)) for a, b, c in zip(*outs)), name
        calls = {"compress_loop": c_loop, "compress_by_shape": c_by_shape, "compress_shapes": c_shapes, "decompress_loop": d_loop, "decompress_by_shape": d_by_shape,
                 "decompress_shapes": d_shapes}
        wall = {k: [] for k in calls}
        split = {k: {"prequant": [], "quant": [], "entropy": [], "host": []} for k in ("compress_shapes", "decompress_shapes")}
        for r in range(args.warmup + args.reps):
            for k, f in calls.items():
                t0 = time.perf_counter()
                got = f()
                ms = (time.perf_counter() - t0) * 1e3
                if r < args.warmup:
                    continue
                wall[k].append(ms)
                if k in split:
                    for key, v in (("prequant", got[-1].ms_prequant), ("quant", got[-1].ms_quant), ("entropy", got[-1].ms_entropy), ("host", got[-1].ms_host)):
                        split[k][key].append(v)
        case = {"batch": name, "count": count, "distinct_shapes": len(groups), "batched_items": n_batched, "decode_batched_items": d_batched, "compress_sweep_launches": launches,
                "decompress_sweep_launches": st.quant_kernel_launches, "bytes_in": int(sum(a.numel() for a in arrays)) * 4, "bytes_streams": int(sum(len(s) for s in singles))}
        for k in calls:
            case[k] = {"ms": med(wall[k]), "min_max": span(wall[k])}
        for k in split:
            case[k]["split"] = {key: med(v) for key, v in split[k].items()}
        for d in ("compress", "decompress"):
            by, one = case[d + "_by_shape"], case[d + "_shapes"]
            case[d + "_by_shape_over_shapes"] = round(by["ms"] / one["ms"], 3)
            case[d + "_gain_beyond_by_shape_spread"] = bool(by["ms"] - one["ms"] > by["min_max"][1] - by["min_max"][0])
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del arrays, outs, streams
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
