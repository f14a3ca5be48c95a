#!/usr/bin/env python3
"""What many small arrays cost one call at a time and in one batch call (GPU box; writes profiles/r15_batch_timing.json).

float32 S-field slices of 32^3, 64^3 and 128^3 (z0 varied from array to array), counts 1, 8, 64 and 512, arrays, streams and outputs device-resident, ABS 1e-4,
the interval optimiser on, boxes of 32^3 (16^3 for the 32^3 arrays: thread_num 8).  Per (edge, count), in one loop so that both share whatever else the machine is doing:
  loop   `count` calls of szhip_compress_omp / szhip_decompress_omp, one after the other (the yardstick: code this tool's subject does not touch)
  batch  one szhip_compress_omp_batch / szhip_decompress_omp_batch call
Time: the host's clock around the calls (every call ends in a synchronisation of its stream); median and min .. max over the repetitions after warm-up.  Of the
batch calls also the library's own split (szhip_stats: ms_prequant / ms_quant / ms_entropy from device events, ms_host).  Before anything is timed the batch's
streams are compared with the single calls' streams and the decoded arrays with the single calls' arrays.  Nothing is asserted about the times.
A (edge, count) whose arrays exceed --max-bytes is skipped and listed."""
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
    ap.add_argument("--edges", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 8, 64, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-bytes", type=int, default=2 << 30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_batch_timing.json"))
    args = ap.parse_args()
    import torch
    import sz_amd
    from sz_amd.fields import s_field
    if not torch.cuda.is_available():
        raise SystemExit("batch_timing.py measures on the GPU; there is none here")
    eb = 1e-4
    ctx = sz_amd.HipContext(0)
    meta = sz_amd.make_meta(np.float32, err_mode=sz_amd.ABS, abs_bound=eb)
    meta = bytes([meta[0], meta[1], meta[2], 0xC0]) + bytes(meta[4:])
    med = lambda v: round(float(np.median(v)), 4)                            # noqa: E731
    span = lambda v: [round(float(min(v)), 4), round(float(max(v)), 4)]      # noqa: E731
    res = {"what": f"float32 S-field slices, ABS {eb}, interval optimiser on, everything device-resident; wall ms of `count` single calls in a loop and of one batch "
                   f"call, median [min, max] over {args.reps} repetitions after {args.warmup} warm-up rounds, loop and batch taken in turn; batch_split: medians of the "
                   "batch call's szhip_stats (device events; host: the code books and headers)",
           "device": torch.cuda.get_device_name(0), "cases": [], "skipped": []}
    for n in args.edges:
        threads = 8 if n <= 64 else (n // 32) ** 3
        shape = (n, n, n)
        for count in args.counts:
            if count * n ** 3 * 4 > args.max_bytes:
                res["skipped"].append({"edge": n, "count": count, "why": "arrays beyond --max-bytes"})
                continue
            arrays = [torch.from_numpy(s_field(n, n, n, np.float32, z0=(37 * i) % 509)).cuda() for i in range(count)]
            outs = [torch.empty_like(a) for a in arrays]
            outs2 = [torch.empty_like(a) for a in arrays]
            torch.cuda.synchronize()
            ptrs = [a.data_ptr() for a in arrays]

            def loop_compress():
                return [ctx.compress_omp(p, True, shape, np.float32, eb, threads, meta, None, True) for p in ptrs]

            def batch_compress():
                return ctx.compress_omp_batch(ptrs, True, shape, np.float32, [eb] * count, threads, [meta] * count, None, True)

            # ---- the same streams, the same values, all in the shared launches
            singles = [ctx.compress_omp(p, True, shape, np.float32, eb, threads, meta)[0] for p in ptrs]
            rc, blob, size, items, st = ctx.compress_omp_batch(ptrs, True, shape, np.float32, [eb] * count, threads, [meta] * count)
            assert rc == 0 and all(blob[it.offset:it.offset + it.size] == s for it, s in zip(items[:count], singles)), (n, count)
            assert all(it.batched == 1 for it in items[:count]), (n, count)
            streams = [torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda() for s in singles]
            torch.cuda.synchronize()
            srcs = [(s.data_ptr(), s.numel()) for s in streams]

            def loop_decompress():
                return [ctx.decompress_omp(p, True, ln, len(meta), shape, np.float32, o.data_ptr(), True) for (p, ln), o in zip(srcs, outs)]

            def batch_decompress():
                return ctx.decompress_omp_batch(srcs, True, len(meta), shape, np.float32, [o.data_ptr() for o in outs2], True)

            loop_decompress(); rc, items, st = batch_decompress()
            torch.cuda.synchronize()
            assert rc == 0 and all(it.batched == 1 for it in items[:count]), (n, count)
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, outs2)), (n, count)
            calls = {"compress_loop": loop_compress, "compress_batch": batch_compress, "decompress_loop": loop_decompress, "decompress_batch": batch_decompress}
            wall = {k: [] for k in calls}
            split = {k: {"prequant": [], "quant": [], "entropy": [], "host": []} for k in ("compress_batch", "decompress_batch")}
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
            case = {"edge": n, "count": count, "thread_num": threads, "bytes_in": count * n ** 3 * 4, "bytes_streams": int(sum(len(s) for s in singles))}
            for k in calls:
                case[k] = {"ms": med(wall[k]), "min_max": span(wall[k])}
            for k in split:
                case[k]["batch_split"] = {key: med(v) for key, v in split[k].items()}
            for d in ("compress", "decompress"):
                case[d + "_loop_over_batch"] = round(case[d + "_loop"]["ms"] / case[d + "_batch"]["ms"], 3)
                case[d + "_gain_beyond_loop_spread"] = bool(case[d + "_loop"]["ms"] - case[d + "_batch"]["ms"] > case[d + "_loop"]["min_max"][1] - case[d + "_loop"]["min_max"][0])
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del arrays, outs, outs2, streams
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
