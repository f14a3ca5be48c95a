#!/usr/bin/env python3
"""What a relative bound costs many small arrays one call at a time and in one batch call (GPU box; writes profiles/r17_args_batch_timing.json).

Protocol as tools/batch_timing.py: float32 S-field slices (z0 varied from array to array), REL 1e-4, arrays device-resident, 8 / 64 / 512 arrays of 32^3 and
64^3, 8 / 64 of 128^3; boxes of 32^3 (16^3 for the 32^3 arrays: SZ_HIP_OMP_THREADS 8).  The host's clock runs around blocking calls; loop and batch are taken in
turn, median [min, max] over the repetitions after the warm-up rounds.  Per (edge, count):
  compress   a loop of SZ_hip_compress_device under SZ_HIP_MODE=omp (the parent's path)    against  one SZ_hip_compress_args_batch
  range      a loop of szhip_minmax                                                         against  one szhip_minmax_batch
  report     a loop of szhip_compare, without and with the correlation                      against  one szhip_compare_batch
Before anything is timed the batch's outputs are compared with the loop's.  Nothing is asserted about the times; `*_gain_beyond_loop_spread` says whether the batch
beats its loop by more than the loop's own min .. max spread.  For the range scan and pass 1 of the report the bytes read over the call time are given too."""
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
    ap.add_argument("--counts", type=int, nargs="+", default=[8, 64, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-bytes", type=int, default=600 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_args_batch_timing.json"))
    args = ap.parse_args()
    import torch
    import sz_amd
    from sz_amd.fields import s_field
    if not torch.cuda.is_available():
        raise SystemExit("args_batch_timing.py measures on the GPU; there is none here")
    rel = 1e-4
    assert sz_amd.SZ_Init(os.path.join(ROOT, "tests", "golden", "sz_speed.config")) == 0
    ctx = sz_amd.HipContext(0)
    med = lambda v: round(float(np.median(v)), 4)                            # noqa: E731
    span = lambda v: [round(float(min(v)), 4), round(float(max(v)), 4)]      # noqa: E731
    res = {"what": f"float32 S-field slices, REL {rel}, arrays device-resident; wall ms of `count` single calls in a loop and of one batch call, median [min, max] "
                   f"over {args.reps} repetitions after {args.warmup} warm-up rounds, loop and batch taken in turn",
           "device": torch.cuda.get_device_name(0), "cases": [], "skipped": []}
    for n in args.edges:
        os.environ["SZ_HIP_OMP_THREADS"] = str(8 if n <= 64 else (n // 32) ** 3)
        shape = (n, n, n)
        for count in args.counts:
            if count * n ** 3 * 4 > args.max_bytes:
                res["skipped"].append({"edge": n, "count": count, "why": "arrays beyond --max-bytes"})
                continue
            arrays = [torch.from_numpy(s_field(n, n, n, np.float32, z0=(37 * i) % 509)).cuda() for i in range(count)]
            torch.cuda.synchronize()
            ptrs = [a.data_ptr() for a in arrays]

            def compress_loop():
                os.environ["SZ_HIP_MODE"] = "omp"
                try:
                    return [sz_amd.SZ_hip_compress_device(p, shape, np.float32, sz_amd.REL, 0.0, rel) for p in ptrs]
                finally:
                    del os.environ["SZ_HIP_MODE"]

            def compress_batch():
                return sz_amd.SZ_hip_compress_args_batch(ptrs, True, shape, np.float32, sz_amd.REL, 0.0, rel)

            def range_loop():
                return [ctx.minmax(p, True, n ** 3, np.float32) for p in ptrs]

            def range_batch():
                return ctx.minmax_batch(ptrs, True, n ** 3, np.float32)[1]

            # ---- the same streams, ranges and records first
            singles = compress_loop()
            rc, streams, batched = compress_batch()
            assert rc == 0 and streams == singles and all(batched), (n, count)
            assert range_batch() == range_loop(), (n, count)
            outs = [torch.empty_like(a) for a in arrays]
            assert sz_amd.SZ_hip_decompress_batch(streams, [o.data_ptr() for o in outs], True, shape, np.float32) == 0
            torch.cuda.synchronize()
            optrs = [o.data_ptr() for o in outs]
            bounds = [float(np.frombuffer(s[36:40], dtype=">f4")[0]) for s in streams]

            def report(corr):
                return (lambda: [ctx.compare(p, q, True, n ** 3, np.float32, b, -1.0, corr) for p, q, b in zip(ptrs, optrs, bounds)],
                        lambda: ctx.compare_batch(ptrs, optrs, True, n ** 3, np.float32, bounds, None, corr)[1])

            for corr in (False, True):
                lp, bt = report(corr)
                assert [q.raw for q in bt()] == [q.raw for q in lp()], (n, count, corr)
            calls = {"compress_loop": compress_loop, "compress_batch": compress_batch, "range_loop": range_loop, "range_batch": range_batch,
                     "report_loop": report(False)[0], "report_batch": report(False)[1], "report_corr_loop": report(True)[0], "report_corr_batch": report(True)[1]}
            wall = {k: [] for k in calls}
            for r in range(args.warmup + args.reps):
                for k, f in calls.items():
                    t0 = time.perf_counter()
                    f()
                    ms = (time.perf_counter() - t0) * 1e3
                    if r >= args.warmup:
                        wall[k].append(ms)
            case = {"edge": n, "count": count, "thread_num": int(os.environ["SZ_HIP_OMP_THREADS"]), "bytes_in": count * n ** 3 * 4,
                    "bytes_streams": int(sum(len(s) for s in streams))}
            for k in calls:
                case[k] = {"ms": med(wall[k]), "min_max": span(wall[k])}
            for d in ("compress", "range", "report", "report_corr"):
                case[d + "_loop_over_batch"] = round(case[d + "_loop"]["ms"] / case[d + "_batch"]["ms"], 3)
                case[d + "_gain_beyond_loop_spread"] = bool(case[d + "_loop"]["ms"] - case[d + "_batch"]["ms"] > case[d + "_loop"]["min_max"][1] - case[d + "_loop"]["min_max"][0])
            # bytes read over the whole call's time (launch, the kernels, the read-back, the host's part): the range scan reads the arrays once, the report both arrays once
            case["range_batch_GBps"] = round(case["bytes_in"] / case["range_batch"]["ms"] / 1e6, 1)
            case["report_batch_GBps"] = round(2 * case["bytes_in"] / case["report_batch"]["ms"] / 1e6, 1)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del arrays, outs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    ctx.close()
    sz_amd.SZ_Finalize()


if __name__ == "__main__":
    main()
