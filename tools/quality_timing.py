#!/usr/bin/env python3
"""What the error report costs where the data lies (GPU box; writes profiles/r15_quality_timing.txt).

Two device-resident pairs -- 512^3 float32 (the bench's S-field and a copy with errors of about 1e-4) and 1024 x 1024 x 512 float64 (a seeded field built on the
device) -- and four ways to the same report:
  (a) fused        szhip_compare: one read of the two arrays (k_quality_pass1 + the one-workgroup merge)
  (b) fused+corr   the same with SZHIP_Q_CORR: two reads (k_quality_pass2 behind the first)
  (c) torch        the report composed from torch expressions on the device, as bench.py does it today: (dec - x).abs(), its max, the double sum of its
                   squares, x.max() - x.min() -- several reads and two temporaries
  (d) host         the route a C caller with device pointers had before: both arrays copied to the host, then the loop of examples/sz_cli.c: report()
                   (restated with numpy: max |dec - x| in the array's type, the double sum of its squares, min and max)
Times are host clocks around calls that end in a device synchronisation, taken in turn in one loop after a warm-up, so that the ways share whatever else the
machine is doing; min / median / max of the rounds are written.  A call of (a) is two launches, one 128-byte copy and one synchronisation, so its time is the
kernel's plus that fixed part; the HBM figure below is therefore bytes / CALL time, a lower bound of the kernel's own: bytes = 2 arrays x passes x n x itemsize,
against the 8 TB/s of the MI355X's HBM.  The four ways are compared on their numbers before anything is timed.  Nothing is asserted about the times."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="64^3 / 64 x 64 x 32: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_quality_timing.txt"))
    args = ap.parse_args()
    import torch
    import sz_amd
    from sz_amd.fields import s_field
    if not torch.cuda.is_available():
        raise SystemExit("quality_timing.py measures on the GPU; there is none here")
    ctx = sz_amd.HipContext(0)
    lines = [f"tools/quality_timing.py --rounds {args.rounds} --warmup {args.warmup}: {torch.cuda.get_device_name(0)}",
             "ms per call: min / median / max over the rounds; GB/s and share of the 8 TB/s HBM peak from the median (bytes = 2 arrays x passes x n x itemsize)", ""]

    def pairs():
        e = 64 if args.small else 512
        x = torch.from_numpy(s_field(e, e, e, np.float32)).cuda()
        g = torch.Generator(device="cuda").manual_seed(1)
        yield f"{e}^3 float32", np.float32, x, x + 1e-4 * (2 * torch.rand(x.shape, generator=g, device="cuda", dtype=torch.float32) - 1)
        shape = (64, 64, 32) if args.small else (1024, 1024, 512)
        x = torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) + 3.0
        d = x + 1e-6 * (2 * torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) - 1)
        yield "x".join(map(str, shape)) + " float64", np.float64, x, d

    for name, dt, x, d in pairs():
        n, isz = x.numel(), x.element_size()
        torch.cuda.synchronize()

        def fused(corr=False):
            return ctx.compare(x.data_ptr(), d.data_ptr(), True, n, dt, 1e-4, -1.0, corr=corr)

        def composed():
            err = (d - x).abs()
            mx = float(err.max().item())
            mse = float((err * err).double().sum().item()) / n
            rng = float((x.max() - x.min()).item())
            return mx, mse, rng

        def host():
            xo, do = x.cpu().numpy().reshape(-1), d.cpu().numpy().reshape(-1)
            err = np.abs(do - xo)
            return float(err.max()), float(np.dot(err.astype(np.float64), err.astype(np.float64))) / n, float(xo.max() - xo.min())

        q, qc, (mx, mse, rng), (hmx, hmse, hrng) = fused(), fused(True), composed(), host()
        assert q.max_abs_err == mx == hmx and q.range == rng == hrng, (q, mx, hmx, rng, hrng)
        assert abs(q.mse - mse) <= 1e-6 * mse and abs(q.mse - hmse) <= 1e-6 * mse and qc.sum_err_sq == q.sum_err_sq and fused().raw == q.raw
        ways = {"fused": (fused, 1), "fused+corr": (lambda: fused(True), 2), "torch": (composed, None)}
        for f, _ in ways.values():
            for _ in range(args.warmup):
                f()
        times = {k: [] for k in ways}
        for _ in range(args.rounds):
            for k, (f, _) in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        times["host"] = []
        for _ in range(args.host_rounds):
            t0 = time.perf_counter()
            host()
            times["host"].append((time.perf_counter() - t0) * 1e3)
        lines.append(f"{name}: n = {n}, {2 * n * isz / 2 ** 20:.0f} MiB in the two arrays; PSNR {q.psnr:.6f}, max abs err {q.max_abs_err:.6g}, acEff {qc.ac_eff:.12f}")
        for k, t in times.items():
            if not t:
                continue
            med = statistics.median(t)
            row = f"  {k:<11s} {min(t):9.3f} / {med:9.3f} / {max(t):9.3f} ms"
            passes = ways[k][1] if k in ways else None
            if passes:
                rate = 2 * passes * n * isz / (med * 1e-3)
                row += f"   {rate / 1e9:8.1f} GB/s = {100 * rate / HBM_PEAK:5.1f} % of the HBM peak ({passes} pass{'es' if passes > 1 else ''})"
            lines.append(row)
        f_med = statistics.median(times["fused"])
        lines.append(f"  torch / fused = {statistics.median(times['torch']) / f_med:.2f} x" + (f", host / fused = {statistics.median(times['host']) / f_med:.0f} x" if times["host"] else ""))
        lines.append("")
        del x, d
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
