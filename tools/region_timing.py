#!/usr/bin/env python3
"""What a sub-box read of an OpenMP-container stream costs beside the full decode (GPU box; writes profiles/r12_region_timing.json).

The bench's 512^3 float32 S-field at ABS 1e-4, thread_num 4096 (boxes of 32^3), stream and output device-resident.  Three calls, taken in turn in one loop so
that they share whatever else the machine is doing:
  full    szhip_decompress_omp of the whole array (the yardstick: the code of the full decode is untouched by the region call)
  crop    szhip_decompress_omp_region of the 64^3 region at (100, 200, 300): 27 boxes, staging array + k_omp_crop
  direct  the box-aligned 64^3 region at (128, 192, 320): 8 boxes, written by the sweep itself
Per call: the host's clock around it (every call ends in a synchronisation of its stream) and the device-event times the library reports in szhip_stats --
ms_entropy (stream intake .. end of the Huffman decode) and ms_quant (the inverse sweep, and the crop behind it).  Nothing is asserted about the times; the
regions are compared with the crop of the full decode before anything is timed."""
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
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_region_timing.json"))
    args = ap.parse_args()
    import torch
    import sz_amd
    from sz_amd.fields import s_field
    if not torch.cuda.is_available():
        raise SystemExit("region_timing.py measures on the GPU; there is none here")
    n, eb = args.edge, 1e-4
    boxes = (n // 32) ** 3
    # (smaller edges: the regions scaled down, for rehearsals)
    regions = {"crop": ((100, 200, 300), 64), "direct": ((128, 192, 320), 64)} if n >= 512 else {"crop": ((n // 8 + 4, n // 4 + 8, n // 2 + 12), n // 8), "direct": ((n // 4, n // 4, n // 2), n // 8)}
    x = torch.from_numpy(s_field(n, n, n, np.float32)).cuda()
    ctx = sz_amd.HipContext(0)
    meta = sz_amd.make_meta(np.float32, err_mode=sz_amd.ABS, abs_bound=eb)
    meta = bytes([meta[0], meta[1], meta[2], 0xC0]) + bytes(meta[4:])
    blob, osize, _ = ctx.compress_omp(x.data_ptr(), True, (n, n, n), np.float32, eb, boxes, meta)
    stream = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()     # the caller's own device buffer, not the context's
    torch.cuda.synchronize()
    full = torch.empty_like(x)
    outs = {k: torch.empty((e, e, e), dtype=torch.float32, device="cuda") for k, (_, e) in regions.items()}

    def call(kind):
        t0 = time.perf_counter()
        if kind == "full":
            st = ctx.decompress_omp(stream.data_ptr(), True, osize, len(meta), (n, n, n), np.float32, full.data_ptr(), True)
        else:
            lo, e = regions[kind]
            st = ctx.decompress_omp_region(stream.data_ptr(), True, osize, len(meta), (n, n, n), np.float32, lo, tuple(v + e for v in lo), outs[kind].data_ptr(), True)
        return (time.perf_counter() - t0) * 1e3, st

    kinds = ("full", "crop", "direct")
    stats = {}
    for k in kinds:
        _, stats[k] = call(k)
    torch.cuda.synchronize()
    for k, (lo, e) in regions.items():                                       # the regions are the crop of the full decode, bit for bit
        want = full[lo[0]:lo[0] + e, lo[1]:lo[1] + e, lo[2]:lo[2] + e]
        assert torch.equal(outs[k].view(torch.int32), want.contiguous().view(torch.int32)), k
    for _ in range(args.warmup):
        for k in kinds:
            call(k)
    wall = {k: [] for k in kinds}; dev_e = {k: [] for k in kinds}; dev_q = {k: [] for k in kinds}; host = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k in kinds:
            ms, st = call(k)
            wall[k].append(ms); dev_e[k].append(st.ms_entropy); dev_q[k].append(st.ms_quant); host[k].append(st.ms_host)
    res = {"what": f"{n}^3 float32 S-field, ABS {eb}, thread_num {boxes}, stream and output on the device; {args.rounds} rounds of full / crop / direct in turn after "
                   f"{args.warmup} warm-up rounds; medians (min .. max).  wall_ms: host clock around the blocking call; entropy_ms / sweep_ms: the call's device events "
                   "(szhip_stats.ms_entropy: intake to the end of the Huffman decode; ms_quant: the inverse sweep, with the crop where there is one); "
                   "tables_host_ms (region calls; inside the entropy window, during which the device waits for it): the host reading the header and the per-box tables "
                   "off the device stream, walking them and building the compact tables; rest_ms = wall - entropy - sweep: launches behind the events, the final synchronisation",
           "stream_bytes": int(osize), "device": torch.cuda.get_device_name(0), "calls": {}}
    med = lambda v: float(np.median(v))                                      # noqa: E731
    for k in kinds:
        res["calls"][k] = {"region": None if k == "full" else {"lo": list(regions[k][0]), "edge": regions[k][1]},
                           "boxes_decoded": int(stats[k].n_blocks), "values": int(stats[k].n_elements), "quant_kernel": int(stats[k].quant_kernel),
                           "wall_ms": round(med(wall[k]), 4), "wall_ms_min_max": [round(min(wall[k]), 4), round(max(wall[k]), 4)],
                           "entropy_ms": round(med(dev_e[k]), 4), "sweep_ms": round(med(dev_q[k]), 4),
                           "tables_host_ms": None if k == "full" else round(med(host[k]), 4),
                           "rest_ms": round(med(wall[k]) - med(dev_e[k]) - med(dev_q[k]), 4)}
    f = res["calls"]["full"]["wall_ms"]
    res["ratio_to_full_wall"] = {k: round(res["calls"][k]["wall_ms"] / f, 4) for k in ("crop", "direct")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
