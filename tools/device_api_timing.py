#!/usr/bin/env python3
"""What the drop-in calls for device-resident arrays cost beside the calls they are made of (GPU box; writes profiles/r14_device_api_timing.json).

512^3 float32, SZ_BEST_SPEED, arrays and streams device-resident; wall clock around the blocking calls (every call of the library returns when its result is
complete), all calls taken in turn in one loop after a warm-up so that they share whatever else the machine is doing; median, min .. max in ms.
  direct      szhip_compress / szhip_decompress on the S-field at ABS 1e-4, driven as bench.py drives them (range from the fit pass, the stream into a device
              buffer): the same kernels without the drop-in logic
  into        SZ_hip_compress_device_into / SZ_hip_decompress_device with the stream on the device: the new calls
  to_host     SZ_hip_compress_device: plus one device-to-host copy of the stream
  host        SZ_compress_args / SZ_decompress on a host copy: what a caller of the C API had before
  raw_*       standard_normal at ABS 1e-7, which takes the raw store: SZ_hip_compress_device_into / SZ_hip_decompress_device, i.e. szhip_store_be /
              szhip_load_be inside a call
  d2d         hipMemcpyDtoD of the same 512 MB (device events), and szhip_store_be / szhip_load_be alone at the stream's alignment (8 mod 16) and at 0 mod 16
              (device events around the blocking entry): the yardstick for a copy-shaped kernel
Streams and decoded values are compared before anything is timed; nothing is asserted about the times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_device_api_timing.json"))
    args = ap.parse_args()
    import ctypes
    import torch
    import sz_amd
    import ref_cases
    from sz_amd.fields import s_field
    if not torch.cuda.is_available():
        raise SystemExit("device_api_timing.py measures on the GPU; there is none here")
    n, eb, f32 = args.edge, 1e-4, np.float32
    shape, nbytes = (n, n, n), n * n * n * 4
    cfg = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"device_api_timing_{os.getpid()}.config")
    ref_cases.write_config(cfg, {})
    assert sz_amd.SZ_Init(cfg) == 0
    xs_host = s_field(n, n, n, f32)
    xr_host = np.random.default_rng(5).standard_normal(shape).astype(f32)
    xs, xr = torch.from_numpy(xs_host).cuda(), torch.from_numpy(xr_host).cuda()
    dec = torch.empty_like(xs)
    cap = nbytes + 4096
    sbuf = torch.empty(cap, dtype=torch.uint8, device="cuda")          # the S-field's stream
    rbuf = torch.empty(cap, dtype=torch.uint8, device="cuda")          # the raw stream
    torch.cuda.synchronize()
    A = (sz_amd.ABS, eb, 0.0, 0.0)
    R = (sz_amd.ABS, 1e-7, 0.0, 0.0)

    # ---- the bar, before any timing
    want = sz_amd.SZ_compress_args(xs_host, *A)
    slen = sz_amd.SZ_hip_compress_device_into(xs.data_ptr(), shape, f32, sbuf.data_ptr(), cap, *A)
    assert bytes(sbuf[:slen].cpu().numpy()) == want and sz_amd.SZ_hip_compress_device(xs.data_ptr(), shape, f32, *A) == want
    want_dec = sz_amd.SZ_decompress(want, shape, f32)
    sz_amd.SZ_hip_decompress_device(sbuf.data_ptr(), True, slen, dec.data_ptr(), shape, f32)
    assert np.array_equal(dec.cpu().numpy().view(np.uint32), want_dec.view(np.uint32))
    rlen = sz_amd.SZ_hip_compress_device_into(xr.data_ptr(), shape, f32, rbuf.data_ptr(), cap, *R)
    raw = bytes(rbuf[:rlen].cpu().numpy())
    assert raw[3] == 0x50 and rlen == 40 + nbytes and raw == sz_amd.SZ_compress_args(xr_host, *R)
    sz_amd.SZ_hip_decompress_device(rbuf.data_ptr(), True, rlen, dec.data_ptr(), shape, f32)
    assert torch.equal(dec.view(torch.int32), xr.view(torch.int32))

    ctx = sz_amd.HipContext(0)
    meta = sz_amd.make_meta(f32, err_mode=sz_amd.ABS, abs_bound=eb, vmin=0.0, vmax=0.0)
    prm = sz_amd.szhip_params(100, 0.99, 65536, 0, 1)
    dbuf = torch.empty(cap, dtype=torch.uint8, device="cuda")

    def direct_compress():
        out, nn, st = ctypes.c_void_p(dbuf.data_ptr()), ctypes.c_size_t(cap), sz_amd.szhip_stats()
        rc = sz_amd.lib().szhip_compress(ctx._h, 0, xs.data_ptr(), 1, n, n, n, eb, ctypes.byref(prm), meta, len(meta), 2, ctypes.byref(out), ctypes.byref(nn), ctypes.byref(st))
        assert rc == 0

    L = sz_amd.lib()
    want_buf = ctypes.create_string_buffer(want, len(want))

    def host_compress():                                               # (the C calls themselves: no copy of the binding's in the time)
        nn = ctypes.c_size_t(0)
        p = L.SZ_compress_args(0, xs_host.ctypes.data, ctypes.byref(nn), sz_amd.ABS, eb, 0.0, 0.0, 0, 0, n, n, n)
        assert p and nn.value == len(want)
        L.free(p)

    def host_decompress():
        p = L.SZ_decompress(0, want_buf, len(want), 0, 0, n, n, n)
        assert p
        L.free(p)

    calls = {
        "direct_compress": direct_compress,
        "direct_decompress": lambda: ctx.decompress(sbuf.data_ptr(), True, slen, 4 + 28 + 8, shape, f32, dec.data_ptr(), True),
        "into_compress": lambda: sz_amd.SZ_hip_compress_device_into(xs.data_ptr(), shape, f32, sbuf.data_ptr(), cap, *A),
        "into_decompress": lambda: sz_amd.SZ_hip_decompress_device(sbuf.data_ptr(), True, slen, dec.data_ptr(), shape, f32),
        "to_host_compress": lambda: sz_amd.SZ_hip_compress_device(xs.data_ptr(), shape, f32, *A),
        "host_compress": host_compress,
        "host_decompress": host_decompress,
        "raw_into_compress": lambda: sz_amd.SZ_hip_compress_device_into(xr.data_ptr(), shape, f32, rbuf.data_ptr(), cap, *R),
        "raw_into_decompress": lambda: sz_amd.SZ_hip_decompress_device(rbuf.data_ptr(), True, rlen, dec.data_ptr(), shape, f32),
    }
    hip = L                                                            # (the HIP runtime the library itself is linked to)
    hip.hipMemcpyDtoD.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    nval = n * n * n
    evented = {
        "d2d_copy": lambda: hip.hipMemcpyDtoD(dec.data_ptr(), xr.data_ptr(), nbytes),
        "store_be_8mod16": lambda: ctx.store_be(xr.data_ptr(), nval, f32, rbuf.data_ptr() + 40, True),
        "store_be_0mod16": lambda: ctx.store_be(xr.data_ptr(), nval, f32, rbuf.data_ptr() + 48, True),
        "load_be_8mod16": lambda: ctx.load_be(rbuf.data_ptr() + 40, True, nval, f32, dec.data_ptr()),
        "load_be_0mod16": lambda: ctx.load_be(rbuf.data_ptr() + 48, True, nval, f32, dec.data_ptr()),
    }
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in list(calls) + list(evented)}
    for r in range(args.warmup + args.rounds):
        for k, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter(); f(); t1 = time.perf_counter()
            if r >= args.warmup:
                ms[k].append((t1 - t0) * 1e3)
        for k, f in evented.items():
            torch.cuda.synchronize()
            ev0.record(); f(); ev1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                ms[k].append(ev0.elapsed_time(ev1))
    sz_amd.SZ_hip_compress_device_into(xr.data_ptr(), shape, f32, rbuf.data_ptr(), cap, *R)        # (the +48 store left a shifted payload behind)
    med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    mm = {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}
    gbps = {k: round(nbytes / 1e6 / med[k], 1) for k in ms}

    def over(new, old):
        """how far the new call's median lies above the direct call's maximum, beside the direct call's own max - min spread"""
        return {"median_minus_direct_max_ms": round(med[new] - mm[old][1], 4), "direct_spread_ms": round(mm[old][1] - mm[old][0], 4)}

    res = {"what": f"{n}^3 float32, SZ_BEST_SPEED; S-field at ABS {eb} (direct / into / to_host / host), standard_normal at ABS 1e-7 (raw_*: the raw store); arrays and streams on "
                   f"the device; wall clock around the blocking calls ({args.rounds} rounds of all calls in turn after {args.warmup} warm-up rounds), device events for d2d_copy, "
                   "store_be_* and load_be_*; ms",
           "device": torch.cuda.get_device_name(0), "stream_bytes": int(slen), "raw_stream_bytes": int(rlen),
           "median_ms": med, "min_max_ms": mm, "GBps_of_the_array_at_the_median": gbps,
           "new_call_beside_direct": {"compress": over("into_compress", "direct_compress"), "decompress": over("into_decompress", "direct_decompress")},
           "fraction_of_d2d_rate": {k: round(med["d2d_copy"] / med[k], 4) for k in evented if k != "d2d_copy"}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    ctx.close()
    sz_amd.SZ_Finalize()
    os.remove(cfg)


if __name__ == "__main__":
    main()
