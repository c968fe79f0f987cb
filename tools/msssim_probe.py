#!/usr/bin/env python3
"""Speed of multi-scale SSIM (rmgr_ssim_hip_compute_msssim_device) next to MODE_SEPARABLE single-scale SSIM on the same batches.

usage (GPU box):  python tools/msssim_probe.py [--reps N]
    Device-resident synthetic pairs (rmgr_ssim_hip_synth_pair_device), 32 x 4096^2 and 128 x 1920x1080, Wang's 5 scales.  After a warm-up
    of every shape, the two computations are timed alternately in the same process, each over N calls between HIP events on the
    context's stream (MS-SSIM calls block and read their results back; SSIM runs through rmgr_ssim_hip_enqueue_batch and one
    synchronize).  Prints one JSON line: ms per call, Mpix/s of scale-0 pixels, and the MS-SSIM / SSIM time ratio, per batch.
Kernel time per kernel and per scale, in a run of its own:
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o ms -- python tools/msssim_probe.py --reps 3
    python tools/msssim_probe.py --summarize OUT/.../ms_kernel_trace.csv     (CPU: groups the trace's dispatches by kernel and grid)
"""
import argparse
import ctypes
import csv
import json
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 4096, 32), (1920, 1080, 128)]


def summarize(path):
    """Mean duration per (kernel, grid) over the trace's dispatches: with one grid per scale, that is the time per kernel and scale."""
    rows = defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "msssim" not in name and "ssim_strip" not in name and "reduce" not in name:
                continue
            grid = r.get("Grid_Size") or r.get("Grid_Size_X") or "?"
            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
            short = name.replace("(anonymous namespace)::", "").split("(")[0]
            rows[(short, grid)].append(dur)
    out = [{"kernel": k, "grid": g, "calls": len(v), "mean_ms": round(sum(v) / len(v), 4)} for (k, g), v in sorted(rows.items(), key=lambda kv: -sum(kv[1]))]
    for o in out:
        print(json.dumps(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--summarize", default=None)
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize)
        return
    import ssim_amd
    if ssim_amd.device_count() < 1:
        raise SystemExit("msssim_probe: needs the MI355X (no CPU fallback)")
    hip = ctypes.CDLL("libamdhip64.so")
    vp = ctypes.c_void_p
    stream = vp()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    ctx = ssim_amd.Context(0, stream=stream)
    ev0, ev1 = vp(), vp()
    assert hip.hipEventCreate(ctypes.byref(ev0)) == 0 and hip.hipEventCreate(ctypes.byref(ev1)) == 0
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]

    def timed(fn, reps):
        assert hip.hipEventRecord(ev0, stream) == 0
        for _ in range(reps):
            fn()
        assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), ev0, ev1) == 0
        return ms.value / reps

    result = {"device": ctx.describe()}
    for (w, h, n) in SHAPES:
        bufs = []
        params = (ssim_amd.Params * n)()
        for i in range(n):
            da, db = ctx.alloc(w * h), ctx.alloc(w * h)
            ctx.synth_pair(da.ptr, w, db.ptr, w, w, h, 0x5EED + i)
            bufs += [da, db]
            params[i] = ssim_amd.make_params(w, h, da.ptr, 1, w, db.ptr, 1, w)
        sums = ctx.alloc(8 * n)
        ctx.synchronize()

        def msssim():
            ctx.msssim_device(params, n)

        def ssim():
            ctx.enqueue_batch(params, n, sums.ptr)
        ctx.set_mode(ssim_amd.MODE_SEPARABLE)
        for _ in range(3):
            msssim()
            ssim()
        ctx.synchronize()
        t_ms, t_ss = [], []
        for _ in range(3):                       # alternated, best of three each
            t_ms.append(timed(msssim, args.reps))
            t_ss.append(timed(ssim, args.reps))
        ms, ss = min(t_ms), min(t_ss)
        px = float(w) * h * n
        key = "%dx%dx%d" % (n, w, h)
        result[key] = {"msssim_ms": round(ms, 3), "ssim_separable_ms": round(ss, 3), "ratio": round(ms / ss, 3),
                       "msssim_mpix_s": round(px / ms / 1e3, 1), "ssim_separable_mpix_s": round(px / ss / 1e3, 1),
                       "msssim_ms_all": [round(t, 3) for t in t_ms], "ssim_ms_all": [round(t, 3) for t in t_ss]}
        for bfr in bufs:
            bfr.free()
        sums.free()
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
