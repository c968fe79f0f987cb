#!/usr/bin/env python3
"""Speed of SSIM on 16-bit samples (rmgr_ssim_hip_enqueue_ssim16) next to MODE_SEPARABLE 8-bit SSIM on the same shapes.

usage (GPU box):  python tools/ssim16_probe.py [--reps N]
    Device-resident batches: 32 x 4096^2 at 16 bits without a map, 2 x 8192^2 at 16 bits with a map, 128 x 1920x1080 at 10 bits
    without a map.  The 16-bit pairs are seeded noise uploaded once per image (every pair in buffers of its own); the 8-bit pairs
    are rmgr_ssim_hip_synth_pair_device's, with a map where the 16-bit shape has one.  After a warm-up of both, the two are timed
    alternately in the same process, each over N enqueues between HIP events on the context's stream.  Prints one JSON line: ms per
    batch and Mpix/s per shape, and the 16-bit / 8-bit time ratio.
Kernel time in a run of its own:
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o s16 -- python tools/ssim16_probe.py --reps 3
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 4096, 32, 16, False), (8192, 8192, 2, 16, True), (1920, 1080, 128, 10, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import ssim_amd
    if ssim_amd.device_count() < 1:
        raise SystemExit("ssim16_probe: needs the MI355X (no CPU fallback)")
    hip = ctypes.CDLL("libamdhip64.so")
    vp = ctypes.c_void_p
    stream = vp()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    ctx = ssim_amd.Context(0, stream=stream, mode=ssim_amd.MODE_SEPARABLE)
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
    rng = np.random.default_rng(16)
    for (w, h, n, depth, with_map) in SHAPES:
        L = (1 << depth) - 1
        a = rng.integers(0, L + 1, (h, w)).astype(np.uint16)
        b = np.clip(a.astype(np.int64) + rng.integers(-L // 64, L // 64 + 1, (h, w)), 0, L).astype(np.uint16)
        bufs = []
        p16 = (ssim_amd.Params16 * n)()
        p8 = (ssim_amd.Params * n)()
        for i in range(n):
            da, db = ctx.upload(a), ctx.upload(b)
            ma = ctx.alloc(w * h * 4) if with_map else None
            p16[i] = ssim_amd.make_params16(w, h, da.ptr, 1, w, db.ptr, 1, w, ma.ptr if ma else None)
            ea, eb = ctx.alloc(w * h), ctx.alloc(w * h)
            ctx.synth_pair(ea.ptr, w, eb.ptr, w, w, h, 0x5EED + i)
            mb = ctx.alloc(w * h * 4) if with_map else None
            p8[i] = ssim_amd.make_params(w, h, ea.ptr, 1, w, eb.ptr, 1, w, mb.ptr if mb else None)
            bufs += [x for x in (da, db, ma, ea, eb, mb) if x is not None]
        sums = ctx.alloc(8 * n)
        ctx.synchronize()

        def s16():
            ctx.enqueue_ssim16(p16, n, depth, sums.ptr)

        def s8():
            ctx.enqueue_batch(p8, n, sums.ptr)
        for _ in range(3):
            s16()
            s8()
        ctx.synchronize()
        t16, t8 = [], []
        for _ in range(3):                       # alternated, best of three each
            t16.append(timed(s16, args.reps))
            t8.append(timed(s8, args.reps))
        m16, m8 = min(t16), min(t8)
        px = float(w) * h * n
        key = "%dx%dx%d_d%d%s" % (n, w, h, depth, "_map" if with_map else "")
        result[key] = {"ssim16_ms": round(m16, 3), "separable8_ms": round(m8, 3), "ratio": round(m16 / m8, 3),
                       "ssim16_mpix_s": round(px / m16 / 1e3, 1), "separable8_mpix_s": round(px / m8 / 1e3, 1),
                       "ssim16_ms_all": [round(t, 3) for t in t16], "separable8_ms_all": [round(t, 3) for t in t8]}
        for bfr in bufs:
            bfr.free()
        sums.free()
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
