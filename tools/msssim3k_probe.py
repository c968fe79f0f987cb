#!/usr/bin/env python3
"""Speed of multi-scale SSIM of volumes under a caller-chosen window (ssim_amd.torch_ops.ms_ssim3d_amp / MSSSIM3DLoss with win_size,
win_sigma, window: the rmgr_ssim_hip_*_msssim3f_win* and *_msssim3h_win* entries) next to the fixed-window call on the same batch.

usage (GPU box):  python tools/msssim3k_probe.py [--reps N] [--default-only] [--root DIR] [--shapes 256,128]
    Batches.  (1, 1, 256, 256, 256) and (4, 1, 128, 128, 128), seeded noise pairs, float32 and bfloat16, Wang's 5 scales, data range 1.
    Rows.  Per batch, dtype and window -- the 3-tap box, the 7-tap box, 7 Gaussian 1.5 --: the forward (no autograd) and a training step
    (loss = MSSSIM3DLoss(...)(x, y); loss.backward(), gradient for x only), each timed alternately with the fixed-window call of the same
    kind on the same tensors in the same process: after three warm-up calls of both, three rounds of N calls each between events on the
    current stream.  Reported per row: the best and the worst of the three rounds of both (ms per call -- the spread), and the ratio of
    the two best.
    --default-only times the fixed-window call alone (best and worst of three rounds), through keyword-free calls, so that the same file
    runs against another checkout of the package: --root DIR imports ssim_amd from DIR.  The fixed-window kernels' device code does not
    depend on this interface, so two checkouts timed in one session should agree within the rounds' spread.
    Prints one JSON line.
torch is imported before the library, so that the process holds one HIP runtime.
"""
import argparse
import json
import os
import sys

import torch

WINDOWS = (("3 box", dict(win_size=3, window="uniform")), ("7 box", dict(win_size=7, window="uniform")), ("7 Gaussian 1.5", dict(win_size=7)))
SHAPES = {"256": (1, 256), "128": (4, 128)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fa, fb, reps):
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(3):
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    return ta, tb


def spread(ts):
    return {"best_ms": round(min(ts), 4), "worst_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--shapes", default="256,128")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from ssim_amd import torch_ops

    result = {"root": os.path.abspath(args.root), "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": []}
    for shape in args.shapes.split(","):
        n, side = SHAPES[shape]
        for dtype in (torch.float32, torch.bfloat16):
            g = torch.Generator(device="cuda").manual_seed(16)
            x = torch.rand((n, 1, side, side, side), device="cuda", generator=g)
            y = (x + 0.05 * torch.randn((n, 1, side, side, side), device="cuda", generator=g)).clamp_(0, 1)
            x, y = x.to(dtype), y.to(dtype)
            xg = x.clone().requires_grad_(True)

            def forward(**kw):
                with torch.no_grad():
                    return torch_ops.ms_ssim3d_amp(x, y, **kw)

            def step(loss_fn):
                xg.grad = None
                loss_fn(xg, y).backward()

            fixed_loss = torch_ops.MSSSIM3DLoss()
            base = {"shape": "(%d, 1, %d, %d, %d)" % (n, side, side, side), "dtype": str(dtype).replace("torch.", "")}
            if args.default_only:
                ta, tb = alternate(forward, lambda: step(fixed_loss), args.reps)
                result["rows"].append(dict(base, window="fixed", forward=spread(ta), training_step=spread(tb)))
                continue
            for name, kw in WINDOWS:
                loss = torch_ops.MSSSIM3DLoss(**kw)
                tw, tf = alternate(lambda: forward(**kw), forward, args.reps)
                sw, sf = alternate(lambda: step(loss), lambda: step(fixed_loss), args.reps)
                result["rows"].append(dict(base, window=name, forward=spread(tw), forward_fixed=spread(tf),
                                           forward_ratio=round(min(tw) / min(tf), 3), training_step=spread(sw), training_step_fixed=spread(sf),
                                           training_step_ratio=round(min(sw) / min(sf), 3)))
            del x, y, xg
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
