#!/usr/bin/env python3
"""Speed and memory of a masked-loss training step on the SSIM map (ssim_amd.torch_ops.ssim_map, whose backward is
rmgr_ssim_hip_enqueue_ssimf_map_grad) next to the plain-mean step of the same shape (SSIMLoss: the uniform-k gradient kernel) and the
float32 conv2d composite with autograd that users of a per-pixel weight build today.

usage (GPU box):  python tools/ssimw_probe.py [--reps N] [--composite-reps N]
    Shapes (8, 3, 1080, 1920) and (32, 3, 512, 512), float32, gradient for x only, weights w = a 0 / 1 mask of about half the pixels
    times uniform [0, 1).  Three steps, warmed up, then timed in turn in the same process over N steps between events, three rounds:
      map        loss = 1 - (w * ssim_map(x, y)).sum() / w.sum();  loss.backward()
      mean       loss = SSIMLoss()(x, y);                           loss.backward()
      composite  the same masked loss on the map of five grouped conv2d of replicate-padded planes
    and, apart, the two backward kernels alone through autograd.grad on a kept forward (map: grad_outputs = w; mean: grad_outputs of
    one value per plane).  Per step: ms (best of three, and all three), the spread (max - min) / min, and the peak extra memory
    (torch.cuda.max_memory_allocated above what is held before the step).  Prints one JSON line.
torch is imported before the library, so that the process holds one HIP runtime.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 3, 1080, 1920), (32, 3, 512, 512)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(ts):
    return round((max(ts) - min(ts)) / min(ts), 4)


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def composite_map(x, y, win, c1, c2):
    def G(t):
        return F.conv2d(F.pad(t, (5, 5, 5, 5), mode="replicate"), win, groups=t.shape[1])
    mx, my = G(x), G(y)
    sxx, syy, sxy = G(x * x) - mx * mx, G(y * y) - my * my, G(x * y) - mx * my
    return (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--composite-reps", type=int, default=3)
    args = ap.parse_args()
    import ssim_amd
    from ssim_amd import torch_ops
    if not torch.cuda.is_available() or ssim_amd.device_count() < 1:
        raise SystemExit("ssimw_probe: needs the MI355X (no CPU fallback)")
    torch.cuda.set_stream(torch.cuda.Stream())          # one explicit stream for torch and the library
    result = {}
    i = torch.arange(-5, 6, dtype=torch.float64)
    g1 = torch.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    g1 = (g1 / g1.sum()).float().cuda()
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    for shape in SHAPES:
        torch.manual_seed(5)
        y = torch.rand(shape, device="cuda")
        x = (y + 0.05 * torch.randn(shape, device="cuda")).clamp_(0, 1).requires_grad_(True)
        w = torch.rand(shape, device="cuda") * (torch.rand(shape, device="cuda") < 0.5)
        wsum = w.sum()
        win = (g1[:, None] * g1[None, :]).expand(shape[1], 1, 11, 11).contiguous()
        loss_f = torch_ops.SSIMLoss()

        def step_map():
            x.grad = None
            (1.0 - (w * torch_ops.ssim_map(x, y)).sum() / wsum).backward()

        def step_mean():
            x.grad = None
            loss_f(x, y).backward()

        def step_composite():
            x.grad = None
            (1.0 - (w * composite_map(x, y, win, c1, c2)).sum() / wsum).backward()
        # the two maps agree, and so do the gradients of the masked loss
        step_map()
        gm = x.grad.clone()
        step_composite()
        e = float((x.grad - gm).abs().max() / gm.abs().max())
        assert e < 1e-2, e
        row = {"composite_gradient_differs_by": e}
        del gm
        kept_map, kept_mean = torch_ops.ssim_map(x, y), torch_ops.ssim(x, y)
        per_plane = torch.full(kept_mean.shape, -1.0 / kept_mean.numel(), device="cuda")
        fns = [("map", step_map, args.reps), ("mean", step_mean, args.reps), ("composite", step_composite, args.composite_reps),
               ("map_backward", lambda: torch.autograd.grad(kept_map, x, grad_outputs=w, retain_graph=True), args.reps),
               ("mean_backward", lambda: torch.autograd.grad(kept_mean, x, grad_outputs=per_plane, retain_graph=True), args.reps)]
        for _, fn, _ in fns:
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in fns}
        for _ in range(3):
            for name, fn, reps in fns:
                times[name].append(timed(fn, reps))
        del kept_map, kept_mean
        for name, fn, _ in fns[:3]:
            x.grad = None
            ts = times[name]
            row[name] = {"step_ms": round(min(ts), 3), "peak_extra_mb": round(peak_extra(fn) / 2.0 ** 20, 1), "spread": spread(ts),
                         "step_ms_all": [round(t, 3) for t in ts]}
        for name in ("map_backward", "mean_backward"):
            ts = times[name]
            row[name] = {"ms": round(min(ts), 3), "spread": spread(ts), "ms_all": [round(t, 3) for t in ts]}
        row["map_backward_over_mean_backward"] = round(row["map_backward"]["ms"] / row["mean_backward"]["ms"], 3)
        row["map_step_over_mean_step"] = round(row["map"]["step_ms"] / row["mean"]["step_ms"], 3)
        row["composite_over_map_time"] = round(row["composite"]["step_ms"] / row["map"]["step_ms"], 1)
        row["composite_over_map_memory"] = round(row["composite"]["peak_extra_mb"] / row["map"]["peak_extra_mb"], 1)
        result["x".join(str(s) for s in shape)] = row
        del x, y, w, win
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
