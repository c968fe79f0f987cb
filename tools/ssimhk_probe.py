#!/usr/bin/env python3
"""Speed and memory of the 16-bit 2-D path under a caller-chosen window (ssim_amd.torch_ops.ssim_amp / SSIMLoss on bfloat16 tensors with
win_size / window; rmgr_ssim_hip_enqueue_ssimh_win and _ssimh_win_grad) next to the two things a user had without it: the float32
windowed path on widened copies -- SSIMLoss(win_size=7)(x.float(), y.float()), whose float32 gradient autograd casts back -- and the
fixed-window 16-bit path on the same tensors.  The strip kernels are VALU- and LDS-bound, so the expectation is a forward near the
float32 windowed path, and a step that holds 2 bytes of torch memory per pixel of x where the widened route holds 12.  An expectation
only: the figures are whatever this prints.

usage (GPU box):  python tools/ssimhk_probe.py [--reps N] [--out FILE]
    Shapes, device-resident: (128, 1, 1080, 1920), (32, 1, 4096, 4096).  Windows: the 3-tap box, the 7-tap box, 7 Gaussian 1.5.  For each
    shape and window, in the same process, warmed up, three rounds, ALTERNATED between two events:
      forward        ssim_amp(x, y, window) on bfloat16 tensors; ssim(xf, yf, window) on their float32 widenings made beforehand;
                     ssim_amp(x, y) under the fixed window on the same bfloat16 tensors
      step           SSIMLoss(window)(x, y).backward(), gradient for x; the same on x.float(), y.float(); SSIMLoss()(x, y).backward()
    Per candidate: ms (best of three, and all three), the spread (max - min) / min, and for the steps the peak of torch's allocator,
    also per pixel of x.  Prints one JSON line (and writes it to FILE).
torch is imported before the library, so that the process holds one HIP runtime.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 1, 1080, 1920), (32, 1, 4096, 4096)]
WINDOWS = [("3 box", dict(win_size=3, window="uniform")), ("7 box", dict(win_size=7, window="uniform")), ("7 Gaussian 1.5", dict(win_size=7, win_sigma=1.5))]


def spread(ts):
    return round((max(ts) - min(ts)) / min(ts), 4)


def probe(torch, shape, kw, reps):
    from ssim_amd import torch_ops
    torch.manual_seed(5)
    yf = torch.rand(shape, device="cuda")
    xf = (yf + 0.05 * torch.randn(shape, device="cuda")).clamp_(0, 1)
    x, y = xf.to(torch.bfloat16).requires_grad_(True), yf.to(torch.bfloat16)
    xf, yf = x.detach().float(), y.float()                                   # the widened planes: the same samples
    loss, fixed = torch_ops.SSIMLoss(**kw), torch_ops.SSIMLoss()

    # the two routes agree before anything is timed: the value bit for bit
    assert torch.equal(torch_ops.ssim_amp(x.detach(), y, **kw), torch_ops.ssim(xf, yf, **kw))

    def forward_16():
        torch_ops.ssim_amp(x.detach(), y, **kw)

    def forward_32():
        torch_ops.ssim(xf, yf, **kw)

    def forward_16_fixed():
        torch_ops.ssim_amp(x.detach(), y)

    def step_16():
        x.grad = None
        loss(x, y).backward()

    def step_widened():
        x.grad = None
        loss(x.float(), y.float()).backward()

    def step_16_fixed():
        x.grad = None
        fixed(x, y).backward()

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def peak(fn):
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    cands = [("forward_16", forward_16), ("forward_float32", forward_32), ("forward_16_fixed_window", forward_16_fixed),
             ("step_16", step_16), ("step_widened", step_widened), ("step_16_fixed_window", step_16_fixed)]
    for _, fn in cands:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cands}
    for _ in range(3):
        for name, fn in cands:
            times[name].append(timed(fn, reps))
    row = {name: {"ms": round(min(ts), 3), "spread": spread(ts), "ms_all": [round(t, 3) for t in ts]} for name, ts in times.items()}
    for name, fn in cands[3:]:
        row[name]["torch_peak_bytes"] = peak(fn)
    pixels = 1
    for d in shape:
        pixels *= d
    row["torch_peak_bytes_per_pixel"] = {name: round(row[name]["torch_peak_bytes"] / float(pixels), 2) for name, _ in cands[3:]}
    row["forward_16_over_float32"] = round(row["forward_16"]["ms"] / row["forward_float32"]["ms"], 3)
    row["forward_16_over_fixed_window"] = round(row["forward_16"]["ms"] / row["forward_16_fixed_window"]["ms"], 3)
    row["step_16_over_widened"] = round(row["step_16"]["ms"] / row["step_widened"]["ms"], 3)
    row["step_16_over_fixed_window"] = round(row["step_16"]["ms"] / row["step_16_fixed_window"]["ms"], 3)
    x.grad = None
    del x, y, xf, yf
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import ssim_amd
    if not torch.cuda.is_available() or ssim_amd.device_count() < 1:
        raise SystemExit("ssimhk_probe: needs the MI355X (no CPU fallback)")
    torch.cuda.set_stream(torch.cuda.Stream())          # one explicit stream for torch and the library
    result = {"device": torch.cuda.get_device_name(0), "dtype": "bfloat16"}
    for shape in SHAPES:
        key = "x".join(str(d) for d in shape)
        result[key] = {}
        for name, kw in WINDOWS:
            result[key][name] = probe(torch, shape, kw, args.reps)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
