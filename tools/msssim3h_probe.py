#!/usr/bin/env python3
"""Speed and memory of the 16-bit multi-scale volume path (ssim_amd.torch_ops.ms_ssim3d_amp / MSSSIM3DLoss on bfloat16 tensors,
rmgr_ssim_hip_enqueue_msssim3h and _msssim3h_grad) next to what a user had without it: MSSSIM3DLoss()(x.float(), y.float()), the float32
path on widened copies, whose float32 gradient autograd casts back.  Only scale 0 differs between the two routes -- its input reads and
its gradient writes halve, the walks are VALU- and LDS-bound and the 12 / 16 bytes per voxel of coefficient traffic stay -- so the
expectation is parity in the forward, and in torch memory 2 bytes per voxel of x for the gradient where the widened route holds two
float32 copies and a float32 gradient (12 bytes) and its cast.  No figure here is a pass criterion.

usage (GPU box):  python tools/msssim3h_probe.py [--reps N] [--out FILE]
    Shapes, device-resident: (1, 1, 256, 256, 256), (4, 1, 128, 128, 128), (16, 1, 64, 64, 64); Wang's five scales.  For each, in the
    same process, warmed up, three rounds, ALTERNATED between two events:
      forward        ms_ssim3d_amp(x, y) on bfloat16 tensors against ms_ssim3d(xf, yf) on their float32 widenings made beforehand
      step           MSSSIM3DLoss()(x, y).backward(), gradient for x, against MSSSIM3DLoss()(x.float(), y.float()).backward()
    Per candidate: ms (best of three, and all three), the spread (max - min) / min, and for the steps the peak of torch's allocator.
    Prints one JSON line (and writes it to FILE; profiles/msssim3h_probe.json is where the README quotes it from).
torch is imported before the library, so that the process holds one HIP runtime.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 1, 256, 256, 256), (4, 1, 128, 128, 128), (16, 1, 64, 64, 64)]


def spread(ts):
    return round((max(ts) - min(ts)) / min(ts), 4)


def probe(torch, shape, reps):
    from ssim_amd import torch_ops
    torch.manual_seed(5)
    yf = torch.rand(shape, device="cuda")
    xf = (yf + 0.05 * torch.randn(shape, device="cuda")).clamp_(0, 1)
    x, y = xf.to(torch.bfloat16).requires_grad_(True), yf.to(torch.bfloat16)
    xf, yf = x.detach().float(), y.float()                                   # the widened volumes: the same samples
    loss = torch_ops.MSSSIM3DLoss()

    # the two routes agree before anything is timed: the value bit for bit, the gradient after the cast autograd applies
    assert torch.equal(torch_ops.ms_ssim3d_amp(x.detach(), y), torch_ops.ms_ssim3d(xf, yf))
    loss(x, y).backward()
    g16, x.grad = x.grad, None
    loss(x.float(), y.float()).backward()
    assert g16.dtype == torch.bfloat16 and torch.equal(g16, x.grad)
    x.grad = None
    del g16

    def forward_16():
        torch_ops.ms_ssim3d_amp(x.detach(), y)

    def forward_32():
        torch_ops.ms_ssim3d(xf, yf)

    def step_16():
        x.grad = None
        loss(x, y).backward()

    def step_widened():
        x.grad = None
        loss(x.float(), y.float()).backward()

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

    cands = [("forward_16", forward_16), ("forward_float32", forward_32), ("step_16", step_16), ("step_widened", step_widened)]
    for _, fn in cands:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cands}
    for _ in range(3):
        for name, fn in cands:
            times[name].append(timed(fn, reps))
    row = {name: {"ms": round(min(ts), 3), "spread": spread(ts), "ms_all": [round(t, 3) for t in ts]} for name, ts in times.items()}
    for name, fn in cands[2:]:
        row[name]["torch_peak_bytes"] = peak(fn)
    voxels = 1
    for d in shape:
        voxels *= d
    row["torch_peak_bytes_per_voxel"] = {name: round(row[name]["torch_peak_bytes"] / float(voxels), 2) for name, _ in cands[2:]}
    row["forward_16_over_float32"] = round(row["forward_16"]["ms"] / row["forward_float32"]["ms"], 3)
    row["step_16_over_widened"] = round(row["step_16"]["ms"] / row["step_widened"]["ms"], 3)
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
        raise SystemExit("msssim3h_probe: needs the MI355X (no CPU fallback)")
    torch.cuda.set_stream(torch.cuda.Stream())          # one explicit stream for torch and the library
    result = {"device": torch.cuda.get_device_name(0), "scales": 5}
    for shape in SHAPES:
        result["x".join(str(d) for d in shape)] = probe(torch, shape, args.reps)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
