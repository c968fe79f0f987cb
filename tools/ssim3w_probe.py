#!/usr/bin/env python3
"""Speed of a masked-mean training step through the differentiable 3-D SSIM map (ssim_amd.torch_ops.ssim3d_map,
rmgr_ssim_hip_enqueue_ssim3f and _ssim3f_map_grad) next to the two things a user has without it: the plain-mean step of ssim3d on the same
tensors (the parent path: the map gradient reads 4 more bytes per voxel and the step carries the map and its product with the mask, so
near parity is the expectation, not a gain), and the float32 composite with the same mask -- replicate padding, one 1-D conv3d per axis on
each of the five statistics, autograd.

usage (GPU box):  python tools/ssim3w_probe.py [--reps N] [--out FILE]
    Shapes, device-resident: (1, 1, 512, 512, 512), (4, 1, 128, 128, 128).  For each: a forward + backward step (gradient for x) of the
    three candidates in the same process, warmed up, then timed in turn between two events, three rounds, ALTERNATED.  Per candidate: ms
    (best of three, and all three), the spread (max - min) / min, and the peak of torch's allocator over one step.
    Prints one JSON line (and writes it to FILE).
torch is imported before the library, so that the process holds one HIP runtime.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 1, 512, 512, 512), (4, 1, 128, 128, 128)]


def spread(ts):
    return round((max(ts) - min(ts)) / min(ts), 4)


def probe(torch, shape, reps):
    import torch.nn.functional as F
    import ssim3f_model as S
    from ssim_amd import torch_ops
    torch.manual_seed(5)
    y = torch.rand(shape, device="cuda")
    x = (y + 0.05 * torch.randn(shape, device="cuda")).clamp_(0, 1).requires_grad_(True)
    mask = (torch.rand(shape, device="cuda") < 0.5).float()          # about half the voxels count
    inside = mask.sum()
    g1 = torch.tensor(S.gaussian_taps(), dtype=torch.float32, device="cuda")
    kx, ky, kz = g1.reshape(1, 1, 1, 1, 11), g1.reshape(1, 1, 1, 11, 1), g1.reshape(1, 1, 11, 1, 1)
    c1, c2 = 0.01 ** 2, 0.03 ** 2

    def G(t):
        t = F.conv3d(F.pad(t, (5, 5, 0, 0, 0, 0), mode="replicate"), kx)
        t = F.conv3d(F.pad(t, (0, 0, 5, 5, 0, 0), mode="replicate"), ky)
        return F.conv3d(F.pad(t, (0, 0, 0, 0, 5, 5), mode="replicate"), kz)

    def composite_map(a, b):
        ma, mb = G(a), G(b)
        saa, sbb, sab = G(a * a) - ma * ma, G(b * b) - mb * mb, G(a * b) - ma * mb
        return (2 * ma * mb + c1) * (2 * sab + c2) / ((ma * ma + mb * mb + c1) * (saa + sbb + c2))

    def map_step():
        x.grad = None
        (1.0 - (mask * torch_ops.ssim3d_map(x, y)).sum() / inside).backward()

    def mean_step():
        x.grad = None
        (1.0 - torch_ops.ssim3d(x, y).mean()).backward()

    def composite_step():
        x.grad = None
        (1.0 - (mask * composite_map(x, y)).sum() / inside).backward()

    # the masked steps agree before anything is timed
    map_step()
    gf = x.grad.clone()
    composite_step()
    dg = float((x.grad - gf).abs().max() / gf.abs().max())
    assert dg < 1e-2, (shape, dg)
    del gf

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

    cands = [("map_step", map_step, reps), ("mean_step", mean_step, reps), ("composite_step", composite_step, max(1, reps // 2))]
    for _, fn, _ in cands:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cands}
    for _ in range(3):
        for name, fn, n in cands:
            times[name].append(timed(fn, n))
    row = {name: {"ms": round(min(ts), 3), "spread": spread(ts), "ms_all": [round(t, 3) for t in ts]} for name, ts in times.items()}
    for name, fn, _ in cands:
        row[name]["torch_peak_bytes"] = peak(fn)
    voxels = 1
    for d in shape:
        voxels *= d
    row["map_step"]["library_scratch_bytes_documented"] = 12 * voxels       # one gradient: 3 floats per voxel, as ssim3d's step
    row["map_step_over_mean_step"] = round(row["map_step"]["ms"] / row["mean_step"]["ms"], 3)
    row["composite_over_map_step"] = round(row["composite_step"]["ms"] / row["map_step"]["ms"], 2)
    row["composite_peak_over_map_step_peak"] = round(row["composite_step"]["torch_peak_bytes"] /
                                                     float(row["map_step"]["torch_peak_bytes"] + 12 * voxels), 2)
    row["masked_gradient_differs_by"] = dg
    x.grad = None
    del x, y, mask
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
        raise SystemExit("ssim3w_probe: needs the MI355X (no CPU fallback)")
    torch.cuda.set_stream(torch.cuda.Stream())          # one explicit stream for torch and the library
    result = {"device": torch.cuda.get_device_name(0)}
    for shape in SHAPES:
        result["x".join(str(d) for d in shape)] = probe(torch, shape, args.reps)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
