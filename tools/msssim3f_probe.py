#!/usr/bin/env python3
"""Speed of multi-scale SSIM of float32 volumes (ssim_amd.torch_ops.ms_ssim3d, rmgr_ssim_hip_enqueue_msssim3f and _msssim3f_grad) next to
single-scale ssim3d on the same tensors and next to the float32 composite users build today: replicate padding to even sizes,
avg_pool3d(2), one 1-D conv3d per axis on each of the five statistics of every scale, and autograd.

usage (GPU box):  python tools/msssim3f_probe.py [--reps N] [--out FILE]
    Shapes, device-resident: (1, 1, 256, 256, 256), (4, 1, 128, 128, 128), (16, 1, 64, 64, 64), Wang's five scales.  For each: the forward
    alone and a forward + backward step (gradient for x) of the three candidates in the same process, warmed up, then timed in turn
    between two events, three rounds, ALTERNATED.  Per candidate: ms (best of three, and all three) and the spread (max - min) / min.
    Prints one JSON line (and writes it to FILE; the committed copy is profiles/msssim3f_probe.json).
torch is imported before the library, so that the process holds one HIP runtime.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 1, 256, 256, 256), (4, 1, 128, 128, 128), (16, 1, 64, 64, 64)]
WANG = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def spread(ts):
    return round((max(ts) - min(ts)) / min(ts), 4)


def probe(torch, shape, reps):
    import torch.nn.functional as F
    import ssim3f_model as S
    from ssim_amd import torch_ops
    torch.manual_seed(5)
    y = torch.rand(shape, device="cuda")
    x = (y + 0.05 * torch.randn(shape, device="cuda")).clamp_(0, 1).requires_grad_(True)
    g1 = torch.tensor(S.gaussian_taps(), dtype=torch.float32, device="cuda")
    kx, ky, kz = g1.reshape(1, 1, 1, 1, 11), g1.reshape(1, 1, 1, 11, 1), g1.reshape(1, 1, 11, 1, 1)
    c1, c2 = 0.01 ** 2, 0.03 ** 2

    def G(t):
        t = F.conv3d(F.pad(t, (5, 5, 0, 0, 0, 0), mode="replicate"), kx)
        t = F.conv3d(F.pad(t, (0, 0, 5, 5, 0, 0), mode="replicate"), ky)
        return F.conv3d(F.pad(t, (0, 0, 0, 0, 5, 5), mode="replicate"), kz)

    def down(t):
        d, h, w = t.shape[-3:]
        return F.avg_pool3d(F.pad(t, (0, w % 2, 0, h % 2, 0, d % 2), mode="replicate"), 2)

    def composite(a, b):
        out = None
        for s, wt in enumerate(WANG):
            if s:
                a, b = down(a), down(b)
            ma, mb = G(a), G(b)
            saa, sbb, sab = G(a * a) - ma * ma, G(b * b) - mb * mb, G(a * b) - ma * mb
            cs = (2 * sab + c2) / (saa + sbb + c2)
            m = cs if s + 1 < len(WANG) else (2 * ma * mb + c1) / (ma * ma + mb * mb + c1) * cs
            term = torch.relu(m.mean(dim=(-3, -2, -1))) ** wt
            out = term if out is None else out * term
        return out

    def forward_of(fn):
        def run():
            with torch.no_grad():
                return fn(x, y)
        return run

    def step_of(fn):
        def run():
            x.grad = None
            (1.0 - fn(x, y).mean()).backward()
        return run
    fns = {"fused": torch_ops.ms_ssim3d, "single_scale": torch_ops.ssim3d, "composite": composite}
    # the fused path and the composite agree before anything is timed
    dv = float((forward_of(fns["fused"])() - forward_of(fns["composite"])()).abs().max())
    step_of(fns["fused"])()
    gf = x.grad.clone()
    step_of(fns["composite"])()
    dg = float((x.grad - gf).abs().max() / gf.abs().max())
    assert dv < 1e-4 and dg < 1e-2, (shape, dv, dg)
    del gf

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n
    cands = []
    for name, fn in fns.items():
        n = reps if name != "composite" else max(1, reps // 2)
        cands += [(name + "_forward", forward_of(fn), n), (name + "_step", step_of(fn), n)]
    for _, fn, _ in cands:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cands}
    for _ in range(3):
        for name, fn, n in cands:
            times[name].append(timed(fn, n))
    row = {name: {"ms": round(min(ts), 3), "spread": spread(ts), "ms_all": [round(t, 3) for t in ts]} for name, ts in times.items()}
    for kind in ("forward", "step"):
        row["composite_over_fused_" + kind] = round(row["composite_" + kind]["ms"] / row["fused_" + kind]["ms"], 2)
        row["fused_over_single_scale_" + kind] = round(row["fused_" + kind]["ms"] / row["single_scale_" + kind]["ms"], 3)
    row["value_differs_by"], row["gradient_differs_by"] = dv, dg
    x.grad = None
    del x, y
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
        raise SystemExit("msssim3f_probe: needs the MI355X (no CPU fallback)")
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
