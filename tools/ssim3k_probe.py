#!/usr/bin/env python3
"""Speed of SSIM of float32 volumes under a caller-chosen window (ssim_amd.torch_ops.ssim3d with win_size / win_sigma / window: the
rmgr_ssim_hip_*_ssim3f_win* entries) next to the fixed 11-tap entry on the same tensors and to the float32 composite users build today
with the same window: replicate padding, one 1-D conv3d per axis on each of the five statistics, and autograd.

usage (GPU box):  python tools/ssim3k_probe.py [--reps N] [--out FILE]
    Windows: 3 box, 7 box, 7 Gaussian 1.5, 11 Gaussian 2.  Shapes, device-resident: (1, 1, 512, 512, 512), (4, 1, 128, 128, 128),
    (16, 1, 64, 64, 64).  For each shape and window: the forward alone and a forward + backward step (gradient for x) of the windowed
    entry, of the fixed-window entry and of the composite, in the same process, warmed up, then timed in turn between two events, three
    rounds, ALTERNATED.  Per candidate: ms (best of three, and all three) and the spread (max - min) / min.  Prints one JSON line (and
    writes it to FILE).  No figure is a pass criterion.
torch is imported before the library, so that the process holds one HIP runtime.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 1, 512, 512, 512), (4, 1, 128, 128, 128), (16, 1, 64, 64, 64)]
WINDOWS = [(3, 0.0, "uniform"), (7, 0.0, "uniform"), (7, 1.5, "gaussian"), (11, 2.0, "gaussian")]


def spread(ts):
    return round((max(ts) - min(ts)) / min(ts), 4)


def probe(torch, shape, window, reps):
    import torch.nn.functional as F
    import ssimk_model as K
    from ssim_amd import torch_ops
    size, sigma, kind = window
    kw = dict(win_size=size, win_sigma=sigma if kind == "gaussian" else 1.5, window=kind)
    R = (size - 1) // 2
    torch.manual_seed(5)
    y = torch.rand(shape, device="cuda")
    x = (y + 0.05 * torch.randn(shape, device="cuda")).clamp_(0, 1).requires_grad_(True)
    g1 = torch.tensor(K.full_taps(window), dtype=torch.float32, device="cuda")
    kx, ky, kz = g1.reshape(1, 1, 1, 1, size), g1.reshape(1, 1, 1, size, 1), g1.reshape(1, 1, size, 1, 1)
    c1, c2 = 0.01 ** 2, 0.03 ** 2

    def G(t):
        t = F.conv3d(F.pad(t, (R, R, 0, 0, 0, 0), mode="replicate"), kx)
        t = F.conv3d(F.pad(t, (0, 0, R, R, 0, 0), mode="replicate"), ky)
        return F.conv3d(F.pad(t, (0, 0, 0, 0, R, R), mode="replicate"), kz)

    def composite(a, b):
        ma, mb = G(a), G(b)
        saa, sbb, sab = G(a * a) - ma * ma, G(b * b) - mb * mb, G(a * b) - ma * mb
        m = (2 * ma * mb + c1) * (2 * sab + c2) / ((ma * ma + mb * mb + c1) * (saa + sbb + c2))
        return m.mean(dim=(-3, -2, -1))

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
    fns = {"window": lambda a, b: torch_ops.ssim3d(a, b, **kw), "fixed11": lambda a, b: torch_ops.ssim3d(a, b), "composite": composite}
    # the windowed entry and the composite agree before anything is timed
    dv = float((forward_of(fns["window"])() - forward_of(fns["composite"])()).abs().max())
    step_of(fns["window"])()
    gf = x.grad.clone()
    step_of(fns["composite"])()
    dg = float((x.grad - gf).abs().max() / gf.abs().max())
    assert dv < 1e-4 and dg < 1e-2, (shape, window, dv, dg)
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
    for what in ("forward", "step"):
        row["fixed11_over_window_" + what] = round(row["fixed11_" + what]["ms"] / row["window_" + what]["ms"], 2)
        row["composite_over_window_" + what] = round(row["composite_" + what]["ms"] / row["window_" + what]["ms"], 2)
    # the supposition the numbers are read against: (16 + 2R)^2 staged positions plus 3 (2R + 1) taps per voxel of a 16 x 16 tile
    row["model_cost_relative_to_11_taps"] = round(((16 + 2 * R) ** 2 + 256 * 3 * (2 * R + 1)) / float(26 ** 2 + 256 * 33), 3)
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
    import ssimk_model as K
    if not torch.cuda.is_available() or ssim_amd.device_count() < 1:
        raise SystemExit("ssim3k_probe: needs the MI355X (no CPU fallback)")
    torch.cuda.set_stream(torch.cuda.Stream())          # one explicit stream for torch and the library
    result = {"device": torch.cuda.get_device_name(0)}
    for shape in SHAPES:
        rows = {}
        for window in WINDOWS:
            rows[K.name_of(window)] = probe(torch, shape, window, args.reps)
        result["x".join(str(d) for d in shape)] = rows
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
