#!/usr/bin/env python3
"""Speed of SSIM of float32 samples under the windows of 3, 5, 7, 9 and 11 taps (rmgr_ssim_hip_enqueue_ssimf_win, ssim_amd.torch_ops with
win_size) next to the fixed-window entry rmgr_ssim_hip_enqueue_ssimf on the same device-resident batch in the same process, and of a
forward + backward step next to the float32 conv2d composite with the same window.

usage (GPU box):  python tools/ssimk_probe.py [--reps N] [--composite-reps N] [--skip-torch]
    Forward, through the C ABI on one context: 32 x 4096^2, 128 x 1080p (1920 x 1080), 2 x 8192^2 with a map.  For each batch the plain
    entry and the _win entry of every size (Gaussian of sigma 1.5; 3 and 7 also as a box; 11 also at sigma 2.0) are warmed up, then
    timed in turn over N enqueues between two host clock reads around a synchronize, three rounds, ALTERNATED (every candidate once
    per round).  Per candidate: ms (best of three, and all three), the spread (max - min) / min, and its time over the plain entry's.
    The one figure worth a sentence if it fails: no smaller window may be slower than ssimf on the same batch ("slower_than_ssimf").
    Step, through torch: (8, 3, 1080, 1920), gradient for x: SSIMLoss(win_size=...) forward + backward against the composite of five
    grouped conv2d of replicate-padded planes with the same taps, alternated, three rounds.
    Prints one JSON line.
torch is imported before the library, so that the process holds one HIP runtime.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCHES = [("32x4096x4096", 32, 4096, 4096, False), ("128x1920x1080", 128, 1920, 1080, False), ("2x8192x8192+map", 2, 8192, 8192, True)]
WINDOWS = [(3, 0.0, "uniform"), (3, 1.5, "gaussian"), (5, 1.5, "gaussian"), (7, 0.0, "uniform"), (7, 1.5, "gaussian"), (9, 1.5, "gaussian"),
           (11, 2.0, "gaussian")]


def name_of(window):
    return "%d box" % window[0] if window[2] == "uniform" else "%d gaussian %g" % (window[0], window[1])


def spread(ts):
    return round((max(ts) - min(ts)) / min(ts), 4)


def forward_probe(torch, ssim_amd, reps):
    out = {}
    with ssim_amd.Context(0) as ctx:
        for label, n, w, h, with_map in BATCHES:
            # one pair of planes stands for the batch: every pair reads the same 2 x W x H floats (the kernels do not know), so that
            # 128 x 1080p and 32 x 4096^2 fit next to a map; a map, where asked for, is one per pair
            torch.manual_seed(1)
            a = torch.rand(h, w, device="cuda")
            b = (a + 0.05 * torch.randn(h, w, device="cuda")).clamp_(0, 1)
            maps = torch.empty(n, h, w, device="cuda") if with_map else None
            sums = torch.empty(n, dtype=torch.float64, device="cuda")
            ps = (ssim_amd.ParamsF * n)()
            for i in range(n):
                ps[i] = ssim_amd.make_params_f(w, h, a.data_ptr(), 1, w, b.data_ptr(), 1, w, maps[i].data_ptr() if with_map else None, 1, w)
            torch.cuda.synchronize()
            cands = [("ssimf", None)] + [(name_of(wd), ssim_amd.make_window(wd[0], wd[1] if wd[2] == "gaussian" else 1.5, wd[2])) for wd in WINDOWS]

            def run(win):
                t0 = time.perf_counter()
                for _ in range(reps):
                    ctx.enqueue_ssimf(ps, n, 1.0, sums.data_ptr(), window=win)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e3 / reps
            for _, win in cands:
                run(win)
            times = {name: [] for name, _ in cands}
            for _ in range(3):
                for name, win in cands:
                    times[name].append(run(win))
            base = min(times["ssimf"])
            row = {name: {"ms": round(min(ts), 3), "spread": spread(ts), "ms_all": [round(t, 3) for t in ts], "over_ssimf": round(min(ts) / base, 3)}
                   for name, ts in times.items()}
            row["slower_than_ssimf"] = [name for name, _ in cands[1:] if not name.startswith("11") and min(times[name]) > base]
            out[label] = row
            del a, b, maps, sums
            torch.cuda.empty_cache()
    return out


def step_probe(torch, reps, composite_reps):
    import torch.nn.functional as F
    import ssimk_model as K
    from ssim_amd import torch_ops
    shape = (8, 3, 1080, 1920)
    torch.manual_seed(5)
    y = torch.rand(shape, device="cuda")
    x = (y + 0.05 * torch.randn(shape, device="cuda")).clamp_(0, 1).requires_grad_(True)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    out = {}
    for window in [(11, 1.5, "gaussian")] + WINDOWS:
        size, sigma, kind = window
        R = (size - 1) // 2
        g1 = torch.tensor(K.full_taps(window), dtype=torch.float32, device="cuda")
        win = (g1[:, None] * g1[None, :]).expand(shape[1], 1, size, size).contiguous()
        loss_f = torch_ops.SSIMLoss(win_size=size, win_sigma=sigma if kind == "gaussian" else 1.5, window=kind)

        def G(t):
            return F.conv2d(F.pad(t, (R, R, R, R), mode="replicate"), win, groups=t.shape[1])

        def step_fused():
            x.grad = None
            loss_f(x, y).backward()

        def step_composite():
            x.grad = None
            mx, my = G(x), G(y)
            sxx, syy, sxy = G(x * x) - mx * mx, G(y * y) - my * my, G(x * y) - mx * my
            m = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
            (1.0 - m.mean()).backward()
        step_fused()
        gf = x.grad.clone()
        step_composite()
        e = float((x.grad - gf).abs().max() / gf.abs().max())
        assert e < 1e-2, (window, e)

        def timed(fn, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / n
        step_fused()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(3):
            tf.append(timed(step_fused, reps))
            tc.append(timed(step_composite, composite_reps))
        out[name_of(window)] = {"fused_step_ms": round(min(tf), 3), "fused_spread": spread(tf), "composite_step_ms": round(min(tc), 3),
                                "composite_spread": spread(tc), "composite_over_fused": round(min(tc) / min(tf), 1),
                                "composite_gradient_differs_by": e}
        del win, gf
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composite-reps", type=int, default=2)
    ap.add_argument("--skip-torch", action="store_true", help="the forward probe only")
    args = ap.parse_args()
    import torch
    import ssim_amd
    if not torch.cuda.is_available() or ssim_amd.device_count() < 1:
        raise SystemExit("ssimk_probe: needs the MI355X (no CPU fallback)")
    torch.cuda.set_stream(torch.cuda.Stream())          # one explicit stream for torch and the library
    result = {"device": torch.cuda.get_device_name(0), "forward": forward_probe(torch, ssim_amd, args.reps)}
    if not args.skip_torch:
        result["step_8x3x1080x1920"] = step_probe(torch, args.reps, args.composite_reps)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
