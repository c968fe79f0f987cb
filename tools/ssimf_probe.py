#!/usr/bin/env python3
"""Speed of SSIM on float32 samples (rmgr_ssim_hip_enqueue_ssimf) next to the 16-bit path on the same shapes, and of the fused
forward + backward (ssim_amd.torch_ops) next to the conv2d composite users build today.

usage (GPU box):  python tools/ssimf_probe.py [--reps N] [--skip-forward] [--skip-training]
    Forward rows.  Device-resident batches: 32 x 4096^2 without a map, 2 x 8192^2 with a map, 128 x 1920x1080 without a map; seeded
    noise, every image in memory of its own; the same pixels as uint16 at depth 16 for rmgr_ssim_hip_enqueue_ssim16.  After a warm-up
    of both, the two are timed alternately in the same process, each over N enqueues between events on the context's stream, best of
    three: ms per batch, Mpix/s, and the float / 16-bit time ratio.
    Training rows.  Forward + backward for x only on (8, 3, 1080, 1920) and (32, 3, 512, 512): loss = SSIMLoss()(x, y); loss.backward().
    The yardstick, in the same process and alternated: five grouped F.conv2d calls with an 11 x 11 window on replicate-padded input
    plus autograd, float32.  Per path: ms per step, ms of the forward alone, the backward / forward ratio and the peak extra memory
    (torch.cuda.max_memory_allocated above what is held before the step; the library's own scratch -- descriptors and cell partials,
    below 1 MB here -- is not torch's and is not in it).
    Prints one JSON line.
torch is imported before the library, so that the process holds one HIP runtime.
"""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORWARD_SHAPES = [(4096, 4096, 32, False), (8192, 8192, 2, True), (1920, 1080, 128, False)]
TRAINING_SHAPES = [(8, 3, 1080, 1920), (32, 3, 512, 512)]


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
    for _ in range(3):                       # alternated, best of three each
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    return ta, tb


def forward_rows(ssim_amd, ctx, reps, result):
    for (w, h, n, with_map) in FORWARD_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(16)
        keep = []
        pf, p16 = (ssim_amd.ParamsF * n)(), (ssim_amd.Params16 * n)()
        for i in range(n):
            a = torch.randint(0, 65536, (h, w), device="cuda", generator=g, dtype=torch.int32)
            b = (a + torch.randint(-1024, 1025, (h, w), device="cuda", generator=g, dtype=torch.int32)).clamp_(0, 65535)
            fa, fb = a.float(), b.float()
            ia, ib = a.to(torch.int16), b.to(torch.int16)        # the same 16 bits
            mf = torch.empty(h, w, device="cuda") if with_map else None
            m16 = torch.empty(h, w, device="cuda") if with_map else None
            pf[i] = ssim_amd.make_params_f(w, h, fa.data_ptr(), 1, w, fb.data_ptr(), 1, w, mf.data_ptr() if with_map else None)
            p16[i] = ssim_amd.make_params16(w, h, ia.data_ptr(), 1, w, ib.data_ptr(), 1, w, m16.data_ptr() if with_map else None)
            keep += [fa, fb, ia, ib, mf, m16]
            del a, b
        sums = torch.empty(2, n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def sf():
            ctx.enqueue_ssimf(pf, n, 65535.0, sums[0].data_ptr())

        def s16():
            ctx.enqueue_ssim16(p16, n, 16, sums[1].data_ptr())
        tf, t16 = alternate(sf, s16, reps)
        torch.cuda.synchronize()
        assert float((sums[0] - sums[1]).abs().max()) / (float(w) * h) < 4e-6          # the two paths measure the same pixels
        mf_, m16_ = min(tf), min(t16)
        px = float(w) * h * n
        result["%dx%dx%d%s" % (n, w, h, "_map" if with_map else "")] = {
            "ssimf_ms": round(mf_, 3), "ssim16_ms": round(m16_, 3), "ratio": round(mf_ / m16_, 3),
            "ssimf_mpix_s": round(px / mf_ / 1e3, 1), "ssim16_mpix_s": round(px / m16_ / 1e3, 1),
            "ssimf_ms_all": [round(t, 3) for t in tf], "ssim16_ms_all": [round(t, 3) for t in t16]}
        del keep, sums
        torch.cuda.empty_cache()


def composite_ssim(x, y, win, c1, c2):
    ch = x.shape[1]

    def G(t):
        return F.conv2d(F.pad(t, (5, 5, 5, 5), mode="replicate"), win, groups=ch)
    mx, my = G(x), G(y)
    sxx, syy, sxy = G(x * x) - mx * mx, G(y * y) - my * my, G(x * y) - mx * my
    smap = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    return smap.mean(dim=(-2, -1))


def training_rows(reps, result):
    from ssim_amd import torch_ops
    k = torch.arange(-5, 6, dtype=torch.float64)
    g1 = torch.exp(-(k * k) / (2 * 1.5 * 1.5))
    g1 = (g1 / g1.sum()).float().cuda()
    for shape in TRAINING_SHAPES:
        torch.manual_seed(5)
        y = torch.rand(shape, device="cuda")
        x = (y + 0.05 * torch.randn(shape, device="cuda")).clamp_(0, 1).requires_grad_(True)
        win = (g1[:, None] * g1[None, :]).expand(shape[1], 1, 11, 11).contiguous()
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        loss_f = torch_ops.SSIMLoss()

        def fused_fwd():
            return loss_f(x, y)

        def comp_fwd():
            return 1.0 - composite_ssim(x, y, win, c1, c2).mean()

        def step(fwd):
            def run():
                x.grad = None
                fwd().backward()
            return run
        # the two paths compute the same loss and the same gradient
        step(fused_fwd)()
        gf, lf = x.grad.clone(), float(fused_fwd().detach())
        step(comp_fwd)()
        gc, lc = x.grad.clone(), float(comp_fwd().detach())
        agree = float((gf - gc).abs().max() / gc.abs().max())
        assert abs(lf - lc) < 1e-5 and agree < 2e-3, (lf, lc, agree)
        del gf, gc
        x.grad = None
        row = {"loss_fused": lf, "loss_composite": lc, "gradient_difference_of_max": agree}
        t_step = alternate(step(fused_fwd), step(comp_fwd), reps)
        t_fwd = alternate(fused_fwd, comp_fwd, reps)
        for name, fwd, ts, tf in (("fused", fused_fwd, t_step[0], t_fwd[0]), ("composite", comp_fwd, t_step[1], t_fwd[1])):
            x.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(fwd)()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            row[name] = {"step_ms": round(min(ts), 3), "forward_ms": round(min(tf), 3),
                         "backward_over_forward": round((min(ts) - min(tf)) / min(tf), 2), "peak_extra_mb": round(peak / 2.0 ** 20, 1),
                         "step_ms_all": [round(t, 3) for t in ts]}
        row["speedup"] = round(row["composite"]["step_ms"] / row["fused"]["step_ms"], 2)
        result["train_" + "x".join(str(s) for s in shape)] = row
        del x, y
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--skip-training", action="store_true")
    args = ap.parse_args()
    import ssim_amd
    if not torch.cuda.is_available() or ssim_amd.device_count() < 1:
        raise SystemExit("ssimf_probe: needs the MI355X (no CPU fallback)")
    torch.cuda.set_stream(torch.cuda.Stream())          # one explicit stream for torch and the library
    stream = torch.cuda.current_stream()
    result = {}
    with ssim_amd.Context(0, ctypes.c_void_p(stream.cuda_stream), mode=ssim_amd.MODE_SEPARABLE) as ctx:
        result["device"] = ctx.describe()
        if not args.skip_forward:
            forward_rows(ssim_amd, ctx, args.reps, result)
    if not args.skip_training:
        training_rows(args.reps, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
