#!/usr/bin/env python3
"""Speed of multi-scale SSIM on float32 samples (rmgr_ssim_hip_enqueue_msssimf) next to single-scale float32 SSIM and to the uint8
multi-scale path on the same shapes, and of the fused forward + backward (ssim_amd.torch_ops.MSSSIMLoss) next to the avg_pool2d +
conv2d composite users build today.

usage (GPU box):  python tools/msssimf_probe.py [--reps N] [--skip-forward] [--skip-training]
    Forward rows.  Device-resident batches, Wang's 5 scales: 32 x 4096^2, 128 x 1920x1080, 2 x 8192^2; seeded 8-bit noise pairs as
    float32 at range 255, every image in memory of its own; the same pixels as uint8 for rmgr_ssim_hip_compute_msssim_device.  After a
    warm-up of all three, msssimf is timed alternately with (i) rmgr_ssim_hip_enqueue_ssimf on the same batch and, in a second round,
    (ii) the uint8 multi-scale call, each over N calls between events on the context's stream, best of three: ms per batch, Mpix/s of
    scale-0 pixels, and the time ratios.  (ii) blocks in every call; the other two are enqueues that end in one synchronise.
    Training rows.  Forward + backward for x only on (8, 3, 1080, 1920) and (32, 3, 512, 512): loss = MSSSIMLoss()(x, y);
    loss.backward().  The yardstick, in the same process and alternated, float32: per scale five grouped F.conv2d calls with an
    11 x 11 window on replicate-padded input, F.avg_pool2d on planes replicate-padded to even sizes between scales, the ReLU'd
    weighted product, autograd.  The two must first agree on the loss (2.5e-6) and on the gradient (5.5e-4 of its maximum), the
    bounds of tests/test_gpu_msssimf.py.  Per path: ms per step, ms of the forward alone, the backward / forward ratio and the peak
    extra memory (torch.cuda.max_memory_allocated above what is held before the step); the library's own scratch -- pyramid, coarse
    gradient planes, cell partials -- is not torch's: it is reported separately, as the drop of the device's free memory
    (rmgr_ssim_hip_get_memory_info) over the fused path's first step beyond what torch reserved in it.
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

FORWARD_SHAPES = [(4096, 4096, 32), (1920, 1080, 128), (8192, 8192, 2)]
TRAINING_SHAPES = [(8, 3, 1080, 1920), (32, 3, 512, 512)]
WANG = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
VALUE_TOL, GRAD_TOL = 2.5e-6, 5.5e-4          # tests/msssimf_model.py


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
    for (w, h, n) in FORWARD_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(16)
        keep = []
        pf, p8 = (ssim_amd.ParamsF * n)(), (ssim_amd.Params * n)()
        for i in range(n):
            a = torch.randint(0, 256, (h, w), device="cuda", generator=g, dtype=torch.int32)
            b = (a + torch.randint(-8, 9, (h, w), device="cuda", generator=g, dtype=torch.int32)).clamp_(0, 255)
            fa, fb = a.float(), b.float()
            ia, ib = a.to(torch.uint8), b.to(torch.uint8)        # the same pixels
            pf[i] = ssim_amd.make_params_f(w, h, fa.data_ptr(), 1, w, fb.data_ptr(), 1, w)
            p8[i] = ssim_amd.make_params(w, h, ia.data_ptr(), 1, w, ib.data_ptr(), 1, w)
            keep += [fa, fb, ia, ib]
            del a, b
        sums = torch.empty(n, dtype=torch.float64, device="cuda")
        values = torch.empty(n, dtype=torch.float64, device="cuda")
        means = torch.empty((n, 5, 2), dtype=torch.float64, device="cuda")
        out8 = [None]
        torch.cuda.synchronize()

        def msf():
            ctx.enqueue_msssimf(pf, n, 255.0, values.data_ptr(), means.data_ptr())

        def sf():
            ctx.enqueue_ssimf(pf, n, 255.0, sums.data_ptr())

        def ms8():
            out8[0] = ctx.msssim_device(p8, n)
        t_ms, t_sf = alternate(msf, sf, reps)
        t_ms2, t_8 = alternate(msf, ms8, reps)
        torch.cuda.synchronize()
        assert float((values.cpu() - torch.from_numpy(out8[0]).double()).abs().max()) < 6e-6      # the two paths measure the same pixels
        m_ms, m_sf, m_8 = min(t_ms + t_ms2), min(t_sf), min(t_8)
        px = float(w) * h * n
        result["%dx%dx%d" % (n, w, h)] = {
            "msssimf_ms": round(m_ms, 3), "ssimf_ms": round(m_sf, 3), "msssim_u8_ms": round(m_8, 3),
            "ratio_to_ssimf": round(m_ms / m_sf, 3), "ratio_to_msssim_u8": round(m_ms / m_8, 3),
            "msssimf_mpix_s": round(px / m_ms / 1e3, 1), "ssimf_mpix_s": round(px / m_sf / 1e3, 1), "msssim_u8_mpix_s": round(px / m_8 / 1e3, 1),
            "msssimf_ms_all": [round(t, 3) for t in t_ms + t_ms2], "ssimf_ms_all": [round(t, 3) for t in t_sf], "msssim_u8_ms_all": [round(t, 3) for t in t_8]}
        del keep, sums, values, means
        torch.cuda.empty_cache()


def composite_msssim(x, y, win, c1, c2, weights):
    """The composite users run today, per plane: (N, C)."""
    ch = x.shape[1]

    def G(t):
        return F.conv2d(F.pad(t, (5, 5, 5, 5), mode="replicate"), win, groups=ch)

    def down(t):
        return F.avg_pool2d(F.pad(t, (0, t.shape[-1] % 2, 0, t.shape[-2] % 2), mode="replicate"), 2)
    out = None
    for s, wgt in enumerate(weights):
        mx, my = G(x), G(y)
        sxx, syy, sxy = G(x * x) - mx * mx, G(y * y) - my * my, G(x * y) - mx * my
        cs = (2 * sxy + c2) / (sxx + syy + c2)
        if s == len(weights) - 1:
            m = ((2 * mx * my + c1) / (mx * mx + my * my + c1) * cs).mean(dim=(-2, -1))
        else:
            m = cs.mean(dim=(-2, -1))
            x, y = down(x), down(y)
        term = m.clamp(min=0) ** wgt
        out = term if out is None else out * term
    return out


def training_rows(ssim_amd, reps, result):
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
        loss_f = torch_ops.MSSSIMLoss()

        def fused_fwd():
            return loss_f(x, y)

        def comp_fwd():
            return 1.0 - composite_msssim(x, y, win, c1, c2, WANG).mean()

        def step(fwd):
            def run():
                x.grad = None
                fwd().backward()
            return run
        # the two paths compute the same loss and the same gradient
        torch.cuda.synchronize()
        free0, reserved0 = ssim_amd.memory_info()[0], torch.cuda.memory_reserved()
        step(fused_fwd)()
        torch.cuda.synchronize()
        # what left the device's free memory over the first fused step and is not torch's: the library's scratch (and its contexts)
        scratch = (free0 - ssim_amd.memory_info()[0]) - (torch.cuda.memory_reserved() - reserved0)
        gf, lf = x.grad.clone(), float(fused_fwd().detach())
        x.grad = None
        step(comp_fwd)()
        gc, lc = x.grad.clone(), float(comp_fwd().detach())
        agree = float((gf - gc).abs().max() / gc.abs().max())
        assert abs(lf - lc) <= VALUE_TOL and agree <= GRAD_TOL, (lf, lc, agree)
        del gf, gc
        x.grad = None
        row = {"loss_fused": lf, "loss_composite": lc, "gradient_difference_of_max": agree,
               "library_scratch_mb": round(scratch / 2.0 ** 20, 1)}
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
        row["memory_ratio"] = round(row["composite"]["peak_extra_mb"] / max(row["fused"]["peak_extra_mb"], 0.1), 1)
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
        raise SystemExit("msssimf_probe: needs the MI355X (no CPU fallback)")
    torch.cuda.set_stream(torch.cuda.Stream())          # one explicit stream for torch and the library
    stream = torch.cuda.current_stream()
    result = {}
    with ssim_amd.Context(0, ctypes.c_void_p(stream.cuda_stream), mode=ssim_amd.MODE_SEPARABLE) as ctx:
        result["device"] = ctx.describe()
        if not args.skip_forward:
            forward_rows(ssim_amd, ctx, args.reps, result)
    if not args.skip_training:
        training_rows(ssim_amd, args.reps, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
