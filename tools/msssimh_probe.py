#!/usr/bin/env python3
"""Speed of multi-scale SSIM on float16 / bfloat16 samples (rmgr_ssim_hip_enqueue_msssimh) next to the float32 path on the widened planes,
and of a bfloat16 training step (ssim_amd.torch_ops.MSSSIMLoss) next to the route through float32 copies, the only one there was before.

usage (GPU box):  python tools/msssimh_probe.py [--reps N] [--skip-forward] [--skip-training]
    Both parts run on 128 x 1920x1080 and 32 x 4096^2 with Wang's five scales.
    Forward rows.  Device-resident batches of seeded integer-valued noise in 0..255 (exact in float16, bfloat16 and float32, so the three
    paths see the same pixels), every image in memory of its own, data range 255.  After a warm-up msssimf on the widened planes, msssimh
    float16 and msssimh bfloat16 are timed in turn in the same process, each over N enqueues between events on the context's stream,
    three rounds: best ms per batch, Mpix/s, the ratio to msssimf and each path's own run-to-run spread ((max - min) / min over the
    three rounds).  The msssimh values and means are checked to have msssimf's bits.
    Training rows.  Forward + backward for x only on (32, 4, 1080, 1920) and (8, 4, 4096, 4096) bfloat16 tensors:
    loss = MSSSIMLoss()(x, y); loss.backward().  The yardstick, in the same process and alternated, is
    MSSSIMLoss()(x.float(), y.float()) with its casts inside the timed region.  Per path: ms per step (best of three, and all three) and
    the peak extra memory (torch.cuda.max_memory_allocated above what is held before the step; the library's own scratch -- the
    float32 pyramids and coarse gradient planes, the same for both routes -- is not torch's and is not in it).
    Prints one JSON line.
torch is imported before the library, so that the process holds one HIP runtime.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORWARD_SHAPES = [(1920, 1080, 128), (4096, 4096, 32)]
TRAINING_SHAPES = [(32, 4, 1080, 1920), (8, 4, 4096, 4096)]
SCALES = 5


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, reps):
    """Every function warmed up, then timed in turn, three rounds: a list of three times per function."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(3):
        for t, fn in zip(times, fns):
            t.append(timed(fn, reps))
    return times


def spread(ts):
    return round((max(ts) - min(ts)) / min(ts), 4)


def forward_rows(ssim_amd, ctx, reps, result):
    for (w, h, n) in FORWARD_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(16)
        keep = []
        pf, ph, pb = (ssim_amd.ParamsF * n)(), (ssim_amd.Params16 * n)(), (ssim_amd.Params16 * n)()
        for i in range(n):
            a = torch.randint(0, 256, (h, w), device="cuda", generator=g, dtype=torch.int32)
            b = (a + torch.randint(-16, 17, (h, w), device="cuda", generator=g, dtype=torch.int32)).clamp_(0, 255)
            planes = [(a.float(), b.float()), (a.half(), b.half()), (a.bfloat16(), b.bfloat16())]
            for ps, make, (pa, pb_) in zip((pf, ph, pb), (ssim_amd.make_params_f, ssim_amd.make_params16, ssim_amd.make_params16), planes):
                ps[i] = make(w, h, pa.data_ptr(), 1, w, pb_.data_ptr(), 1, w)
            keep.append(planes)
            del a, b
        vals = torch.empty(3, n, dtype=torch.float64, device="cuda")
        means = torch.empty(3, n, SCALES, 2, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        fns = [lambda: ctx.enqueue_msssimf(pf, n, 255.0, vals[0].data_ptr(), means[0].data_ptr()),
               lambda: ctx.enqueue_msssimh(ph, n, 255.0, "float16", vals[1].data_ptr(), means[1].data_ptr()),
               lambda: ctx.enqueue_msssimh(pb, n, 255.0, "bfloat16", vals[2].data_ptr(), means[2].data_ptr())]
        times = alternate(fns, reps)
        torch.cuda.synchronize()
        for k in (1, 2):                                                                   # the bits of msssimf on the widened planes
            assert torch.equal(vals[k], vals[0]) and torch.equal(means[k], means[0])
        px = float(w) * h * n
        row = {"value_0": float(vals[0, 0])}
        for name, ts in zip(("msssimf", "msssimh_float16", "msssimh_bfloat16"), times):
            row[name] = {"ms": round(min(ts), 3), "mpix_s": round(px / min(ts) / 1e3, 1), "over_msssimf": round(min(ts) / min(times[0]), 3),
                         "spread": spread(ts), "ms_all": [round(t, 3) for t in ts]}
        result["%dx%dx%d" % (n, w, h)] = row
        del keep, vals, means
        torch.cuda.empty_cache()


def training_rows(reps, result):
    from ssim_amd import torch_ops
    for shape in TRAINING_SHAPES:
        torch.manual_seed(5)
        y32 = torch.rand(shape, device="cuda")
        x = (y32 + 0.05 * torch.randn(shape, device="cuda")).clamp_(0, 1).to(torch.bfloat16).requires_grad_(True)
        y = y32.to(torch.bfloat16)
        del y32
        loss_f = torch_ops.MSSSIMLoss()

        def native():
            x.grad = None
            loss_f(x, y).backward()

        def widened():
            x.grad = None
            loss_f(x.float(), y.float()).backward()
        # the two routes compute the same loss; the native gradient is the float32 one rounded once, which is what autograd's cast of
        # the float32 gradient back to bfloat16 gives as well
        native()
        gn, ln = x.grad.clone(), float(loss_f(x, y).detach())
        widened()
        gw, lw = x.grad.clone(), float(loss_f(x.float(), y.float()).detach())
        assert ln == lw and torch.equal(gn, gw), (ln, lw)
        del gn, gw
        row = {"loss": ln}
        times = alternate([native, widened], reps)
        for name, fn, ts in (("native", native, times[0]), ("through_float32", widened, times[1])):
            x.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            row[name] = {"step_ms": round(min(ts), 3), "peak_extra_mb": round(peak / 2.0 ** 20, 1), "spread": spread(ts),
                         "step_ms_all": [round(t, 3) for t in ts]}
        row["speedup"] = round(row["through_float32"]["step_ms"] / row["native"]["step_ms"], 2)
        row["memory_ratio"] = round(row["through_float32"]["peak_extra_mb"] / row["native"]["peak_extra_mb"], 2)
        result["train_bfloat16_" + "x".join(str(s) for s in shape)] = row
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
        raise SystemExit("msssimh_probe: needs the MI355X (no CPU fallback)")
    torch.cuda.set_stream(torch.cuda.Stream())          # one explicit stream for torch and the library
    stream = torch.cuda.current_stream()
    result = {}
    with ssim_amd.Context(0, ctypes.c_void_p(stream.cuda_stream)) as ctx:
        result["device"] = ctx.describe()
        if not args.skip_forward:
            forward_rows(ssim_amd, ctx, args.reps, result)
    if not args.skip_training:
        training_rows(args.reps, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
