#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_msssimf.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/msssimf_torch_checks.py
"""
import json
import os
import sys
import traceback

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ssim_amd                                     # noqa: E402
import msssimf_model as M                           # noqa: E402
from conftest import GOLDEN, image_entries, load_pair   # noqa: E402
from ssim_amd import torch_ops                      # noqa: E402
from msssimf_model import GRAD_TOL, VALUE_TOL       # noqa: E402


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def torch_pair(man):
    """(2, 3, H, W) tensors from six of the einstein pairs."""
    pool = []
    for n in image_entries(man):
        if n.startswith("einstein_") and n != "einstein_einstein":
            a, b = load_pair(man[n])
            pool.append((a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)))
    a = np.stack([np.stack([pool[(3 * i + c) % len(pool)][0] for c in range(3)]) for i in range(2)])
    b = np.stack([np.stack([pool[(3 * i + c) % len(pool)][1] for c in range(3)]) for i in range(2)])
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def abi_of_tensors(ctx, x, y, r, g_out, scales=5, weights=None):
    """The C ABI on the tensors' own memory (contiguous (N, C, H, W)): values, and the gradients of x and of y for dLoss/dMS_i = g_out."""
    torch.cuda.synchronize()
    n, (h, w) = x.shape[0] * x.shape[1], x.shape[-2:]
    ps = (ssim_amd.ParamsF * n)()
    for i in range(n):
        ps[i] = ssim_amd.make_params_f(w, h, x.data_ptr() + 4 * i * h * w, 1, w, y.data_ptr() + 4 * i * h * w, 1, w)
    vals = ctx.msssimf_device(ps, n, r, scales, weights)
    values = torch.empty(n, dtype=torch.float64, device=x.device)
    means = torch.empty((n, scales, 2), dtype=torch.float64, device=x.device)
    go = torch.full((n,), g_out, dtype=torch.float32, device=x.device)
    gx, gy = torch.empty_like(x), torch.empty_like(y)
    ga, gb = (ssim_amd.GradF * n)(), (ssim_amd.GradF * n)()
    for i in range(n):
        ga[i] = ssim_amd.GradF(gx.data_ptr() + 4 * i * h * w, 1, w)
        gb[i] = ssim_amd.GradF(gy.data_ptr() + 4 * i * h * w, 1, w)
    torch.cuda.synchronize()
    ctx.enqueue_msssimf(ps, n, r, values.data_ptr(), means.data_ptr(), scales, weights)
    ctx.enqueue_msssimf_grad(ps, n, r, means.data_ptr(), go.data_ptr(), ga, gb, scales, weights)
    ctx.synchronize()
    assert np.array_equal(bits(values.cpu().numpy().astype(np.float32)), bits(vals))
    return vals, gx, gy


def forward_and_backward_are_the_c_abi_bit_for_bit(man, ctx):
    x, y = torch_pair(man)
    x = x.clone().requires_grad_(True)
    s = torch_ops.ms_ssim(x, y)
    assert s.shape == (2, 3) and s.dtype == torch.float32
    loss = torch_ops.MSSSIMLoss()(x, y)
    loss.backward()
    vals, gx, gy = abi_of_tensors(ctx, x.detach(), y, 1.0, -1.0 / 6.0)
    assert np.array_equal(bits(s.detach().cpu().numpy().reshape(-1)), bits(vals))
    assert abs(float(loss) - (1.0 - float(np.mean(vals.astype(np.float64))))) < 1e-6
    assert torch.equal(x.grad, gx)
    # y alone, and both: only what needs a gradient gets one, with the same bits
    x2, y2 = x.detach().clone().requires_grad_(True), y.clone().requires_grad_(True)
    torch_ops.MSSSIMLoss()(x2, y2).backward()
    assert torch.equal(x2.grad, gx) and torch.equal(y2.grad, gy)
    y3 = y.clone().requires_grad_(True)
    torch_ops.MSSSIMLoss()(x.detach(), y3).backward()
    assert torch.equal(y3.grad, gy)
    none = torch_ops.MSSSIMLoss(reduction="none")(x.detach(), y)
    assert none.shape == (2, 3) and not none.requires_grad
    # other scales and weights, a zero weight among them
    w3 = (0.5, 0.0, 0.5)
    x4 = x.detach().clone().requires_grad_(True)
    s3 = torch_ops.ms_ssim(x4, y, 1.0, 3, w3)
    s3.sum().backward()
    vals3, gx3, _ = abi_of_tensors(ctx, x.detach(), y, 1.0, 1.0, 3, w3)
    assert np.array_equal(bits(s3.detach().cpu().numpy().reshape(-1)), bits(vals3)) and torch.equal(x4.grad, gx3)


def refusals_on_gpu_tensors(man, ctx):
    x, y = torch_pair(man)
    for bad in (lambda: torch_ops.ms_ssim(x, y, data_range=0.0), lambda: torch_ops.ms_ssim(x, y[:, :, :-1]), lambda: torch_ops.ms_ssim(x, y.cpu()),
                lambda: torch_ops.ms_ssim(x, y, scales=0), lambda: torch_ops.ms_ssim(x, y, scales=9, weights=[0.1] * 9),
                lambda: torch_ops.ms_ssim(x, y, scales=4), lambda: torch_ops.ms_ssim(x, y, scales=3, weights=[0.5, 0.5]),
                lambda: torch_ops.ms_ssim(x, y, scales=2, weights=[0.5, -0.5]), lambda: torch_ops.ms_ssim(x, y, scales=2, weights=[0.5, float("nan")])):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("no ValueError")
    try:
        torch_ops.ms_ssim(x.double(), y.double())
    except TypeError:
        return
    raise AssertionError("no TypeError")


def _slices():
    torch.manual_seed(3)
    big_x, big_y = torch.rand(4, 8, 40, 50, device="cuda"), torch.rand(4, 8, 44, 50, device="cuda")
    x, y = big_x[1:3, 2:8:2, 3:35, 5:45:2], big_y[0:2, 1:4, 7:39, 6:26]
    assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape == (2, 3, 32, 20)
    return big_x, big_y, x, y


def non_contiguous_slice_without_a_copy(man, ctx):
    big_x, big_y, x, y = _slices()
    xc, yc = x.contiguous().requires_grad_(True), y.contiguous()
    want = torch_ops.ms_ssim(xc, yc)
    want.sum().backward()
    xs = x.detach().requires_grad_(True)
    assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride()
    before = (big_x.clone(), big_y.clone())
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = torch_ops.ms_ssim(xs, y)
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < x.numel() * 4, peak                   # the values, the means and the result only: no contiguous copy of a plane was made
    got.sum().backward()
    assert torch.equal(got, want) and torch.equal(xs.grad, xc.grad)
    assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])


def non_default_stream(man, ctx):
    _, _, x, y = _slices()
    xc, yc = x.contiguous().requires_grad_(True), y.contiguous()
    want = torch_ops.ms_ssim(xc, yc)                     # on the default stream
    want.sum().backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xq = xc.detach().clone().requires_grad_(True)
        on_side = torch_ops.ms_ssim(xq, yc)
        on_side.sum().backward()
    side.synchronize()
    assert torch.equal(on_side, want) and torch.equal(xq.grad, xc.grad)


def legacy_default_stream(man, ctx):
    """On the legacy default stream the work runs on a side stream ordered against it on the device: results produced by default-stream
    kernels just before, and consumed by default-stream kernels just after, without any host synchronisation in between."""
    assert torch.cuda.current_stream().cuda_stream == 0
    x, y = torch_pair(man)
    want = torch_ops.ms_ssim(x, y)
    torch.cuda.synchronize()
    for _ in range(3):
        xs = (x * 0.5 + x * 0.5).requires_grad_(True)    # produced on the default stream, no synchronise
        got = torch_ops.ms_ssim(xs, y)
        total = (got * 2.0).sum()                        # consumed on the default stream
        total.backward()
        assert torch.equal(got, want) and abs(float(total) - 2.0 * float(want.sum())) < 1e-5
        assert torch.isfinite(xs.grad).all() and float(xs.grad.abs().max()) > 0


def gradient_agrees_with_the_float64_model(man, ctx):
    """A gradcheck-style comparison: torch's backward for a weighted sum of the per-plane values against the float64 model's gradient."""
    x32, y32 = torch_pair(man)
    w = torch.tensor([[1.0, -0.5, 0.25], [2.0, 0.75, -1.5]], device="cuda")
    for scales, wts in ((5, None), (3, (0.2, 0.3, 0.5))):
        xs, ys = x32.clone().requires_grad_(True), y32.clone().requires_grad_(True)
        got = torch_ops.ms_ssim(xs, ys, 1.0, scales, wts)
        (got * w).sum().backward()
        gx, gy, gv = xs.grad.cpu().numpy(), ys.grad.cpu().numpy(), got.detach().cpu().numpy()
        for i in range(2):
            for c in range(3):
                mod = M.Model(x32[i, c].cpu().numpy(), y32[i, c].cpu().numpy(), 1.0)
                dv = abs(float(gv[i, c]) - mod.msssim(scales, wts)[0])
                wa, wb = mod.grad(float(w[i, c]), scales, wts)
                ea = float(np.abs(gx[i, c] - wa).max() / np.abs(wa).max())
                eb = float(np.abs(gy[i, c] - wb).max() / np.abs(wb).max())
                print("model, %d scales, plane %d,%d: value %.3g, gradients %.3g %.3g of max|grad|" % (scales, i, c, dv, ea, eb))
                assert dv <= VALUE_TOL and ea <= GRAD_TOL and eb <= GRAD_TOL, (scales, i, c, dv, ea, eb)


def training_step_memory_is_the_gradients_and_the_means(man, ctx):
    """torch's own count over a training step: beyond the gradient tensor, only small per-plane tensors (values, means, gOut) -- the
    pyramid and the coarse gradients live in the library's scratch, which the library reports itself."""
    torch.manual_seed(5)
    n, c, h, w = 4, 3, 256, 320
    y = torch.rand(n, c, h, w, device="cuda")
    x = (y + 0.05 * torch.randn_like(y)).clamp(0, 1).requires_grad_(True)
    torch_ops.MSSSIMLoss()(x, y).backward()              # warm: contexts, scratch
    x.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    torch_ops.MSSSIMLoss()(x, y).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    grad_bytes, means_bytes = x.numel() * 4, n * c * 5 * 2 * 8
    print("training step: peak extra %d bytes; gradient %d, means %d" % (peak, grad_bytes, means_bytes))
    assert grad_bytes <= peak <= grad_bytes + means_bytes + 64 * 1024, (peak, grad_bytes, means_bytes)      # + a handful of 512-byte blocks


CHECKS = [forward_and_backward_are_the_c_abi_bit_for_bit, refusals_on_gpu_tensors, non_contiguous_slice_without_a_copy, non_default_stream,
          legacy_default_stream, gradient_agrees_with_the_float64_model, training_step_memory_is_the_gradients_and_the_means]


def main():
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    man = manifest()
    result = {}
    with ssim_amd.Context(0) as ctx:
        for check in CHECKS:
            try:
                check(man, ctx)
                result[check.__name__] = "ok"
            except Exception:
                result[check.__name__] = traceback.format_exc()
            torch.cuda.synchronize()
    print("RESULT " + json.dumps(result))


if __name__ == "__main__":
    main()
