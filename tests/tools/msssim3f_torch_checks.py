#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_msssim3f.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/msssim3f_torch_checks.py
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
import msssim3f_model as M                          # noqa: E402
from ssim_amd import torch_ops                      # noqa: E402

VALUE_TOL, MEAN_TOL, GRAD_TOL, IDENT_TOL = M.tolerances()


def volumes(shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def c_abi(ctx, x, y, g, scales, weights, want_x, want_y):
    """The C ABI on the contiguous volumes of x and y: (float32 values, dA or None, dB or None) as tensors."""
    d, h, w = x.shape[-3:]
    n = x.numel() // (d * h * w)
    xc, yc = x.contiguous(), y.contiguous()
    ps = (ssim_amd.Params3F * n)()
    for i in range(n):
        ps[i] = ssim_amd.make_params3f(w, h, d, xc.data_ptr() + 4 * i * d * h * w, (1, w, w * h), yc.data_ptr() + 4 * i * d * h * w, (1, w, w * h))
    values = torch.empty(n, dtype=torch.float64, device="cuda")
    means = torch.empty((n, scales, 2), dtype=torch.float64, device="cuda")
    gc = g.to(torch.float32).reshape(-1).contiguous()
    ga, gb = (torch.empty_like(xc) if want_x else None), (torch.empty_like(yc) if want_y else None)
    torch.cuda.synchronize()
    ctx.enqueue_msssim3f(ps, n, 1.0, values.data_ptr(), means.data_ptr(), scales, weights)

    def grads(t):
        arr = (ssim_amd.Grad3F * n)()
        for i in range(n):
            arr[i] = ssim_amd.Grad3F(t.data_ptr() + 4 * i * d * h * w, 1, w, w * h)
        return arr
    ctx.enqueue_msssim3f_grad(ps, n, 1.0, means.data_ptr(), gc.data_ptr(), grads(ga) if want_x else None, grads(gb) if want_y else None, scales, weights)
    ctx.synchronize()
    return values.to(torch.float32).reshape(x.shape[:-3]), ga, gb


def value_and_gradients_against_the_c_abi(ctx):
    x, y = volumes((2, 2, 9, 20, 33), 1)
    w = torch.tensor([[1.0, -0.5], [0.25, 2.0]], device="cuda")
    for scales, weights in ((5, None), (3, (0.5, 0.0, 0.5))):
        for want_x, want_y in ((True, False), (False, True), (True, True)):
            xs, ys = x.clone().requires_grad_(want_x), y.clone().requires_grad_(want_y)
            s = torch_ops.ms_ssim3d(xs, ys, 1.0, scales, weights)
            assert s.shape == (2, 2) and s.dtype == torch.float32
            (s * w).sum().backward()
            assert (xs.grad is not None) == want_x and (ys.grad is not None) == want_y
            v, ga, gb = c_abi(ctx, x, y, w, scales, weights, want_x, want_y)
            assert torch.equal(s.detach(), v)
            assert (not want_x or torch.equal(xs.grad, ga)) and (not want_y or torch.equal(ys.grad, gb))
    # and against the float64 model
    xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    s = torch_ops.ms_ssim3d(xs, ys)
    (s * w).sum().backward()
    for i in range(2):
        for c in range(2):
            mod = M.Model(x[i, c].cpu().numpy(), y[i, c].cpu().numpy(), 1.0)
            assert abs(float(s[i, c]) - mod.msssim()[0]) <= VALUE_TOL + 1e-7
            for t, g in zip((xs.grad, ys.grad), mod.grad(float(w[i, c]))):
                e = float(np.abs(t[i, c].cpu().numpy() - g).max() / np.abs(g).max())
                print("model: volume %d,%d gradient %.3g of max|grad|" % (i, c, e))
                assert e <= GRAD_TOL, (i, c, e)


def loss_forms_and_errors(ctx):
    x, y = volumes((3, 1, 7, 12, 12), 2)
    xs = x.clone().requires_grad_(True)
    s = torch_ops.ms_ssim3d(xs, y, 1.0)
    loss = torch_ops.MSSSIM3DLoss()(xs, y)
    assert loss.shape == () and abs(float(loss) - (1.0 - float(s.double().mean()))) < 1e-6
    loss.backward()
    g = M.grad(x[1, 0].cpu().numpy(), y[1, 0].cpu().numpy(), 1.0, -1.0 / 3.0)[0]
    assert float(np.abs(xs.grad[1, 0].cpu().numpy() - g).max() / np.abs(g).max()) <= GRAD_TOL
    none = torch_ops.MSSSIM3DLoss(reduction="none", scales=2, weights=(0.5, 0.5))(x, y)
    assert none.shape == (3, 1) and not none.requires_grad
    assert torch.equal(none, 1.0 - torch_ops.ms_ssim3d(x, y, 1.0, 2, (0.5, 0.5)))
    for bad in (lambda: torch_ops.ms_ssim3d(x, y, data_range=0.0), lambda: torch_ops.ms_ssim3d(x, y[..., :-1]), lambda: torch_ops.ms_ssim3d(x, y.cpu()),
                lambda: torch_ops.ms_ssim3d(x[0, 0, 0], y[0, 0, 0]), lambda: torch_ops.ms_ssim3d(x, y, scales=9), lambda: torch_ops.ms_ssim3d(x, y, scales=3),
                lambda: torch_ops.ms_ssim3d(x, y, scales=2, weights=(1.0, -1.0)), lambda: torch_ops.MSSSIM3DLoss(reduction="sum")):
        try:
            bad()
        except ValueError as e:
            assert "ms_ssim3d" in str(e) or "MSSSIM3DLoss" in str(e), str(e)
            continue
        raise AssertionError("no ValueError")
    for bad in (lambda: torch_ops.ms_ssim3d(x.half(), y.half()), lambda: torch_ops.ms_ssim3d(x.bfloat16(), y.bfloat16())):
        try:
            bad()
        except TypeError as e:
            assert "3-D multi-scale path is float32 for now" in str(e)
        else:
            raise AssertionError("no TypeError")


def non_contiguous_and_expanded_inputs(ctx):
    torch.manual_seed(3)
    big_x, big_y = torch.rand(3, 4, 14, 30, 40, device="cuda"), torch.rand(40, 3, 12, 26, device="cuda")
    x = big_x[0:2, 1:4:2, 2:12, 3:27, 5:39:2]                      # (2, 2, 10, 24, 17): offsets, step 2
    y = big_y[3:37:2, 0:2, 1:11, 2:26].permute(1, 2, 3, 0)[:, None].expand(2, 2, 10, 24, 17)      # W stored outermost; the second dimension expanded
    assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape and y.stride(1) == 0
    xc, yc = x.contiguous().requires_grad_(True), y.contiguous().requires_grad_(True)
    want = torch_ops.ms_ssim3d(xc, yc, 1.0, 3, (0.2, 0.3, 0.5))
    want.sum().backward()
    xs, ys = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
    before = (big_x.clone(), big_y.clone())
    got = torch_ops.ms_ssim3d(xs, ys, 1.0, 3, (0.2, 0.3, 0.5))
    got.sum().backward()
    assert torch.equal(got, want) and torch.equal(xs.grad, xc.grad) and torch.equal(ys.grad, yc.grad)
    assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])


def side_stream(ctx):
    x, y = volumes((2, 1, 12, 18, 21), 4)
    xc = x.clone().requires_grad_(True)
    want = torch_ops.ms_ssim3d(xc, y)                               # on the default stream
    want.sum().backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xq = x.clone().requires_grad_(True)
        on_side = torch_ops.ms_ssim3d(xq, y)
        on_side.sum().backward()
    side.synchronize()
    assert torch.equal(on_side, want) and torch.equal(xq.grad, xc.grad)


def empty_batch(ctx):
    x = torch.zeros(0, 2, 4, 5, 6, device="cuda", requires_grad=True)
    s = torch_ops.ms_ssim3d(x, torch.zeros(0, 2, 4, 5, 6, device="cuda"))
    assert s.shape == (0, 2) and s.dtype == torch.float32
    s.sum().backward()
    assert x.grad.shape == x.shape
    v, w = volumes((4, 5, 6), 5)                                     # no leading dimension at all: a scalar
    assert torch_ops.ms_ssim3d(v, w).shape == ()


CHECKS = [value_and_gradients_against_the_c_abi, loss_forms_and_errors, non_contiguous_and_expanded_inputs, side_stream, empty_batch]


def main():
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    result = {}
    with ssim_amd.Context(0) as ctx:
        for check in CHECKS:
            try:
                check(ctx)
                result[check.__name__] = "ok"
            except Exception:
                result[check.__name__] = traceback.format_exc()
            torch.cuda.synchronize()
    print("RESULT " + json.dumps(result))


if __name__ == "__main__":
    main()
