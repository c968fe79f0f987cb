#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_ssim3f.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/ssim3f_torch_checks.py
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
import ssim3f_model as S                            # noqa: E402
from ssim_amd import torch_ops                      # noqa: E402

PX_TOL, G_TOL, GRAD_TOL, IDENT_TOL = S.tolerances()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def volumes(shape, seed):
    """x, y of `shape` (..., D, H, W): smooth-ish random volumes in [0, 1] and a noisy copy."""
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def value_and_gradients_against_the_model(ctx):
    x, y = volumes((2, 2, 9, 20, 33), 1)
    w = torch.tensor([[1.0, -0.5], [0.25, 2.0]], device="cuda")
    for want_x, want_y in ((True, False), (False, True), (True, True)):
        xs, ys = x.clone().requires_grad_(want_x), y.clone().requires_grad_(want_y)
        s = torch_ops.ssim3d(xs, ys)
        assert s.shape == (2, 2) and s.dtype == torch.float32
        (s * w).sum().backward()
        assert (xs.grad is not None) == want_x and (ys.grad is not None) == want_y
        for i in range(2):
            for c in range(2):
                a, b = x[i, c].cpu().numpy(), y[i, c].cpu().numpy()
                gv, _ = S.ssim(a, b, 1.0)
                ga, gb = S.grad(a, b, 1.0, float(w[i, c]))
                assert abs(float(s[i, c]) - gv) <= G_TOL, (i, c, float(s[i, c]), gv)
                for t, g in ((xs.grad, ga), (ys.grad, gb)):
                    if t is not None:
                        e = float(np.abs(t[i, c].cpu().numpy() - g).max() / np.abs(g).max())
                        print("model: volume %d,%d gradient %.3g of max|grad|" % (i, c, e))
                        assert e <= GRAD_TOL, (i, c, e)
    # one gradient or both: the same bits
    x1, y1 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    torch_ops.ssim3d(x1, y1).sum().backward()
    x2 = x.clone().requires_grad_(True)
    torch_ops.ssim3d(x2, y).sum().backward()
    y2 = y.clone().requires_grad_(True)
    torch_ops.ssim3d(x, y2).sum().backward()
    assert torch.equal(x1.grad, x2.grad) and torch.equal(y1.grad, y2.grad)


def loss_forms(ctx):
    x, y = volumes((3, 1, 7, 12, 12), 2)
    xs = x.clone().requires_grad_(True)
    s = torch_ops.ssim3d(xs, y, 1.0)
    loss = torch_ops.SSIM3DLoss()(xs, y)
    assert loss.shape == () and abs(float(loss) - (1.0 - float(s.double().mean()))) < 1e-6
    loss.backward()
    none = torch_ops.SSIM3DLoss(reduction="none")(x, y)
    assert none.shape == (3, 1) and not none.requires_grad
    assert torch.equal(none, 1.0 - s.detach())
    g = S.grad(x[1, 0].cpu().numpy(), y[1, 0].cpu().numpy(), 1.0, -1.0 / 3.0)[0]
    assert float(np.abs(xs.grad[1, 0].cpu().numpy() - g).max() / np.abs(g).max()) <= GRAD_TOL
    # at range 255 the loss of the scaled volumes is the same to the model's tolerance
    s255 = torch_ops.SSIM3DLoss(data_range=255.0, reduction="none")(x * 255, y * 255)
    assert float((s255 - none).abs().max()) <= 2 * G_TOL
    for bad in (lambda: torch_ops.ssim3d(x, y, data_range=0.0), lambda: torch_ops.ssim3d(x, y[..., :-1]), lambda: torch_ops.ssim3d(x, y.cpu()),
                lambda: torch_ops.ssim3d(x[0, 0, 0], y[0, 0, 0])):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("no ValueError")
    try:
        torch_ops.ssim3d(x.half(), y.half())
    except TypeError as e:
        assert "float32 for now" in str(e)
    else:
        raise AssertionError("no TypeError")


def non_contiguous_and_expanded_inputs(ctx):
    torch.manual_seed(3)
    big_x, big_y = torch.rand(3, 4, 14, 30, 40, device="cuda"), torch.rand(40, 3, 12, 26, device="cuda")
    x = big_x[0:2, 1:4:2, 2:12, 3:27, 5:39:2]                      # (2, 2, 10, 24, 17): offsets, step 2
    y = big_y[3:37:2, 0:2, 1:11, 2:26].permute(1, 2, 3, 0)[:, None].expand(2, 2, 10, 24, 17)      # W stored outermost; the second dimension expanded
    assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape and y.stride(1) == 0
    xc, yc = x.contiguous().requires_grad_(True), y.contiguous().requires_grad_(True)
    want = torch_ops.ssim3d(xc, yc)
    want.sum().backward()
    xs, ys = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
    assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride() and ys.stride() == y.stride()
    before = (big_x.clone(), big_y.clone())
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = torch_ops.ssim3d(xs, ys)
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < x[0, 0].numel() * 4, peak                       # the sums and the result only: no contiguous copy of a volume was made
    got.sum().backward()
    assert torch.equal(got, want) and torch.equal(xs.grad, xc.grad) and torch.equal(ys.grad, yc.grad)
    assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])


def side_stream(ctx):
    x, y = volumes((2, 1, 12, 18, 21), 4)
    xc = x.clone().requires_grad_(True)
    want = torch_ops.ssim3d(xc, y)                                   # on the default stream
    want.sum().backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xq = x.clone().requires_grad_(True)
        on_side = torch_ops.ssim3d(xq, y)
        on_side.sum().backward()
    side.synchronize()
    assert torch.equal(on_side, want) and torch.equal(xq.grad, xc.grad)


def empty_leading_shape(ctx):
    x = torch.zeros(0, 2, 4, 5, 6, device="cuda", requires_grad=True)
    s = torch_ops.ssim3d(x, torch.zeros(0, 2, 4, 5, 6, device="cuda"))
    assert s.shape == (0, 2) and s.dtype == torch.float32
    s.sum().backward()
    assert x.grad.shape == x.shape
    v, w = volumes((4, 5, 6), 5)                                     # no leading dimension at all: a scalar
    assert torch_ops.ssim3d(v, w).shape == ()


def ssim_on_the_same_5d_tensor_is_unchanged_and_differs(ctx):
    x, y = volumes((2, 1, 6, 24, 24), 6)
    two_d = torch_ops.ssim(x, y)
    assert two_d.shape == (2, 1, 6)
    # unchanged: the 2-D C ABI on each slice, bit for bit
    n, (h, w) = 12, x.shape[-2:]
    ps = (ssim_amd.ParamsF * n)()
    for i in range(n):
        ps[i] = ssim_amd.make_params_f(w, h, x.data_ptr() + 4 * i * h * w, 1, w, y.data_ptr() + 4 * i * h * w, 1, w)
    torch.cuda.synchronize()
    vals = ctx.ssimf_device(ps, n, 1.0)
    assert np.array_equal(bits(two_d.cpu().numpy().reshape(-1)), bits(vals))
    three_d = torch_ops.ssim3d(x, y)
    assert three_d.shape == (2, 1)
    d = float((three_d - two_d.mean(-1)).abs().max())
    print("3-D against the mean of 2-D slices: %.3g" % d)
    assert d > 1e-3                                                  # a window across slices is another quantity
    for i in range(2):
        gv, _ = S.ssim(x[i, 0].cpu().numpy(), y[i, 0].cpu().numpy(), 1.0)
        assert abs(float(three_d[i, 0]) - gv) <= G_TOL


CHECKS = [value_and_gradients_against_the_model, loss_forms, non_contiguous_and_expanded_inputs, side_stream, empty_leading_shape,
          ssim_on_the_same_5d_tensor_is_unchanged_and_differs]


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
