#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_msssim3h.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints one line `RESULT {json}`: "ok" or the traceback per check.

The reference is always torch_ops.ms_ssim3d on x.float(), y.float() in this process: the value bit for bit, the gradient that call's
float32 gradient rounded once into the inputs' dtype (torch's .to(dtype) rounds to nearest-even, keeps float16 subnormals and overflows to
Inf: tests/test_ssimh_cpu.py holds tests/halfmodel.py to it).

usage (GPU box):  python tests/tools/msssim3h_torch_checks.py
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

import ssim_amd                                     # noqa: E402,F401
from ssim_amd import torch_ops                      # noqa: E402

HALVES = (torch.float16, torch.bfloat16)


def volumes(shape, seed, dtype):
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(a).cuda().to(dtype), torch.from_numpy(b).cuda().to(dtype)


def same(got, want):
    """Two tensors of one dtype with the same bits, NaN compared as NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(got[~gn], want[~wn]))


def reference(x, y, w, scales, weights, want_x=True, want_y=True):
    """ms_ssim3d on the widened tensors: (values, dA rounded once or None, dB rounded once or None)."""
    xf, yf = x.float().contiguous().requires_grad_(want_x), y.float().contiguous().requires_grad_(want_y)
    s = torch_ops.ms_ssim3d(xf, yf, 1.0, scales, weights)
    (s * w).sum().backward()
    return s.detach(), (xf.grad.to(x.dtype) if want_x else None), (yf.grad.to(y.dtype) if want_y else None)


def forward_and_backward_are_the_float32_path_rounded_once():
    for dtype in HALVES:
        x, y = volumes((2, 2, 9, 20, 33), 1, dtype)
        # dLoss/dS of the order of the voxel count: the float16 gradients land in the normal range
        w = torch.tensor([[1.0, -0.5], [0.25, 2.0]], device="cuda") * float(9 * 20 * 33)
        for scales, weights in ((5, None), (3, (0.5, 0.0, 0.5)), (1, (1.0,)), (3, (0.0, 0.5, 0.5))):
            for want_x, want_y in ((True, False), (False, True), (True, True)):
                xs, ys = x.clone().requires_grad_(want_x), y.clone().requires_grad_(want_y)
                s = torch_ops.ms_ssim3d_amp(xs, ys, 1.0, scales, weights)
                assert s.shape == (2, 2) and s.dtype == torch.float32
                (s * w).sum().backward()
                v, ga, gb = reference(x, y, w, scales, weights, want_x, want_y)
                assert same(s.detach(), v), (dtype, scales)
                assert (xs.grad is not None) == want_x and (ys.grad is not None) == want_y
                if want_x:
                    assert xs.grad.dtype == dtype and same(xs.grad, ga), (dtype, scales, "dA")
                    assert float(xs.grad.float().abs().max()) > 0
                if want_y:
                    assert ys.grad.dtype == dtype and same(ys.grad, gb), (dtype, scales, "dB")
    # float32 tensors take exactly ms_ssim3d's path
    x, y = volumes((2, 1, 9, 20, 33), 2, torch.float32)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    a, b = torch_ops.ms_ssim3d_amp(xa, y), torch_ops.ms_ssim3d(xb, y)
    a.sum().backward()
    b.sum().backward()
    assert same(a.detach(), b.detach()) and same(xa.grad, xb.grad)


def non_contiguous_and_expanded_inputs_are_read_in_place():
    torch.manual_seed(3)
    for dtype in HALVES:
        big_x, big_y = torch.rand(3, 4, 14, 30, 41, device="cuda").to(dtype), torch.rand(40, 3, 12, 26, device="cuda").to(dtype)
        x = big_x[0:2, 1:4:2, 2:12, 3:27, 5:39:2]                      # a channel slice (1, 3), offsets, step 2; an odd first sample
        y = big_y[3:37:2, 0:2, 1:11, 2:26].permute(1, 2, 3, 0)[:, None].expand(2, 2, 10, 24, 17)      # W stored outermost; one dimension expanded
        assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape and y.stride(1) == 0
        w = torch.full((2, 2), float(10 * 24 * 17), device="cuda")
        want, wa, wb = reference(x, y, w, 3, (0.2, 0.3, 0.5))
        xs, ys = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
        before = (big_x.clone(), big_y.clone())
        allocated = torch.cuda.memory_allocated()
        got = torch_ops.ms_ssim3d_amp(xs, ys, 1.0, 3, (0.2, 0.3, 0.5))
        # no copy and no widening of the inputs: the forward keeps the values and the float64 means, nothing of the volumes' size
        assert torch.cuda.memory_allocated() - allocated < x.numel()
        (got * w).sum().backward()
        assert same(got.detach(), want) and same(xs.grad, wa) and same(ys.grad, wb), dtype
        assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])


def loss_under_autocast_reaches_a_bfloat16_leaf_as_bfloat16():
    x, y = volumes((2, 1, 12, 18, 21), 4, torch.bfloat16)
    leaf = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = torch_ops.MSSSIM3DLoss()(leaf, y)
    assert loss.dtype == torch.float32 and loss.shape == ()
    (loss * 4096.0).backward()
    assert leaf.grad.dtype == torch.bfloat16
    v, ga, _ = reference(x, y, torch.full((2, 1), -4096.0 / 2.0, device="cuda"), 5, None, True, False)
    assert same(leaf.grad, ga) and float(leaf.grad.float().abs().max()) > 0
    assert abs(float(loss) - (1.0 - float(v.double().mean()))) < 1e-6
    # through a layer that autocast runs in bfloat16: the function takes the tensor as it comes
    lin = torch.nn.Conv3d(1, 1, 1).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = lin(x.float())
        assert out.dtype == torch.bfloat16
        torch_ops.MSSSIM3DLoss()(out, y).backward()
    assert lin.weight.grad is not None and bool(torch.isfinite(lin.weight.grad).all())


def side_stream():
    for dtype in HALVES:
        x, y = volumes((2, 1, 12, 18, 21), 5, dtype)
        xc = x.clone().requires_grad_(True)
        want = torch_ops.ms_ssim3d_amp(xc, y)                           # on the default stream
        (want * 4096.0).sum().backward()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            xq = x.clone().requires_grad_(True)
            on_side = torch_ops.ms_ssim3d_amp(xq, y)
            (on_side * 4096.0).sum().backward()
        side.synchronize()
        assert same(on_side.detach(), want.detach()) and same(xq.grad, xc.grad) and float(xq.grad.float().abs().max()) > 0


def loss_forms_on_sixteen_bit_tensors():
    for dtype in HALVES:
        x, y = volumes((3, 1, 7, 12, 12), 6, dtype)
        none = torch_ops.MSSSIM3DLoss(reduction="none", scales=2, weights=(0.5, 0.5))(x, y)
        assert none.shape == (3, 1) and none.dtype == torch.float32 and not none.requires_grad
        assert same(none, 1.0 - torch_ops.ms_ssim3d(x.float(), y.float(), 1.0, 2, (0.5, 0.5)))
        mean = torch_ops.MSSSIM3DLoss(scales=2, weights=(0.5, 0.5))(x, y)
        assert mean.shape == () and same(mean, none.mean())
        # an empty batch and no leading dimension at all
        e = torch.zeros(0, 2, 4, 5, 6, device="cuda", dtype=dtype, requires_grad=True)
        s = torch_ops.ms_ssim3d_amp(e, torch.zeros(0, 2, 4, 5, 6, device="cuda", dtype=dtype))
        assert s.shape == (0, 2) and s.dtype == torch.float32
        s.sum().backward()
        assert e.grad.shape == e.shape and e.grad.dtype == dtype
        assert torch_ops.ms_ssim3d_amp(x[0, 0], y[0, 0]).shape == ()


def refusals():
    x, y = volumes((1, 1, 7, 12, 12), 7, torch.float32)
    for dtype in HALVES:
        try:
            torch_ops.ms_ssim3d(x.to(dtype), y.to(dtype))               # ms_ssim3d still refuses 16-bit tensors
        except TypeError as e:
            assert str(e).startswith("ms_ssim3d: the 3-D multi-scale path is float32 for now"), str(e)
        else:
            raise AssertionError("no TypeError")
        for bad in (lambda: torch_ops.ms_ssim3d_amp(x.to(dtype), y), lambda: torch_ops.ms_ssim3d_amp(x, y.to(dtype)),
                    lambda: torch_ops.ms_ssim3d_amp(x.half(), y.bfloat16()), lambda: torch_ops.ms_ssim3d_amp(x.double(), y.double())):
            try:
                bad()
            except TypeError as e:
                assert str(e).startswith("ms_ssim3d_amp: "), str(e)
            else:
                raise AssertionError("no TypeError")
        h, k = x.to(dtype), y.to(dtype)
        for bad in (lambda: torch_ops.ms_ssim3d_amp(h, k, data_range=0.0), lambda: torch_ops.ms_ssim3d_amp(h, k[..., :-1]),
                    lambda: torch_ops.ms_ssim3d_amp(h, k.cpu()), lambda: torch_ops.ms_ssim3d_amp(h[0, 0, 0], k[0, 0, 0]),
                    lambda: torch_ops.ms_ssim3d_amp(h, k, scales=9), lambda: torch_ops.ms_ssim3d_amp(h, k, scales=3),
                    lambda: torch_ops.ms_ssim3d_amp(h, k, scales=2, weights=(1.0, -1.0))):
            try:
                bad()
            except ValueError as e:
                assert str(e).startswith("ms_ssim3d_amp: "), str(e)
            else:
                raise AssertionError("no ValueError")


CHECKS = [forward_and_backward_are_the_float32_path_rounded_once, non_contiguous_and_expanded_inputs_are_read_in_place,
          loss_under_autocast_reaches_a_bfloat16_leaf_as_bfloat16, side_stream, loss_forms_on_sixteen_bit_tensors, refusals]


def main():
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    result = {}
    for check in CHECKS:
        try:
            check()
            result[check.__name__] = "ok"
        except Exception:
            result[check.__name__] = traceback.format_exc()
        torch.cuda.synchronize()
    print("RESULT " + json.dumps(result))


if __name__ == "__main__":
    main()
