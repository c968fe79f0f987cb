#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_ssim3w.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/ssim3w_torch_checks.py
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
import ssim3w_model as MW                           # noqa: E402
from ssim_amd import torch_ops                      # noqa: E402

GRAD_TOL = MW.tolerances()


def volumes(shape, seed):
    """x, y of `shape` (..., D, H, W): random volumes in [0, 1] and a noisy copy."""
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def rel(t, g):
    return float(np.abs(t.cpu().numpy() - g).max() / np.abs(g).max())


def map_is_the_map_of_compute_ssim3f(ctx):
    x, y = volumes((2, 2, 9, 20, 33), 1)
    m = torch_ops.ssim3d_map(x, y)
    assert m.shape == x.shape and m.dtype == torch.float32 and m.is_contiguous() and not m.requires_grad
    for i in range(2):
        for c in range(2):
            _, want = ssim_amd.compute_ssim3f(x[i, c].cpu().numpy(), y[i, c].cpu().numpy(), 1.0, want_map=True, ctx=ctx)
            assert np.array_equal(m[i, c].cpu().numpy().view(np.uint32), want.view(np.uint32)), (i, c)
    # the mean of the map is ssim3d to the rounding of a float32 mean
    assert float((m.double().mean(dim=(-3, -2, -1)) - torch_ops.ssim3d(x, y).double()).abs().max()) < 1e-6
    # no leading dimension, and an empty one
    v, w = volumes((4, 5, 6), 5)
    assert torch_ops.ssim3d_map(v, w).shape == (4, 5, 6)
    e = torch.zeros(0, 2, 4, 5, 6, device="cuda", requires_grad=True)
    me = torch_ops.ssim3d_map(e, torch.zeros(0, 2, 4, 5, 6, device="cuda"))
    assert me.shape == e.shape
    me.sum().backward()
    assert e.grad.shape == e.shape


def weighted_sum_against_the_model(ctx):
    x, y = volumes((2, 2, 9, 20, 33), 2)
    torch.manual_seed(7)
    w = torch.randn(x.shape, device="cuda") * (torch.rand(x.shape, device="cuda") < 0.5)      # a signed weight under a mask
    grads = {}
    for want_x, want_y in ((True, False), (False, True), (True, True)):
        xs, ys = x.clone().requires_grad_(want_x), y.clone().requires_grad_(want_y)
        (w * torch_ops.ssim3d_map(xs, ys)).sum().backward()
        assert (xs.grad is not None) == want_x and (ys.grad is not None) == want_y
        grads[(want_x, want_y)] = (xs.grad, ys.grad)
    for i in range(2):
        for c in range(2):
            ga, gb = MW.grad_map(x[i, c].cpu().numpy(), y[i, c].cpu().numpy(), 1.0, w[i, c].cpu().numpy())
            ea, eb = rel(grads[(True, True)][0][i, c], ga), rel(grads[(True, True)][1][i, c], gb)
            print("weighted sum: volume %d,%d gradients %.3g %.3g of max|grad|" % (i, c, ea, eb))
            assert max(ea, eb) <= GRAD_TOL, (i, c, ea, eb)
    # one gradient or both: the same bits
    assert torch.equal(grads[(True, False)][0], grads[(True, True)][0]) and torch.equal(grads[(False, True)][1], grads[(True, True)][1])
    # the masked mean of the issue, at range 255, and a float64 weight (grad_out is cast to float32 once)
    mask = (torch.rand(x.shape, device="cuda") < 0.3).double()
    xs = (x * 255).requires_grad_(True)
    loss = 1 - (mask * torch_ops.ssim3d_map(xs, y * 255, 255.0)).sum() / mask.sum()
    loss.backward()
    k = (-mask / mask.sum()).float().cpu().numpy()
    g = MW.grad_map((x[1, 0] * 255).cpu().numpy(), (y[1, 0] * 255).cpu().numpy(), 255.0, k[1, 0])[0]
    e = rel(xs.grad[1, 0], g)
    print("masked mean at range 255: %.3g of max|grad|" % e)
    assert e <= GRAD_TOL, e


def mean_over_the_volume_against_ssim3d(ctx):
    """ssim3d_map(x, y).mean over each volume hands the backward an expanded grad_out.  Where every element of it is
    float(gOut / voxels), the gradient has the bits of ssim3d's backward for gOut; where torch's division rounds otherwise, it is held
    to the model at the bound."""
    x, y = volumes((2, 2, 9, 20, 33), 3)
    g_out = torch.tensor([[1.0, -0.5], [0.25, 2.0]], device="cuda")
    vox = 9.0 * 20.0 * 33.0
    seen = []
    xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    m = torch_ops.ssim3d_map(xs, ys)
    m.register_hook(lambda g: seen.append(g))
    (m.mean(dim=(-3, -2, -1)) * g_out).sum().backward()
    assert len(seen) == 1 and seen[0].shape == x.shape and seen[0].dtype == torch.float32
    print("mean: grad_out arrives with strides %r" % (tuple(seen[0].stride()),))
    xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    (torch_ops.ssim3d(xr, yr) * g_out).sum().backward()
    for i in range(2):
        for c in range(2):
            k = float(seen[0][i, c, 0, 0, 0])
            exact = np.float32(float(g_out[i, c]) / vox)
            if bool((seen[0][i, c] == float(exact)).all()):
                assert torch.equal(xs.grad[i, c], xr.grad[i, c]) and torch.equal(ys.grad[i, c], yr.grad[i, c]), (i, c)
                print("mean: volume %d,%d grad_out is float(gOut / voxels): the bits of ssim3d" % (i, c))
            else:
                ga, gb = S.grad(x[i, c].cpu().numpy(), y[i, c].cpu().numpy(), 1.0, float(g_out[i, c]))
                ea, eb = rel(xs.grad[i, c], ga), rel(ys.grad[i, c], gb)
                print("mean: volume %d,%d grad_out %r is not float(gOut / voxels) %r: %.3g %.3g of max|grad|" % (i, c, k, float(exact), ea, eb))
                assert max(ea, eb) <= GRAD_TOL, (i, c, ea, eb)


def non_contiguous_x_and_sliced_grad_out_are_read_in_place(ctx):
    torch.manual_seed(3)
    big_x, big_y = torch.rand(3, 4, 14, 30, 40, device="cuda"), torch.rand(40, 3, 12, 26, device="cuda")
    x = big_x[0:2, 1:4:2, 2:12, 3:27, 5:39:2]                      # (2, 2, 10, 24, 17): offsets, step 2
    y = big_y[3:37:2, 0:2, 1:11, 2:26].permute(1, 2, 3, 0)[:, None].expand(2, 2, 10, 24, 17)      # W stored outermost; the second dimension expanded
    assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape and y.stride(1) == 0
    big_w = torch.randn(2, 2, 24, 10, 40, device="cuda")
    w = big_w[..., 3:37:2].permute(0, 1, 3, 2, 4)                  # (2, 2, 10, 24, 17): H and D exchanged in storage, step 2
    assert w.shape == x.shape and not w.is_contiguous()
    xc, yc = x.contiguous().requires_grad_(True), y.contiguous().requires_grad_(True)
    want = torch_ops.ssim3d_map(xc, yc)
    want.backward(w.contiguous())
    xs, ys = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
    assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride() and ys.stride() == y.stride()
    before = (big_x.clone(), big_y.clone(), big_w.clone())
    got = torch_ops.ssim3d_map(xs, ys)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got.backward(w)                                                # a sliced, permuted grad_out
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 3 * x.numel() * 4, peak                          # the two gradients only: no contiguous copy of grad_out, x or y
    assert torch.equal(got, want) and torch.equal(xs.grad, xc.grad) and torch.equal(ys.grad, yc.grad)
    assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1]) and torch.equal(big_w, before[2])
    ga = MW.grad_map(x[1, 0].cpu().numpy(), y[1, 0].cpu().numpy(), 1.0, w[1, 0].cpu().numpy())[0]
    assert rel(xs.grad[1, 0], ga) <= GRAD_TOL
    # it keeps x and y, not the map
    m = torch_ops.ssim3d_map(xc, yc)
    saved = [t.data_ptr() for t in m.grad_fn.saved_tensors]
    assert sorted(saved) == sorted([xc.data_ptr(), yc.data_ptr()]) and m.data_ptr() not in saved


def side_stream(ctx):
    x, y = volumes((2, 1, 12, 18, 21), 4)
    torch.manual_seed(5)
    w = torch.randn(x.shape, device="cuda")
    xc = x.clone().requires_grad_(True)
    want = torch_ops.ssim3d_map(xc, y)                               # on the default stream
    (w * want).sum().backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xq = x.clone().requires_grad_(True)
        on_side = torch_ops.ssim3d_map(xq, y)
        (w * on_side).sum().backward()
    side.synchronize()
    assert torch.equal(on_side, want) and torch.equal(xq.grad, xc.grad)
    g = MW.grad_map(x[0, 0].cpu().numpy(), y[0, 0].cpu().numpy(), 1.0, w[0, 0].cpu().numpy())[0]
    assert rel(xq.grad[0, 0], g) <= GRAD_TOL


CHECKS = [map_is_the_map_of_compute_ssim3f, weighted_sum_against_the_model, mean_over_the_volume_against_ssim3d,
          non_contiguous_x_and_sliced_grad_out_are_read_in_place, side_stream]


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
