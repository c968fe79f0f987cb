#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_ssim3k.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

The yardstick is a composite written here in torch float64 on the CPU -- F.conv3d per axis on replicate-padded volumes with the
window's float32 taps, the five statistics, autograd --, at the window's bounds of tests/ssim3k_model.py.

usage (GPU box):  python tests/tools/ssim3k_torch_checks.py
"""
import json
import os
import sys
import traceback

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ssim_amd                                     # noqa: E402,F401
import ssim3k_model as K3                           # noqa: E402
from ssim_amd import torch_ops                      # noqa: E402

WINDOWS = ((3, 0.0, "uniform"), (7, 1.5, "gaussian"), (11, 2.0, "gaussian"))


def kw(window):
    size, sigma, kind = window
    return dict(win_size=size, win_sigma=sigma if kind == "gaussian" else 1.5, window=kind)


def volumes(shape, seed):
    """x, y of `shape` (..., D, H, W): random volumes in [0, 1] and a noisy copy."""
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def composite(x, y, data_range, window):
    """(per-volume SSIM, map) of two float64 CPU tensors (..., D, H, W), differentiable."""
    g = torch.tensor(K3.full_taps(window), dtype=torch.float64)
    R, n = K3.radius(window), 2 * K3.radius(window) + 1
    c1, c2 = K3.constants(data_range)
    lead = x.shape[:-3]

    def blur(v):
        v = v.reshape((-1, 1) + tuple(v.shape[-3:]))
        v = Fn.conv3d(Fn.pad(v, (R, R, 0, 0, 0, 0), mode="replicate"), g.reshape(1, 1, 1, 1, n))
        v = Fn.conv3d(Fn.pad(v, (0, 0, R, R, 0, 0), mode="replicate"), g.reshape(1, 1, 1, n, 1))
        v = Fn.conv3d(Fn.pad(v, (0, 0, 0, 0, R, R), mode="replicate"), g.reshape(1, 1, n, 1, 1))
        return v.reshape(x.shape)
    ma, mb = blur(x), blur(y)
    s_aa, s_bb, s_ab = blur(x * x) - ma * ma, blur(y * y) - mb * mb, blur(x * y) - ma * mb
    m = (2 * ma * mb + c1) * (2 * s_ab + c2) / ((ma * ma + mb * mb + c1) * (s_aa + s_bb + c2))
    return m.reshape(lead + (-1,)).sum(-1) / (float(x.shape[-1]) * float(x.shape[-2]) * float(x.shape[-3])), m


def rel_per_volume(got, want):
    """The worst, over the volumes, of max|got - want| over the volume's largest |want|."""
    got, want = got.detach().double().cpu(), want.detach()
    lead = got.shape[:-3]
    e = (got - want).abs().reshape(lead + (-1,)).amax(-1) / want.abs().reshape(lead + (-1,)).amax(-1)
    return float(e.max())


def value_map_and_loss_against_the_conv3d_composite(ctx):
    x, y = volumes((2, 2, 9, 20, 33), 1)
    w = torch.tensor([[1.0, -0.5], [0.25, 2.0]])
    torch.manual_seed(7)
    wm = torch.randn(x.shape) * (torch.rand(x.shape) < 0.5)                    # a signed weight under a mask
    for window in WINDOWS:
        px_tol, g_tol, grad_tol, _, mapgrad_tol = K3.tolerances(window)
        for r in (1.0, 255.0):
            xr, yr = (x * r), (y * r)
            # the float64 composite and its three backwards
            cx, cy = xr.double().cpu().requires_grad_(True), yr.double().cpu().requires_grad_(True)
            cs, cm = composite(cx, cy, r, window)
            g_mean = torch.autograd.grad((cs * w).sum(), (cx, cy), retain_graph=True)
            g_map = torch.autograd.grad((cm * wm).sum(), (cx, cy), retain_graph=True)
            g_loss = torch.autograd.grad(1.0 - cs.mean(), (cx, cy))
            # ssim3d
            xs, ys = xr.clone().requires_grad_(True), yr.clone().requires_grad_(True)
            s = torch_ops.ssim3d(xs, ys, r, **kw(window))
            assert s.shape == (2, 2) and s.dtype == torch.float32
            (s * w.cuda()).sum().backward()
            ev = float((s.double().cpu() - cs.detach()).abs().max())
            ea, eb = rel_per_volume(xs.grad, g_mean[0]), rel_per_volume(ys.grad, g_mean[1])
            # ssim3d_map
            xm, ym = xr.clone().requires_grad_(True), yr.clone().requires_grad_(True)
            m = torch_ops.ssim3d_map(xm, ym, r, **kw(window))
            assert m.shape == x.shape and m.dtype == torch.float32
            (m * wm.cuda()).sum().backward()
            ep = float((m.double().cpu() - cm.detach()).abs().max())
            ma, mb = rel_per_volume(xm.grad, g_map[0]), rel_per_volume(ym.grad, g_map[1])
            # SSIM3DLoss
            xl, yl = xr.clone().requires_grad_(True), yr.clone().requires_grad_(True)
            loss = torch_ops.SSIM3DLoss(r, "mean", **kw(window))(xl, yl)
            loss.backward()
            el = abs(float(loss) - float(1.0 - cs.mean()))
            la, lb = rel_per_volume(xl.grad, g_loss[0]), rel_per_volume(yl.grad, g_loss[1])
            none = torch_ops.SSIM3DLoss(r, "none", **kw(window))(xr, yr)
            print("%s at range %g: value %.3g (%.3g), map %.3g (%.3g), gradients %.3g %.3g (%.3g), map gradients %.3g %.3g (%.3g), loss %.3g, "
                  "its gradients %.3g %.3g" % (K3.name_of(window), r, ev, g_tol, ep, px_tol, ea, eb, grad_tol, ma, mb, mapgrad_tol, el, la, lb))
            assert ev <= g_tol and ep <= px_tol and max(ea, eb) <= grad_tol and max(ma, mb) <= mapgrad_tol
            assert el <= g_tol and max(la, lb) <= grad_tol
            assert none.shape == (2, 2) and torch.equal(none, 1.0 - s.detach())
    # the windows are read: three different values for the same volumes
    vals = [float(torch_ops.ssim3d(x, y, **kw(window))[0, 0]) for window in WINDOWS]
    assert len(set(vals)) == 3, vals


def non_contiguous_expanded_sum_and_y_only(ctx):
    torch.manual_seed(3)
    big_x, big_y = torch.rand(3, 4, 14, 30, 40, device="cuda"), torch.rand(40, 3, 12, 26, device="cuda")
    x = big_x[0:2, 1:4:2, 2:12, 3:27, 5:39:2]                      # (2, 2, 10, 24, 17): offsets, step 2
    y = big_y[3:37:2, 0:2, 1:11, 2:26].permute(1, 2, 3, 0)[:, None].expand(2, 2, 10, 24, 17)      # W stored outermost; the second dimension expanded
    assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape and y.stride(1) == 0
    for window in WINDOWS:
        grad_tol, mapgrad_tol = K3.tolerances(window)[2], K3.tolerances(window)[4]
        xc, yc = x.contiguous().requires_grad_(True), y.contiguous().requires_grad_(True)
        want = torch_ops.ssim3d(xc, yc, **kw(window))
        want.sum().backward()
        xs, ys = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
        assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride() and ys.stride() == y.stride()
        before = (big_x.clone(), big_y.clone())
        got = torch_ops.ssim3d(xs, ys, **kw(window))
        got.sum().backward()
        assert torch.equal(got, want) and torch.equal(xs.grad, xc.grad) and torch.equal(ys.grad, yc.grad)
        assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])
        # the map: sum().backward() hands the backward an expanded grad_out (strides 0), read in place
        xm, ym = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
        seen = []
        m = torch_ops.ssim3d_map(xm, ym, **kw(window))
        m.register_hook(lambda g: seen.append(g))
        m.sum().backward()
        assert len(seen) == 1 and seen[0].shape == x.shape
        print("%s: the grad_out of sum() arrives with strides %r" % (K3.name_of(window), tuple(seen[0].stride())))
        cx, cy = x.double().cpu().requires_grad_(True), y.double().cpu().requires_grad_(True)
        cs, cm = composite(cx, cy, 1.0, window)
        g_map = torch.autograd.grad(cm.sum(), (cx, cy), retain_graph=True)
        g_mean = torch.autograd.grad(cs.sum(), (cx, cy))
        ea, eb = rel_per_volume(xm.grad, g_map[0]), rel_per_volume(ym.grad, g_map[1])
        fa, fb = rel_per_volume(xs.grad, g_mean[0]), rel_per_volume(ys.grad, g_mean[1])
        print("%s: non-contiguous map gradients %.3g %.3g (%.3g), mean gradients %.3g %.3g (%.3g)" % (K3.name_of(window), ea, eb, mapgrad_tol, fa, fb, grad_tol))
        assert max(ea, eb) <= mapgrad_tol and max(fa, fb) <= grad_tol
        # a gradient wanted for y only: the bits it has together with x's
        y2 = y.detach().requires_grad_(True)
        torch_ops.ssim3d(x, y2, **kw(window)).sum().backward()
        assert torch.equal(y2.grad, ys.grad)
        y3 = y.detach().requires_grad_(True)
        torch_ops.ssim3d_map(x, y3, **kw(window)).sum().backward()
        assert torch.equal(y3.grad, ym.grad)
        loss = torch_ops.SSIM3DLoss(**kw(window))
        y4 = y.detach().requires_grad_(True)
        loss(x, y4).backward()
        assert rel_per_volume(y4.grad, -g_mean[1] / 4.0) <= grad_tol


def default_keywords_are_the_call_without_keywords(ctx):
    x, y = volumes((2, 1, 9, 20, 33), 4)
    default = dict(win_size=11, win_sigma=1.5, window="gaussian")
    for fn in (torch_ops.ssim3d, torch_ops.ssim3d_map, torch_ops.ssim3d_amp, torch_ops.ssim3d_map_amp):
        outs = []
        for k in ({}, default):
            xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            out = fn(xs, ys, 1.0, **k)
            (out * out).sum().backward()
            outs.append((out.detach(), xs.grad, ys.grad))
        assert all(torch.equal(p, q) for p, q in zip(*outs)), fn.__name__
        other = fn(x, y, 1.0, win_size=9)
        assert not torch.equal(other, outs[0][0]), fn.__name__
    a = torch_ops.SSIM3DLoss()(x, y)
    b = torch_ops.SSIM3DLoss(1.0, "mean", 11, 1.5, "gaussian")(x, y)
    assert torch.equal(a, b)


def bfloat16_with_the_default_window_still_works(ctx):
    x, y = volumes((2, 1, 9, 20, 33), 5)
    for dtype in (torch.bfloat16, torch.float16):
        xh, yh = x.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
        s = torch_ops.ssim3d_amp(xh, yh, 1.0, win_size=11, win_sigma=1.5, window="gaussian")
        s.sum().backward()
        want = torch_ops.ssim3d(xh.detach().float(), yh.detach().float())
        assert s.dtype == torch.float32 and torch.equal(s, want) and xh.grad.dtype == dtype and bool(torch.isfinite(xh.grad.float()).all())
        m = torch_ops.ssim3d_map_amp(xh.detach(), yh.detach())
        assert torch.equal(m, torch_ops.ssim3d_map(xh.detach().float(), yh.detach().float()))
        loss = torch_ops.SSIM3DLoss()(xh.detach(), yh.detach())
        assert abs(float(loss) - (1.0 - float(want.double().mean()))) < 1e-6


CHECKS = [value_map_and_loss_against_the_conv3d_composite, non_contiguous_expanded_sum_and_y_only,
          default_keywords_are_the_call_without_keywords, bfloat16_with_the_default_window_still_works]


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
