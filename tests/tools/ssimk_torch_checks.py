#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_ssimk.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/ssimk_torch_checks.py
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

import ssim_amd                                     # noqa: E402
from ssim_amd import torch_ops                      # noqa: E402
import ssimk_model as K                             # noqa: E402

SHAPE = (2, 3, 33, 31)
# (ssimk_model window, the keywords of torch_ops that select it)
WINDOWS = (((7, 1.5, "gaussian"), dict(win_size=7)), ((3, 0.0, "uniform"), dict(win_size=3, window="uniform")))


def tensors(shape=SHAPE, seed=3):
    torch.manual_seed(seed)
    x = torch.rand(shape, device="cuda")
    y = (x + 0.1 * torch.randn(shape, device="cuda")).clamp(0, 1)
    w = torch.randn(shape, device="cuda")
    return x, y, w


def same(t, u):
    """The same bits (the tensors here hold no NaN)."""
    assert t.dtype == u.dtype and t.shape == u.shape
    return torch.equal(t.contiguous().view(torch.int32), u.contiguous().view(torch.int32))


def abi_of_tensors(ctx, x, y, w, g_out, r, win):
    """The C ABI on the tensors' own memory (contiguous (N, C, H, W)) under the Window `win`: per-plane values, the map, the gradient of x
    for the scalar upstream gradients g_out (one per plane) and for the planes w."""
    torch.cuda.synchronize()
    n, (h, wd) = x.shape[0] * x.shape[1], x.shape[-2:]
    smap = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    sums = torch.empty(n, dtype=torch.float64, device=x.device)
    gs, gp = torch.empty_like(x), torch.empty_like(x)
    ps, ms = (ssim_amd.ParamsF * n)(), (ssim_amd.GradOutF * n)()
    ga, gb = (ssim_amd.GradF * n)(), (ssim_amd.GradF * n)()
    for i in range(n):
        o = i * h * wd
        ps[i] = ssim_amd.make_params_f(wd, h, x.data_ptr() + 4 * o, 1, wd, y.data_ptr() + 4 * o, 1, wd, smap.data_ptr() + 4 * o, 1, wd)
        ms[i] = ssim_amd.GradOutF(w.data_ptr() + 4 * o, 1, wd)
        ga[i], gb[i] = ssim_amd.GradF(gs.data_ptr() + 4 * o, 1, wd), ssim_amd.GradF(gp.data_ptr() + 4 * o, 1, wd)
    go = g_out.to(torch.float32).reshape(-1).contiguous()
    torch.cuda.synchronize()
    ctx.enqueue_ssimf(ps, n, r, sums.data_ptr(), window=win)
    ctx.enqueue_ssimf_grad(ps, n, r, go.data_ptr(), ga, None, window=win)
    ctx.enqueue_ssimf_map_grad(ps, n, r, ms, gb, None, window=win)
    ctx.synchronize()
    return (sums / (float(wd) * float(h))).to(torch.float32).reshape(x.shape[:-2]), smap, gs, gp


def forward_and_backward_are_the_c_abi_bit_for_bit(ctx):
    x, y, w = tensors()
    torch.manual_seed(5)
    g_out = torch.randn(SHAPE[:2], device="cuda")
    for window, kw in WINDOWS:
        win = ssim_amd.make_window(window[0], window[1] if window[2] == "gaussian" else 1.5, window[2])
        vals, smap, gs, gp = abi_of_tensors(ctx, x, y, w, g_out, 1.0, win)
        xs = x.clone().requires_grad_(True)
        s = torch_ops.ssim(xs, y, **kw)
        assert s.shape == SHAPE[:2] and same(s.detach(), vals)
        (g_out * s).sum().backward()
        assert same(xs.grad, gs) and float(xs.grad.abs().max()) > 0, window
        xm = x.clone().requires_grad_(True)
        m = torch_ops.ssim_map(xm, y, **kw)
        assert same(m.detach(), smap)
        (w * m).sum().backward()
        assert same(xm.grad, gp) and float(xm.grad.abs().max()) > 0, window
        # SSIMLoss: 1 - ssim, the mean over the planes
        xl = x.clone().requires_grad_(True)
        loss = torch_ops.SSIMLoss(**kw)(xl, y)
        assert same(loss.detach(), (1.0 - vals).mean())
        loss.backward()
        _, _, gl, _ = abi_of_tensors(ctx, x, y, w, torch.full(SHAPE[:2], -1.0 / (SHAPE[0] * SHAPE[1]), device="cuda"), 1.0, win)
        assert same(xl.grad, gl), window
        # the window changes the result
        assert not same(torch_ops.ssim(x, y, **kw), torch_ops.ssim(x, y))
        # a different window of the same size, and win_sigma ignored by the box
        if window[2] == "uniform":
            assert same(torch_ops.ssim(x, y, win_sigma=0.3, **kw), s.detach())
        else:
            assert not same(torch_ops.ssim(x, y, win_sigma=0.9, **kw), s.detach())


def slice_without_a_copy_and_a_side_stream(ctx):
    x, y, w = tensors()
    torch.manual_seed(11)
    big = torch.rand(2, 6, 40, 40, device="cuda")
    xv = big[:, 1::2, 3:36, 4:35]                                              # a channel slice of wider rows: not contiguous
    assert xv.shape == SHAPE and not xv.is_contiguous()
    for window, kw in WINDOWS:
        keep = big.clone()
        want_s, want_m = torch_ops.ssim(xv.contiguous(), y, **kw), torch_ops.ssim_map(xv.contiguous(), y, **kw)
        seen = []
        saved = ssim_amd.api.Context.enqueue_ssimf

        def spy(c, params, n, r, sums, window=None):
            seen.append([(params[i].imgA.topLeft, params[i].imgA.step, params[i].imgA.stride) for i in range(n)])
            return saved(c, params, n, r, sums, window=window)
        ssim_amd.api.Context.enqueue_ssimf = spy
        try:
            got_s = torch_ops.ssim(xv, y, **kw)
        finally:
            ssim_amd.api.Context.enqueue_ssimf = saved
        assert seen[0] == [(xv.data_ptr() + 4 * o, 1, 40) for o in torch_ops._plane_offsets(xv)]       # addressed in place
        assert same(got_s, want_s) and same(torch_ops.ssim_map(xv, y, **kw), want_m) and torch.equal(big, keep), window
        yr = y.clone().requires_grad_(True)
        gy, = torch.autograd.grad(torch_ops.ssim_map(xv, yr, **kw), yr, grad_outputs=w)
        gy2, = torch.autograd.grad(torch_ops.ssim_map(xv.contiguous(), yr, **kw), yr, grad_outputs=w)
        assert same(gy, gy2), window
        # a non-default stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            xq = x.clone().requires_grad_(True)
            on_side, = torch.autograd.grad(torch_ops.ssim_map(xq, y, **kw), xq, grad_outputs=w)
            s_side = torch_ops.ssim(x, y, **kw)
        side.synchronize()
        xq = x.clone().requires_grad_(True)
        here, = torch.autograd.grad(torch_ops.ssim_map(xq, y, **kw), xq, grad_outputs=w)
        assert same(on_side, here) and same(s_side, torch_ops.ssim(x, y, **kw)), window


def conv2d_ssim_map(x, y, r, window):
    """The float64 restatement: F.conv2d with the outer product of the window's taps on replicate-padded planes."""
    g = torch.tensor(K.full_taps(window), dtype=torch.float64, device=x.device)
    R = K.radius(window)
    k2 = (g[:, None] * g[None, :])[None, None]
    c1, c2 = K.constants(r)

    def blur(t):
        n, c, h, w = t.shape
        return Fn.conv2d(Fn.pad(t.reshape(n * c, 1, h, w), (R, R, R, R), mode="replicate"), k2).reshape(n, c, h, w)
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    return (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))


def gradient_agrees_with_the_conv2d_restatement(ctx):
    x, y, w = tensors()
    for window, kw in WINDOWS:
        px_tol, g_tol, grad_tol, _ = K.tolerances(window)
        xd, yd = x.double().requires_grad_(True), y.double().requires_grad_(True)
        ref = conv2d_ssim_map(xd, yd, 1.0, window)
        want_mean = torch.autograd.grad(ref.mean(dim=(-2, -1)).sum(), (xd, yd), retain_graph=True)
        want_map = torch.autograd.grad((w.double() * ref).sum(), (xd, yd))
        xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        m = torch_ops.ssim_map(xs, ys, **kw)
        s = torch_ops.ssim(xs, ys, **kw)
        e_px = float((m.detach().double() - ref.detach()).abs().max())
        e_g = float((s.detach().double() - ref.detach().mean(dim=(-2, -1))).abs().max())
        got_mean = torch.autograd.grad(s.sum(), (xs, ys))
        got_map = torch.autograd.grad((w * m).sum(), (xs, ys))
        print("%s: per pixel %.3g (bound %.3g), per plane %.3g (bound %.3g)" % (K.name_of(window), e_px, px_tol, e_g, g_tol))
        assert e_px <= px_tol and e_g <= g_tol, window
        for what, got, want in (("mean", got_mean, want_mean), ("map", got_map, want_map)):
            for g, wt in zip(got, want):
                for i in range(SHAPE[0]):
                    for c in range(SHAPE[1]):
                        e = float((g[i, c].double() - wt[i, c]).abs().max() / wt[i, c].abs().max())
                        assert e <= grad_tol, (window, what, i, c, e)


def default_arguments_are_todays_call_bit_for_bit(ctx):
    x, y, w = tensors()
    seen = []
    saved = (ssim_amd.api.Context.enqueue_ssimf, ssim_amd.api.Context.enqueue_ssimf_grad, ssim_amd.api.Context.enqueue_ssimf_map_grad)

    def spy(k):
        def f(*a, **kwargs):
            seen.append(kwargs.get("window"))
            return saved[k](*a, **kwargs)
        return f
    ssim_amd.api.Context.enqueue_ssimf, ssim_amd.api.Context.enqueue_ssimf_grad, ssim_amd.api.Context.enqueue_ssimf_map_grad = spy(0), spy(1), spy(2)
    try:
        out = []
        for kw in (dict(), dict(win_size=11, win_sigma=1.5, window="gaussian")):
            xs = x.clone().requires_grad_(True)
            s = torch_ops.ssim(xs, y, **kw)
            gs, = torch.autograd.grad(s.sum(), xs)
            m = torch_ops.ssim_map(xs, y, **kw)
            gm, = torch.autograd.grad((w * m).sum(), xs)
            xl = x.clone().requires_grad_(True)
            loss = torch_ops.SSIMLoss(**kw)(xl, y)
            loss.backward()
            out.append((s.detach(), gs, m.detach(), gm, loss.detach(), xl.grad))
    finally:
        ssim_amd.api.Context.enqueue_ssimf, ssim_amd.api.Context.enqueue_ssimf_grad, ssim_amd.api.Context.enqueue_ssimf_map_grad = saved
    assert len(seen) == 12 and all(v is None for v in seen), seen              # every call took the entry without _win
    assert all(same(p, q) for p, q in zip(out[0], out[1]))
    # and the C ABI's entries without a window give those bits
    h, wd = SHAPE[-2:]
    vals, smap, gs, gp = abi_of_tensors(ctx, x, y, w, torch.ones(SHAPE[:2], device="cuda"), 1.0, None)
    assert same(out[0][0], vals) and same(out[0][1], gs) and same(out[0][2], smap) and same(out[0][3], gp)
    # 16-bit tensors keep working with the defaults, and refuse a window
    hx, hy = x.half(), y.half()
    assert torch_ops.ssim(hx, hy).dtype == torch.float32
    try:
        torch_ops.ssim(hx, hy, win_size=7)
    except TypeError as e:
        assert "fixed window" in str(e)
    else:
        raise AssertionError("no TypeError")
    assert np.isfinite(float(torch_ops.SSIMLoss()(hx, hy)))


CHECKS = [forward_and_backward_are_the_c_abi_bit_for_bit, slice_without_a_copy_and_a_side_stream, gradient_agrees_with_the_conv2d_restatement,
          default_arguments_are_todays_call_bit_for_bit]


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
