#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_ssimw.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/ssimw_torch_checks.py
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
from ssim_amd import api, torch_ops                 # noqa: E402
from ssimw_model import WGRAD_TOL                   # noqa: E402

SHAPE = (2, 3, 33, 31)


def tensors(dtype, shape=SHAPE, seed=3):
    torch.manual_seed(seed)
    x = torch.rand(shape, device="cuda")
    y = (x + 0.1 * torch.randn(shape, device="cuda")).clamp(0, 1)
    w = torch.randn(shape, device="cuda")
    return x.to(dtype), y.to(dtype), w


def same(t, u):
    """The same bits (the gradients here hold no NaN)."""
    assert t.dtype == u.dtype and t.shape == u.shape
    v = torch.int32 if t.dtype == torch.float32 else torch.int16
    return torch.equal(t.contiguous().view(v), u.contiguous().view(v))


def abi_of_tensors(ctx, x, y, w, r):
    """The C ABI on the tensors' own memory (contiguous (N, C, H, W)): the map, and the gradient of x for the weight planes w."""
    torch.cuda.synchronize()
    n, (h, wd) = x.shape[0] * x.shape[1], x.shape[-2:]
    es = x.element_size()
    st = {torch.float16: ssim_amd.SAMPLE_F16, torch.bfloat16: ssim_amd.SAMPLE_BF16}.get(x.dtype)
    smap = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    sums = torch.empty(n, dtype=torch.float64, device=x.device)
    gx = torch.empty_like(x)
    ps = ((ssim_amd.ParamsF if st is None else ssim_amd.Params16) * n)()
    make = ssim_amd.make_params_f if st is None else ssim_amd.make_params16
    ms, ga = (ssim_amd.GradOutF * n)(), ((ssim_amd.GradF if st is None else ssim_amd.GradH) * n)()
    for i in range(n):
        o = i * h * wd
        ps[i] = make(wd, h, x.data_ptr() + es * o, 1, wd, y.data_ptr() + es * o, 1, wd, smap.data_ptr() + 4 * o, 1, wd)
        ms[i] = ssim_amd.GradOutF(w.data_ptr() + 4 * o, 1, wd)
        ga[i] = type(ga[0])(gx.data_ptr() + es * o, 1, wd)
    torch.cuda.synchronize()
    if st is None:
        ctx.enqueue_ssimf(ps, n, r, sums.data_ptr())
        ctx.enqueue_ssimf_map_grad(ps, n, r, ms, ga, None)
    else:
        ctx.enqueue_ssimh(ps, n, r, st, sums.data_ptr())
        ctx.enqueue_ssimh_map_grad(ps, n, r, st, ms, ga, None)
    ctx.synchronize()
    return smap, gx


class Recorded(object):
    """Records the gMap descriptors ssim_map's backward hands to the library: [(topLeft, step, stride)] of the last call."""

    def __enter__(self):
        self.maps = None
        self.saved = (api.Context.enqueue_ssimf_map_grad, api.Context.enqueue_ssimh_map_grad)
        rec = self

        def f(ctx, params, n, r, maps, ga=None, gb=None):
            rec.maps = [(maps[i].topLeft, maps[i].step, maps[i].stride) for i in range(n)]
            return rec.saved[0](ctx, params, n, r, maps, ga, gb)

        def h(ctx, params, n, r, st, maps, ga=None, gb=None):
            rec.maps = [(maps[i].topLeft, maps[i].step, maps[i].stride) for i in range(n)]
            return rec.saved[1](ctx, params, n, r, st, maps, ga, gb)
        api.Context.enqueue_ssimf_map_grad, api.Context.enqueue_ssimh_map_grad = f, h
        return self

    def __exit__(self, *exc):
        api.Context.enqueue_ssimf_map_grad, api.Context.enqueue_ssimh_map_grad = self.saved


def in_place(maps, g):
    """The descriptors address g itself, plane by plane, through g's own strides."""
    want = [(g.data_ptr() + 4 * o, g.stride(-1), g.stride(-2)) for o in torch_ops._plane_offsets(g)]
    return maps == want


def map_and_backward_are_the_c_abi_bit_for_bit(ctx):
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        x, y, w = tensors(dtype)
        x = x.clone().requires_grad_(True)
        m = torch_ops.ssim_map(x, y)
        assert m.shape == x.shape and m.dtype == torch.float32 and m.requires_grad
        (w * m).sum().backward()
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        smap, gx = abi_of_tensors(ctx, x.detach(), y, w, 1.0)
        assert same(m.detach(), smap) and float(m.detach().abs().max()) > 0.1
        assert same(x.grad, gx) and float(x.grad.float().abs().max()) > 0, dtype
        # the per-plane mean of the map is ssim()
        s = torch_ops.ssim(x.detach(), y)
        assert float((m.detach().double().mean(dim=(-2, -1)) - s.double()).abs().max()) < 1e-6
        # x and y together, and y alone: only what needs a gradient gets one, with the same bits
        x2, y2 = x.detach().clone().requires_grad_(True), y.clone().requires_grad_(True)
        (w * torch_ops.ssim_map(x2, y2)).sum().backward()
        assert same(x2.grad, gx) and y2.grad.dtype == dtype
        y3 = y.clone().requires_grad_(True)
        (w * torch_ops.ssim_map(x.detach(), y3)).sum().backward()
        assert same(y3.grad, y2.grad)
        assert not torch_ops.ssim_map(x.detach(), y).requires_grad
        for bad, exc in ((lambda: torch_ops.ssim_map(x.detach(), y, data_range=0.0), ValueError), (lambda: torch_ops.ssim_map(x.detach(), y[:, :, :-1]), ValueError),
                         (lambda: torch_ops.ssim_map(x.detach(), y.cpu()), ValueError), (lambda: torch_ops.ssim_map(x.detach(), y.double()), TypeError)):
            try:
                bad()
            except exc:
                continue
            raise AssertionError("no %s" % exc.__name__)


def mean_runs_on_the_grad_out_it_is_handed_and_agrees_with_ssim(ctx):
    x, y, _ = tensors(torch.float32)
    seen = []
    for reduce in ("sum", "mean"):
        xs = x.clone().requires_grad_(True)
        m = torch_ops.ssim_map(xs, y)
        m.register_hook(lambda g: seen.append(g))
        with Recorded() as rec:
            getattr(m, reduce)().backward()
        g = seen[-1]
        print("%s().backward() hands grad_out with strides %s" % (reduce, tuple(g.stride())))
        assert in_place(rec.maps, g), (reduce, rec.maps)                   # read where it is: no copy, whatever its strides
        if reduce == "sum":                                                # an expanded scalar: one float stands for every plane
            assert tuple(g.stride()) == (0, 0, 0, 0) and rec.maps == [(g.data_ptr(), 0, 0)] * 6
            want = x.clone().requires_grad_(True)
            torch_ops.ssim(want, y).sum().mul(float(SHAPE[-1] * SHAPE[-2])).backward()
        else:
            want = x.clone().requires_grad_(True)
            torch_ops.ssim(want, y).mean().backward()
        # k differs by at most an ulp between the two routes: agreement, not bits
        for i in range(SHAPE[0]):
            for c in range(SHAPE[1]):
                e = float((xs.grad[i, c].double() - want.grad[i, c].double()).abs().max() / want.grad[i, c].double().abs().max())
                assert e <= WGRAD_TOL, (reduce, i, c, e)
    # an expanded grad_out given directly
    xs = x.clone().requires_grad_(True)
    one = torch.full((1, 1, 1, 1), 0.5, device="cuda").expand(SHAPE)
    with Recorded() as rec:
        gx, = torch.autograd.grad(torch_ops.ssim_map(xs, y), xs, grad_outputs=one)
    assert rec.maps == [(one.data_ptr(), 0, 0)] * 6
    dense, = torch.autograd.grad(torch_ops.ssim_map(xs, y), xs, grad_outputs=one.contiguous())
    assert same(gx, dense)


def grad_out_slice_stream_and_needs_input_grad(ctx):
    for dtype in (torch.float32, torch.bfloat16):
        x, y, _ = tensors(dtype)
        torch.manual_seed(11)
        big = torch.randn(2, 6, 33, 40, device="cuda")
        w = big[:, 1::2, :, 4:35]                                          # a channel slice of wider rows: not contiguous
        assert w.shape == SHAPE and not w.is_contiguous()
        xs = x.clone().requires_grad_(True)
        want, = torch.autograd.grad(torch_ops.ssim_map(xs, y), xs, grad_outputs=w.contiguous())
        keep = big.clone()
        with Recorded() as rec:
            got, = torch.autograd.grad(torch_ops.ssim_map(xs, y), xs, grad_outputs=w)
        assert in_place(rec.maps, w) and rec.maps[0][2] == 40 and same(got, want) and torch.equal(big, keep), dtype
        # a grad_out of another dtype is cast once
        g64, = torch.autograd.grad(torch_ops.ssim_map(xs, y), xs, grad_outputs=w.double())
        assert same(g64, want), dtype
        # a non-default stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            xq = x.clone().requires_grad_(True)
            on_side, = torch.autograd.grad(torch_ops.ssim_map(xq, y), xq, grad_outputs=w)
        side.synchronize()
        assert same(on_side, want), dtype
        # requires_grad on y only: None for x, and y's gradient as it is with both
        xb, yb = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        (w * torch_ops.ssim_map(xb, yb)).sum().backward()
        xn, yo = x.clone(), y.clone().requires_grad_(True)
        (w * torch_ops.ssim_map(xn, yo)).sum().backward()
        assert xn.grad is None and same(yo.grad, yb.grad) and same(xb.grad, want), dtype
        gx, gy = torch.autograd.grad(torch_ops.ssim_map(xb, yb), (xb, yb), grad_outputs=w)
        assert same(gx, want) and same(gy, yb.grad)


def memory_is_the_gradient_tensor_and_nothing_else(ctx):
    """Over a backward of (4, 3, 256, 256) planes, gradient for x only, torch's allocator rises by the gradient tensor (4 or 2 B/px) and
    4 KiB at most (it rounds a block to 512 B): no copy of grad_out (dense float32, or the expanded scalar of sum()), no float32
    intermediate of a bfloat16 gradient.  A float64 grad_out is cast once: one float32 plane set more."""
    shape = (4, 3, 256, 256)
    for dtype in (torch.float32, torch.bfloat16):
        x, y, w = tensors(dtype, shape, seed=7)
        x.requires_grad_(True)
        one = torch.ones((), device="cuda").expand(shape)
        w64 = w.double()
        for g in (w, one):                                   # contexts, streams and the allocator's pools exist before measuring
            torch.autograd.grad(torch_ops.ssim_map(x, y), x, grad_outputs=g)
        torch.cuda.empty_cache()
        es = x.element_size()
        for what, g, extra in (("dense float32 grad_out", w, 0), ("expanded grad_out", one, 0), ("float64 grad_out", w64, 4 * x.numel())):
            m = torch_ops.ssim_map(x, y)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            gx, = torch.autograd.grad(m, x, grad_outputs=g)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            bound = es * x.numel() + extra + 4096
            print("backward memory, %s, %s: %d B above the forward's, bound %d B" % (dtype, what, peak, bound))
            assert gx.dtype == dtype and peak <= bound, (dtype, what, peak, bound)
            del m, gx


CHECKS = [map_and_backward_are_the_c_abi_bit_for_bit, mean_runs_on_the_grad_out_it_is_handed_and_agrees_with_ssim,
          grad_out_slice_stream_and_needs_input_grad, memory_is_the_gradient_tensor_and_nothing_else]


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
