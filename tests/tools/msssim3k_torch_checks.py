#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_msssim3k.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/msssim3k_torch_checks.py
"""
import json
import os
import sys
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ssim_amd                                     # noqa: E402
from ssim_amd import torch_ops                      # noqa: E402

SHAPE = (2, 2, 12, 40, 52)                           # (N, C, D, H, W): a 12-frame clip, depth 12, 6, 3, 2, 1 down Wang's scales


def pair(dtype=torch.float32, seed=3, shape=SHAPE):
    torch.manual_seed(seed)
    x = torch.rand(shape, device="cuda")
    y = (x + 0.1 * torch.randn(shape, device="cuda")).clamp(0, 1)
    return x.to(dtype), y.to(dtype)


def abi_of_tensors(ctx, x, y, r, g_out, window, scales=5, weights=None):
    """The C ABI's entries (window None: those without _win) on the tensors' own memory (contiguous (N, C, D, H, W), float32 or 16-bit):
    float32 values, and the gradients of x and of y in the tensors' dtype for dLoss/dMS_i = g_out."""
    torch.cuda.synchronize()
    n, (d, h, w) = x.shape[0] * x.shape[1], x.shape[-3:]
    half = x.dtype != torch.float32
    es = 2 if half else 4
    st = {torch.float16: "float16", torch.bfloat16: "bfloat16"}.get(x.dtype)
    P, make, G = (ssim_amd.Params3H, ssim_amd.make_params3h, ssim_amd.Grad3H) if half else (ssim_amd.Params3F, ssim_amd.make_params3f, ssim_amd.Grad3F)
    dense, vol = (1, w, w * h), d * h * w
    ps = (P * n)()
    for i in range(n):
        ps[i] = make(w, h, d, x.data_ptr() + es * i * vol, dense, y.data_ptr() + es * i * vol, dense)
    values = torch.empty(n, dtype=torch.float64, device=x.device)
    means = torch.empty((n, scales, 2), dtype=torch.float64, device=x.device)
    go = torch.full((n,), g_out, dtype=torch.float32, device=x.device)
    gx, gy = torch.empty_like(x), torch.empty_like(y)
    ga, gb = (G * n)(), (G * n)()
    for i in range(n):
        ga[i] = G(gx.data_ptr() + es * i * vol, *dense)
        gb[i] = G(gy.data_ptr() + es * i * vol, *dense)
    torch.cuda.synchronize()
    if half:
        ctx.enqueue_msssim3h(ps, n, r, st, values.data_ptr(), means.data_ptr(), scales, weights, window=window)
        ctx.enqueue_msssim3h_grad(ps, n, r, st, means.data_ptr(), go.data_ptr(), ga, gb, scales, weights, window=window)
    else:
        ctx.enqueue_msssim3f(ps, n, r, values.data_ptr(), means.data_ptr(), scales, weights, window=window)
        ctx.enqueue_msssim3f_grad(ps, n, r, means.data_ptr(), go.data_ptr(), ga, gb, scales, weights, window=window)
    ctx.synchronize()
    return values.to(torch.float32), gx, gy


def same_bits(a, b):
    """Tensors of one dtype with the same bit patterns."""
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def windowed_ms_ssim3d_is_the_c_abi_bit_for_bit(ctx):
    for kw, win in ((dict(win_size=7), ssim_amd.make_window(7)), (dict(win_size=3, window="uniform"), ssim_amd.make_window(3, kind="uniform")),
                    (dict(win_sigma=2.0), ssim_amd.make_window(11, 2.0))):
        x, y = pair()
        x, y = x.requires_grad_(True), y.requires_grad_(True)
        s = torch_ops.ms_ssim3d(x, y, **kw)
        assert s.shape == (2, 2) and s.dtype == torch.float32
        (s.sum() * -0.5).backward()
        vals, gx, gy = abi_of_tensors(ctx, x.detach(), y.detach(), 1.0, -0.5, win)
        assert same_bits(s.detach().reshape(-1), vals), kw
        assert same_bits(x.grad, gx) and same_bits(y.grad, gy), kw
        assert float(x.grad.abs().max()) > 0
        assert not torch.equal(s.detach(), torch_ops.ms_ssim3d(x.detach(), y.detach())), kw      # it is another window
        # positional, after weights
        s2 = torch_ops.ms_ssim3d(x.detach(), y.detach(), 1.0, 5, None, kw.get("win_size", 11), kw.get("win_sigma", 1.5), kw.get("window", "gaussian"))
        assert same_bits(s2, s.detach())
    x, y = pair()
    s3 = torch_ops.ms_ssim3d(x, y, scales=3, weights=(0.2, 0.3, 0.5), win_size=9)
    vals, _, _ = abi_of_tensors(ctx, x, y, 1.0, 1.0, ssim_amd.make_window(9), 3, (0.2, 0.3, 0.5))
    assert same_bits(s3.reshape(-1), vals)


def windowed_ms_ssim3d_amp_on_16_bit_tensors_is_the_c_abi_bit_for_bit(ctx):
    scale = float(SHAPE[-3] * SHAPE[-2] * SHAPE[-1])
    for dtype in (torch.bfloat16, torch.float16):
        x, y = pair(dtype)
        x, y = x.requires_grad_(True), y.requires_grad_(True)
        s = torch_ops.ms_ssim3d_amp(x, y, win_size=7)
        assert s.dtype == torch.float32
        (s.sum() * scale).backward()
        assert x.grad.dtype == dtype and y.grad.dtype == dtype
        vals, gx, gy = abi_of_tensors(ctx, x.detach(), y.detach(), 1.0, scale, ssim_amd.make_window(7))
        assert same_bits(s.detach().reshape(-1), vals), dtype
        assert same_bits(x.grad, gx) and same_bits(y.grad, gy), dtype
        assert float(x.grad.float().abs().max()) > 0
        # the value has the bits of ms_ssim3d on the widened tensors under the same window
        assert same_bits(s.detach(), torch_ops.ms_ssim3d(x.detach().float(), y.detach().float(), win_size=7))
        try:
            torch_ops.ms_ssim3d(x.detach(), y.detach(), win_size=7)            # ms_ssim3d itself stays float32-only
        except TypeError:
            pass
        else:
            raise AssertionError("no TypeError")


def loss_under_autocast_hands_out_a_bfloat16_gradient(ctx):
    torch.manual_seed(5)
    conv = torch.nn.Conv3d(2, 2, 3, padding=1).cuda()
    with torch.no_grad():                                    # near the identity: the output resembles the target, so MS-SSIM is not
        conv.weight.mul_(0.1)                                # on the flat side of its ReLU, where every gradient is 0
        for c in range(2):
            conv.weight[c, c, 1, 1, 1] += 1.0
    img = torch.rand(SHAPE, device="cuda")
    seen = []
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out = conv(img)
        assert out.dtype == torch.bfloat16
        out.register_hook(lambda g: seen.append(g.dtype))
        loss = torch_ops.MSSSIM3DLoss(win_size=3, window="uniform")(out, img.to(torch.bfloat16))
        assert loss.dtype == torch.float32
    loss.backward()
    assert seen == [torch.bfloat16], seen                    # `out` is handed a bfloat16 gradient
    g = conv.weight.grad
    assert g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert 0.0 < float(loss) < 2.0
    want = 1.0 - torch_ops.ms_ssim3d_amp(out.detach(), img.to(torch.bfloat16), win_size=3, window="uniform").mean()
    assert abs(float(loss) - float(want)) < 1e-6


def default_keywords_give_the_bits_of_todays_call(ctx):
    for dtype in (torch.float32, torch.bfloat16):
        fn = torch_ops.ms_ssim3d if dtype == torch.float32 else torch_ops.ms_ssim3d_amp
        x, y = pair(dtype, 9)
        x = x.requires_grad_(True)
        s = fn(x, y)
        (s.sum() * 1000.0).backward()
        vals, gx, _ = abi_of_tensors(ctx, x.detach(), y, 1.0, 1000.0, None)                  # the entries without _win
        assert same_bits(s.detach().reshape(-1), vals) and same_bits(x.grad, gx)
        x2 = x.detach().clone().requires_grad_(True)
        s2 = fn(x2, y, win_size=11, win_sigma=1.5, window="gaussian")
        (s2.sum() * 1000.0).backward()
        assert same_bits(s2.detach(), s.detach()) and same_bits(x2.grad, x.grad)
        x3 = x.detach().clone().requires_grad_(True)
        loss = torch_ops.MSSSIM3DLoss(1.0, 5, None, "none")(x3, y)                                # an existing positional call
        (loss.sum() * -1000.0).backward()
        assert same_bits(loss.detach(), (1.0 - s).detach()) and same_bits(x3.grad, x.grad)


def non_contiguous_expanded_and_side_stream(ctx):
    d, h, w = SHAPE[-3:]
    scale = float(d * h * w)
    for dtype in (torch.float32, torch.bfloat16):
        fn = torch_ops.ms_ssim3d if dtype == torch.float32 else torch_ops.ms_ssim3d_amp
        kw = dict(win_size=5, win_sigma=0.8)
        torch.manual_seed(5)
        big_x = torch.rand(2, 5, d + 2, h + 6, w + 9, device="cuda").to(dtype)
        big_y = torch.rand(2, 3, d, h, w + 1, device="cuda").to(dtype)
        x, y = big_x[:, 1:5:2, 1:1 + d, 3:3 + h, 4:4 + w], big_y[:, 1:3, :, :, 1:]
        assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape == SHAPE
        xc, yc = x.contiguous().requires_grad_(True), y.contiguous()
        want = fn(xc, yc, **kw)
        (want.sum() * scale).backward()
        xs = x.detach().requires_grad_(True)
        assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride()
        before = (big_x.clone(), big_y.clone())
        got = fn(xs, y, **kw)
        (got.sum() * scale).backward()
        assert same_bits(got.detach(), want.detach()) and same_bits(xs.grad, xc.grad)
        assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])
        # an expanded target: one volume read by every batch element through a stride of 0
        one = yc[:1, :1]
        ye = one.expand(SHAPE)
        assert ye.stride()[0] == 0 and ye.stride()[1] == 0
        xe = xc.detach().clone().requires_grad_(True)
        got = fn(xe, ye, **kw)
        (got.sum() * scale).backward()
        xd = xc.detach().clone().requires_grad_(True)
        want_e = fn(xd, ye.contiguous(), **kw)
        (want_e.sum() * scale).backward()
        assert same_bits(got.detach(), want_e.detach()) and same_bits(xe.grad, xd.grad)
        # a side stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream().cuda_stream != 0
            xq = xc.detach().clone().requires_grad_(True)
            on_side = fn(xq, yc, **kw)
            (on_side.sum() * scale).backward()
        side.synchronize()
        assert same_bits(on_side.detach(), want.detach()) and same_bits(xq.grad, xc.grad)


CHECKS = [windowed_ms_ssim3d_is_the_c_abi_bit_for_bit, windowed_ms_ssim3d_amp_on_16_bit_tensors_is_the_c_abi_bit_for_bit,
          loss_under_autocast_hands_out_a_bfloat16_gradient, default_keywords_give_the_bits_of_todays_call,
          non_contiguous_expanded_and_side_stream]


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
