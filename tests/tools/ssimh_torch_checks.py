#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_ssimh.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/ssimh_torch_checks.py
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

import halfmodel as HM                              # noqa: E402
import ssim_amd                                     # noqa: E402
from conftest import GOLDEN, image_entries, load_pair   # noqa: E402
from ssim_amd import torch_ops                      # noqa: E402

DTYPES = ((torch.float16, HM.F16), (torch.bfloat16, HM.BF16))


def u16(t):
    """The bit patterns of a float16 / bfloat16 tensor as a numpy uint16 array."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def same(t, want, enc):
    return HM.same(u16(t), u16(want) if isinstance(want, torch.Tensor) else want, enc)


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def torch_pair(man, dtype):
    """(2, 3, H, W) tensors from six of the einstein pairs, rounded to dtype."""
    pool = []
    for n in image_entries(man):
        if n.startswith("einstein_") and n != "einstein_einstein":
            a, b = load_pair(man[n])
            pool.append((a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)))
    a = np.stack([np.stack([pool[(3 * i + c) % len(pool)][0] for c in range(3)]) for i in range(2)])
    b = np.stack([np.stack([pool[(3 * i + c) % len(pool)][1] for c in range(3)]) for i in range(2)])
    return torch.from_numpy(a).cuda().to(dtype), torch.from_numpy(b).cuda().to(dtype)


def abi_of_tensors(ctx, x, y, enc, r, g_out):
    """The C ABI on the tensors' own memory (contiguous (N, C, H, W), 16-bit): values and the gradient of x for dLoss/dS_i = g_out."""
    torch.cuda.synchronize()
    n, (h, w) = x.shape[0] * x.shape[1], x.shape[-2:]
    ps = (ssim_amd.Params16 * n)()
    for i in range(n):
        ps[i] = ssim_amd.make_params16(w, h, x.data_ptr() + 2 * i * h * w, 1, w, y.data_ptr() + 2 * i * h * w, 1, w)
    vals = ctx.ssimh_device(ps, n, r, enc)
    go = torch.full((n,), g_out, dtype=torch.float32, device=x.device)
    gx = torch.empty_like(x)
    ga = (ssim_amd.GradH * n)()
    for i in range(n):
        ga[i] = ssim_amd.GradH(gx.data_ptr() + 2 * i * h * w, 1, w)
    torch.cuda.synchronize()
    ctx.enqueue_ssimh_grad(ps, n, r, enc, go.data_ptr(), ga, None)
    ctx.synchronize()
    return vals, gx


def forward_and_backward_are_the_c_abi_bit_for_bit(man, ctx):
    for dtype, enc in DTYPES:
        x, y = torch_pair(man, dtype)
        x = x.clone().requires_grad_(True)
        s = torch_ops.ssim(x, y)
        assert s.shape == (2, 3) and s.dtype == torch.float32                # float32 at every input dtype
        h, w = x.shape[-2:]
        scale = float(h * w)                                                  # keeps the float16 gradient in the normal range
        loss = torch_ops.SSIMLoss()(x, y)
        assert loss.dtype == torch.float32
        (loss * scale).backward()
        assert x.grad.dtype == dtype and x.grad.shape == x.shape              # the gradient has the input's dtype
        g_out = float(np.float32(-scale) / np.float32(6.0))              # what autograd hands the backward: scale / 6 planes, negated
        vals, gx = abi_of_tensors(ctx, x.detach(), y, enc, 1.0, g_out)
        assert np.array_equal(s.detach().cpu().numpy().reshape(-1).view(np.uint32), vals.view(np.uint32))
        assert same(x.grad, gx, enc) and float(x.grad.float().abs().max()) > 0
        # ... which is the float32 path on the widened tensors, rounded once
        xf = x.detach().float().requires_grad_(True)
        sf = torch_ops.ssim(xf, y.float())
        assert torch.equal(sf, s.detach())
        ((1.0 - sf).mean() * scale).backward()
        assert same(x.grad, HM.round_to(xf.grad.cpu().numpy(), enc), enc)
        # y alone, and both: only what needs a gradient gets one, with the same bits
        x2, y2 = x.detach().clone().requires_grad_(True), y.clone().requires_grad_(True)
        (torch_ops.SSIMLoss()(x2, y2) * scale).backward()
        assert same(x2.grad, gx, enc) and y2.grad.dtype == dtype
        y3 = y.clone().requires_grad_(True)
        (torch_ops.SSIMLoss()(x.detach(), y3) * scale).backward()
        assert same(y3.grad, y2.grad, enc)
        none = torch_ops.SSIMLoss(reduction="none")(x.detach(), y)
        assert none.shape == (2, 3) and not none.requires_grad and none.dtype == torch.float32
        for bad, exc in ((lambda: torch_ops.ssim(x.detach(), y.float()), TypeError), (lambda: torch_ops.ssim(x.detach(), y[:, :, :-1]), ValueError),
                         (lambda: torch_ops.ssim(x.detach(), y.cpu()), ValueError), (lambda: torch_ops.ms_ssim(x.detach(), y), TypeError)):
            try:
                bad()
            except exc:
                continue
            raise AssertionError("no %s" % exc.__name__)


def _slices(dtype):
    torch.manual_seed(3)
    big_x, big_y = torch.rand(4, 8, 40, 51, device="cuda").to(dtype), torch.rand(4, 8, 44, 51, device="cuda").to(dtype)
    x, y = big_x[1:3, 2:8:2, 3:35, 5:45:2], big_y[0:2, 1:4, 7:39, 6:26]
    assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape == (2, 3, 32, 20)
    assert x.data_ptr() % 4 == 2 or y.data_ptr() % 4 == 2              # an odd element offset: 2-byte but not 4-byte aligned
    return big_x, big_y, x, y


def non_contiguous_slice_without_a_copy(man, ctx):
    for dtype, enc in DTYPES:
        big_x, big_y, x, y = _slices(dtype)
        xc, yc = x.contiguous().requires_grad_(True), y.contiguous()
        want = torch_ops.ssim(xc, yc)
        (want.sum() * 640.0).backward()
        xs = x.detach().requires_grad_(True)
        assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride()
        before = (big_x.clone(), big_y.clone())
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        got = torch_ops.ssim(xs, y)
        peak = torch.cuda.max_memory_allocated() - base
        assert peak < x.numel() * 2, peak                   # the sums and the result only: no contiguous copy of a plane was made
        (got.sum() * 640.0).backward()
        assert torch.equal(got, want) and same(xs.grad, xc.grad, enc) and xs.grad.dtype == dtype
        assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])


def non_default_and_legacy_default_stream(man, ctx):
    for dtype, enc in DTYPES:
        _, _, x, y = _slices(dtype)
        xc, yc = x.contiguous().requires_grad_(True), y.contiguous()
        assert torch.cuda.current_stream().cuda_stream == 0                # the legacy default stream
        want = torch_ops.ssim(xc, yc)
        (want.sum() * 640.0).backward()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream().cuda_stream != 0
            xq = xc.detach().clone().requires_grad_(True)
            on_side = torch_ops.ssim(xq, yc)
            (on_side.sum() * 640.0).backward()
        side.synchronize()
        assert torch.equal(on_side, want) and same(xq.grad, xc.grad, enc)
        # both are the float32 path on the widened planes
        xf = xc.detach().float().requires_grad_(True)
        wf = torch_ops.ssim(xf, yc.float())
        (wf.sum() * 640.0).backward()
        assert torch.equal(wf, want) and same(xc.grad, HM.round_to(xf.grad.cpu().numpy(), enc), enc)


def a_scaled_loss_is_rounded_once(man, ctx):
    """A loss scaled by 65536 (what GradScaler does) arrives in grad_out and is applied before the single rounding: round(65536 g), not
    65536 round(g) -- in float16 the unscaled gradient of a mean over 256 x 256 pixels is subnormal or zero."""
    for dtype, enc in DTYPES:
        x, y = torch_pair(man, dtype)
        x = x.clone().requires_grad_(True)
        (torch_ops.SSIMLoss()(x, y) * 65536.0).backward()
        xf = x.detach().float().requires_grad_(True)
        (torch_ops.SSIMLoss()(xf, y.float()) * 65536.0).backward()
        assert same(x.grad, HM.round_to(xf.grad.cpu().numpy(), enc), enc)                    # round(65536 g)
        xu = x.detach().clone().requires_grad_(True)
        torch_ops.SSIMLoss()(xu, y).backward()
        twice = (xu.grad.float() * 65536.0).to(dtype)                                        # 65536 round(g)
        differ = int((u16(twice) != u16(x.grad)).sum())
        print("scaled loss, %s: %d of %d pixels differ from 65536 * round(g)" % (enc, differ, x.numel()))
        if enc == HM.F16:                                    # bfloat16 has float32's exponent range: a power of two commutes with its rounding
            tiny = int(HM.is_subnormal(u16(xu.grad), enc).sum() + ((u16(xu.grad) & 0x7FFF) == 0).sum())
            print("scaled loss, float16: %d of %d unscaled gradient pixels are subnormal or zero" % (tiny, x.numel()))
            assert differ > 0 and tiny > 0                   # the unscaled float16 gradient has lost bits the scaled one keeps


def autocast_conv_feeds_the_loss(man, ctx):
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(3, 3, 3, padding=1).cuda()
    img, target = torch.rand(2, 3, 48, 72, device="cuda"), torch.rand(2, 3, 48, 72, device="cuda")
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out = conv(img)
        assert out.dtype == torch.bfloat16
        loss = torch_ops.SSIMLoss()(out, target.to(torch.bfloat16))          # taken as it comes: not itself autocast
        assert loss.dtype == torch.float32
        try:
            torch_ops.ssim(out, target)                                      # a mixed pair stays a TypeError inside autocast
        except TypeError:
            pass
        else:
            raise AssertionError("no TypeError")
    loss.backward()
    g = conv.weight.grad
    assert g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert 0.0 < float(loss) < 2.0


def _step_memory(step, x, y):
    """Peak of torch's allocator over one forward + backward above what is allocated before it; x.grad is dropped first."""
    x.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(x, y)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def memory_is_the_gradient_tensor_and_nothing_else(man, ctx):
    """(4, 3, 512, 512) bfloat16, gradient for x only: forward + backward rise above the inputs by at most the gradient tensor (2 B/px)
    plus 1 MiB (the per-plane sums, grad_out, allocator rounding).  The route through ssim(x.float(), y.float()) -- two float32 copies,
    a float32 gradient and its cast back -- is measured beside it and must exceed that bound."""
    torch.manual_seed(7)
    x = torch.rand(4, 3, 512, 512, device="cuda").to(torch.bfloat16).requires_grad_(True)
    y = torch.rand(4, 3, 512, 512, device="cuda").to(torch.bfloat16)

    def native(x, y):
        torch_ops.SSIMLoss()(x, y).backward()

    def widened(x, y):
        torch_ops.SSIMLoss()(x.float(), y.float()).backward()
    native(x, y)                                             # contexts, streams and the allocator's pools exist before measuring
    widened(x, y)
    torch.cuda.empty_cache()
    bound = 2 * x.numel() + (1 << 20)
    got, other = _step_memory(native, x, y), _step_memory(widened, x, y)
    print("training step memory above the inputs: native %d B, through float32 %d B, bound %d B" % (got, other, bound))
    assert x.grad.dtype == torch.bfloat16
    assert got <= bound, (got, bound)
    assert other > bound, (other, bound)


CHECKS = [forward_and_backward_are_the_c_abi_bit_for_bit, non_contiguous_slice_without_a_copy, non_default_and_legacy_default_stream,
          a_scaled_loss_is_rounded_once, autocast_conv_feeds_the_loss, memory_is_the_gradient_tensor_and_nothing_else]


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
