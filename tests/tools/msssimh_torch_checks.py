#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_msssimh.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/msssimh_torch_checks.py
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
from ssim_amd import torch_ops                      # noqa: E402

DTYPES = ((torch.bfloat16, HM.BF16), (torch.float16, HM.F16))
SHAPE = (2, 3, 70, 150)


def u16(t):
    """The bit patterns of a float16 / bfloat16 tensor as a numpy uint16 array."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def same(t, want, enc):
    return HM.same(u16(t), u16(want), enc)


def pair(dtype, seed=3, shape=SHAPE):
    torch.manual_seed(seed)
    x = torch.rand(shape, device="cuda")
    y = (x + 0.1 * torch.randn(shape, device="cuda")).clamp(0, 1)
    return x.to(dtype), y.to(dtype)


def forward_and_backward_are_the_float32_path_bit_for_bit():
    h, w = SHAPE[-2:]
    scale = float(h * w)                                                      # keeps the float16 gradient in the normal range
    for dtype, enc in DTYPES:
        for kw in ({}, {"scales": 1, "weights": (1.0,)}, {"scales": 3, "weights": (0.0, 0.5, 0.5)}):
            x, y = pair(dtype)
            x, y = x.requires_grad_(True), y.requires_grad_(True)
            s = torch_ops.ms_ssim_amp(x, y, **kw)
            assert s.shape == (2, 3) and s.dtype == torch.float32            # float32 at every input dtype
            (s.sum() * scale).backward()
            assert x.grad.dtype == dtype and y.grad.dtype == dtype and x.grad.shape == x.shape      # the gradients have the inputs' dtype
            xf, yf = x.detach().float().requires_grad_(True), y.detach().float().requires_grad_(True)
            sf = torch_ops.ms_ssim(xf, yf, **kw)
            (sf.sum() * scale).backward()
            assert torch.equal(s.detach(), sf.detach()), (dtype, kw)
            assert same(x.grad, xf.grad.to(dtype), enc) and same(y.grad, yf.grad.to(dtype), enc), (dtype, kw)
            assert float(x.grad.float().abs().max()) > 0
            # x alone: only what needs a gradient gets one, with the same bits
            x2 = x.detach().clone().requires_grad_(True)
            (torch_ops.ms_ssim_amp(x2, y.detach(), **kw).sum() * scale).backward()
            assert same(x2.grad, x.grad, enc)
        loss = torch_ops.MSSSIMLoss()(x.detach(), y.detach())
        assert loss.dtype == torch.float32 and loss.dim() == 0
        none = torch_ops.MSSSIMLoss(reduction="none")(x.detach(), y.detach())
        assert none.shape == (2, 3) and none.dtype == torch.float32 and not none.requires_grad
        # float32 tensors: ms_ssim_amp is ms_ssim
        assert torch.equal(torch_ops.ms_ssim_amp(xf.detach(), yf.detach()), torch_ops.ms_ssim(xf.detach(), yf.detach()))
        for bad, exc in ((lambda: torch_ops.ms_ssim_amp(x.detach(), y.detach().float()), TypeError),
                         (lambda: torch_ops.ms_ssim_amp(x.detach(), y.detach()[:, :, :-1]), ValueError),
                         (lambda: torch_ops.ms_ssim_amp(x.detach(), y.detach().cpu()), ValueError),
                         (lambda: torch_ops.ms_ssim_amp(x.detach().cpu(), y.detach().cpu()), TypeError),
                         (lambda: torch_ops.ms_ssim(x.detach(), y.detach()), TypeError)):      # ms_ssim itself stays float32-only
            try:
                bad()
            except exc:
                continue
            raise AssertionError("no %s" % exc.__name__)


def non_contiguous_channel_slice_without_a_copy():
    h, w = SHAPE[-2:]
    for dtype, enc in DTYPES:
        torch.manual_seed(5)
        big_x = torch.rand(2, 7, h + 6, w + 9, device="cuda").to(dtype)
        big_y = torch.rand(2, 5, h, w + 1, device="cuda").to(dtype)
        x, y = big_x[:, 1:7:2, 3:3 + h, 4:4 + w], big_y[:, 1:4, :, 1:]
        assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape == SHAPE
        assert y.data_ptr() % 4 == 2                        # an odd element offset: 2-byte but not 4-byte aligned
        xc, yc = x.contiguous().requires_grad_(True), y.contiguous()
        want = torch_ops.ms_ssim_amp(xc, yc)
        (want.sum() * float(h * w)).backward()
        xs = x.detach().requires_grad_(True)
        assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride()
        before = (big_x.clone(), big_y.clone())
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        got = torch_ops.ms_ssim_amp(xs, y)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert peak < x.numel() * 2, peak                   # the values and the means only: no contiguous copy of a plane was made
        (got.sum() * float(h * w)).backward()
        assert torch.equal(got, want) and same(xs.grad, xc.grad, enc) and xs.grad.dtype == dtype
        assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])


def non_default_stream():
    h, w = SHAPE[-2:]
    for dtype, enc in DTYPES:
        x, y = pair(dtype, 11)
        x = x.requires_grad_(True)
        assert torch.cuda.current_stream().cuda_stream == 0                # the legacy default stream
        want = torch_ops.ms_ssim_amp(x, y)
        (want.sum() * float(h * w)).backward()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream().cuda_stream != 0
            xq = x.detach().clone().requires_grad_(True)
            on_side = torch_ops.ms_ssim_amp(xq, y)
            (on_side.sum() * float(h * w)).backward()
        side.synchronize()
        assert torch.equal(on_side, want) and same(xq.grad, x.grad, enc)


def autocast_conv_feeds_the_loss():
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(3, 3, 3, padding=1).cuda()
    with torch.no_grad():                                    # near the identity: the output resembles the target, so MS-SSIM is not
        conv.weight.mul_(0.1)                                # on the flat side of its ReLU, where every gradient is 0
        for c in range(3):
            conv.weight[c, c, 1, 1] += 1.0
    img = torch.rand(SHAPE, device="cuda")
    target = img
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out = conv(img)
        assert out.dtype == torch.bfloat16
        loss = torch_ops.MSSSIMLoss()(out, target.to(torch.bfloat16))        # taken as it comes: not itself autocast
        assert loss.dtype == torch.float32
        try:
            torch_ops.ms_ssim_amp(out, target)                                 # a mixed pair stays a TypeError inside autocast
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


def training_step_memory_is_the_16_bit_gradient():
    """(4, 3, 256, 256) bfloat16, gradient for x only: forward + backward rise above the inputs by less than 3 bytes per element of x.  The
    2 B/px gradient fits under that; a float32 copy or a float32 gradient does not, and the route through ms_ssim(x.float(), y.float())
    is measured beside it."""
    x, y = pair(torch.bfloat16, 7, (4, 3, 256, 256))
    x = x.requires_grad_(True)

    def native(x, y):
        torch_ops.MSSSIMLoss()(x, y).backward()

    def widened(x, y):
        torch_ops.MSSSIMLoss()(x.float(), y.float()).backward()
    native(x, y)                                             # contexts, streams and the allocator's pools exist before measuring
    widened(x, y)
    torch.cuda.empty_cache()
    bound = 3 * x.numel()
    got, other = _step_memory(native, x, y), _step_memory(widened, x, y)
    print("training step memory above the inputs: native %d B, through float32 %d B, bound %d B" % (got, other, bound))
    assert x.grad.dtype == torch.bfloat16
    assert got < bound, (got, bound)
    assert other >= bound, (other, bound)


CHECKS = [forward_and_backward_are_the_float32_path_bit_for_bit, non_contiguous_channel_slice_without_a_copy, non_default_stream,
          autocast_conv_feeds_the_loss, training_step_memory_is_the_16_bit_gradient]


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
