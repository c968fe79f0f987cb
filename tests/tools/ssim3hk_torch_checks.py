#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_ssim3hk.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

ssim3d_amp, ssim3d_map_amp and SSIM3DLoss with float16 / bfloat16 tensors under a non-default window: the value is
ssim3d(x.float(), y.float(), ...) exactly, the gradient has the inputs' dtype and is that call's float32 gradient rounded once.

usage (GPU box):  python tests/tools/ssim3hk_torch_checks.py
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
WINDOWS = (dict(win_size=7, window="uniform"), dict(win_size=5, win_sigma=0.8))


def u16(t):
    """The bit patterns of a float16 / bfloat16 tensor as a numpy uint16 array."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def rounded(t, g32, enc):
    """The 16-bit gradient t is the float32 gradient g32 rounded once."""
    return t.shape == g32.shape and HM.same(u16(t), HM.round_to(g32.detach().cpu().numpy(), enc), enc)


def volumes(shape, seed, dtype):
    """x, y of `shape` (..., D, H, W): random volumes in [0, 1] and a noisy copy, rounded to dtype."""
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(a).cuda().to(dtype), torch.from_numpy(b).cuda().to(dtype)


def value_and_gradient_are_the_float32_windowed_path_rounded_once():
    for dtype, enc in DTYPES:
        for kw in WINDOWS:
            x, y = volumes((2, 2, 9, 20, 33), 1, dtype)
            x, y = x.requires_grad_(True), y.requires_grad_(True)
            xf, yf = x.detach().float().requires_grad_(True), y.detach().float().requires_grad_(True)
            s, sf = torch_ops.ssim3d_amp(x, y, **kw), torch_ops.ssim3d(xf, yf, **kw)
            assert s.shape == (2, 2) and s.dtype == torch.float32 and torch.equal(s.detach(), sf.detach())
            assert not torch.equal(s.detach(), torch_ops.ssim3d_amp(x.detach(), y.detach()))      # the window is used
            scale = float(9 * 20 * 33)                                        # keeps the float16 gradient in the normal range
            loss, lf = torch_ops.SSIM3DLoss(**kw)(x, y), torch_ops.SSIM3DLoss(**kw)(xf, yf)
            assert loss.dtype == torch.float32 and torch.equal(loss.detach(), lf.detach())
            (loss * scale).backward()
            (lf * scale).backward()
            assert x.grad.dtype == dtype and y.grad.dtype == dtype and float(x.grad.float().abs().max()) > 0
            assert rounded(x.grad, xf.grad, enc) and rounded(y.grad, yf.grad, enc)
            # the map and its backward for a per-voxel upstream gradient
            torch.manual_seed(2)
            w = torch.randn(x.shape, device="cuda") * 100.0
            x3, y3 = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
            xf3, yf3 = x.detach().float().requires_grad_(True), y.detach().float().requires_grad_(True)
            m, mf = torch_ops.ssim3d_map_amp(x3, y3, **kw), torch_ops.ssim3d_map(xf3, yf3, **kw)
            assert m.shape == x.shape and m.dtype == torch.float32 and torch.equal(m.detach(), mf.detach())
            m.backward(w)
            mf.backward(w)
            assert x3.grad.dtype == dtype and rounded(x3.grad, xf3.grad, enc) and rounded(y3.grad, yf3.grad, enc)
            # reduction "none", and float32 tensors: exactly ssim3d
            none = torch_ops.SSIM3DLoss(reduction="none", **kw)(x.detach(), y.detach())
            assert none.shape == (2, 2) and torch.equal(none, 1.0 - sf.detach())
            assert torch.equal(torch_ops.ssim3d_amp(xf.detach(), yf.detach(), **kw), sf.detach())


def non_contiguous_expanded_and_y_only():
    for dtype, enc in DTYPES:
        for kw in WINDOWS:
            torch.manual_seed(3)
            big_x, big_y = torch.rand(3, 4, 14, 30, 41, device="cuda").to(dtype), torch.rand(40, 3, 12, 26, device="cuda").to(dtype)
            x = big_x[0:2, 1:4:2, 2:12, 3:27, 6:40:2]                      # (2, 2, 10, 24, 17): an odd element offset, step 2
            y = big_y[3:37:2, 0:2, 1:11, 2:26].permute(1, 2, 3, 0)[:, None].expand(2, 2, 10, 24, 17)      # W stored outermost; an expanded dimension
            assert not x.is_contiguous() and not y.is_contiguous() and y.stride(1) == 0 and x.data_ptr() % 4 == 2
            before = (big_x.clone(), big_y.clone())
            xs = x.detach().requires_grad_(True)
            assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride()
            xf = x.float().contiguous().requires_grad_(True)
            yf = y.float().contiguous()
            got, want = torch_ops.ssim3d_amp(xs, y, **kw), torch_ops.ssim3d(xf, yf, **kw)
            (got.sum() * 4080.0).backward()
            (want.sum() * 4080.0).backward()
            assert torch.equal(got.detach(), want.detach()) and xs.grad.dtype == dtype and rounded(xs.grad, xf.grad, enc)
            # y only: only what needs a gradient gets one, with the same bits
            yc = y.contiguous().requires_grad_(True)
            yg = yf.clone().requires_grad_(True)
            (torch_ops.SSIM3DLoss(**kw)(x, yc) * 4080.0).backward()
            (torch_ops.SSIM3DLoss(**kw)(xf.detach(), yg) * 4080.0).backward()
            assert yc.grad.dtype == dtype and rounded(yc.grad, yg.grad, enc) and float(yc.grad.float().abs().max()) > 0
            assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])


def side_stream():
    for dtype, enc in DTYPES:
        kw = WINDOWS[0]
        x, y = volumes((2, 1, 12, 18, 21), 4, dtype)
        torch.manual_seed(5)
        w = torch.randn(x.shape, device="cuda") * 100.0
        assert torch.cuda.current_stream().cuda_stream == 0                  # the legacy default stream
        xc = x.clone().requires_grad_(True)
        want_v = torch_ops.ssim3d_amp(xc, y, **kw)
        (want_v.sum() * 4536.0).backward()
        gv = xc.grad.clone()
        xc.grad = None
        want_m = torch_ops.ssim3d_map_amp(xc, y, **kw)
        (w * want_m).sum().backward()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream().cuda_stream != 0
            xq = x.clone().requires_grad_(True)
            on_side = torch_ops.ssim3d_amp(xq, y, **kw)
            (on_side.sum() * 4536.0).backward()
            gq = xq.grad.clone()
            xq.grad = None
            map_on_side = torch_ops.ssim3d_map_amp(xq, y, **kw)
            (w * map_on_side).sum().backward()
        side.synchronize()
        assert torch.equal(on_side, want_v) and HM.same(u16(gq), u16(gv), enc)
        assert torch.equal(map_on_side, want_m) and HM.same(u16(xq.grad), u16(xc.grad), enc) and float(gv.float().abs().max()) > 0


def sum_of_the_map_and_a_scaled_loss():
    """sum().backward() of the map hands the backward one expanded float (strides 0); a loss scaled by 65536 (what GradScaler does)
    arrives in grad_out, which stays float32, before the single rounding: round(65536 g), not 65536 round(g)."""
    for dtype, enc in DTYPES:
        for kw in WINDOWS:
            x, y = volumes((2, 1, 12, 18, 21), 7, dtype)
            seen = []
            xs, xf = x.clone().requires_grad_(True), x.float().requires_grad_(True)
            m = torch_ops.ssim3d_map_amp(xs, y, **kw)
            m.register_hook(lambda g: seen.append(g))
            (m.sum() * 0.5).backward()
            assert len(seen) == 1 and seen[0].dtype == torch.float32
            print("sum: grad_out arrives with strides %r" % (tuple(seen[0].stride()),))
            (torch_ops.ssim3d_map(xf, y.float(), **kw).sum() * 0.5).backward()
            assert rounded(xs.grad, xf.grad, enc) and float(xs.grad.float().abs().max()) > 0
            x2, xf2 = x.clone().requires_grad_(True), x.float().requires_grad_(True)
            (torch_ops.SSIM3DLoss(**kw)(x2, y) * 65536.0).backward()
            (torch_ops.SSIM3DLoss(**kw)(xf2, y.float()) * 65536.0).backward()
            assert rounded(x2.grad, xf2.grad, enc)                               # round(65536 g)
            xu = x.clone().requires_grad_(True)
            torch_ops.SSIM3DLoss(**kw)(xu, y).backward()
            differ = int((u16((xu.grad.float() * 65536.0).to(dtype)) != u16(x2.grad)).sum())
            print("scaled loss, %s, %r: %d of %d voxels differ from 65536 * round(g)" % (enc, kw, differ, x.numel()))
            if enc == HM.F16:                                # bfloat16 has float32's exponent range: a power of two commutes with its rounding
                assert differ > 0


def default_keywords_are_the_call_without_keywords():
    for dtype, enc in DTYPES:
        x, y = volumes((1, 2, 9, 20, 33), 8, dtype)
        x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        a = torch_ops.ssim3d_amp(x1, y)
        b = torch_ops.ssim3d_amp(x2, y, win_size=11, win_sigma=1.5, window="gaussian")
        assert torch.equal(a.detach(), b.detach()) and a.grad_fn is not None
        (a.sum() * 5940.0).backward()
        (b.sum() * 5940.0).backward()
        assert HM.same(u16(x1.grad), u16(x2.grad), enc) and float(x1.grad.float().abs().max()) > 0
        assert torch.equal(torch_ops.ssim3d_map_amp(x, y), torch_ops.ssim3d_map_amp(x, y, win_size=11, win_sigma=1.5, window="gaussian"))
        assert torch.equal(torch_ops.SSIM3DLoss()(x, y), torch_ops.SSIM3DLoss(1.0, "mean", 11, 1.5, "gaussian")(x, y))


def ssim3d_still_refuses_16_bit_tensors():
    x, y = volumes((1, 1, 6, 8, 9), 9, torch.float16)
    for fn in (torch_ops.ssim3d, torch_ops.ssim3d_map):
        for t in (x, x.bfloat16()):
            for kw in (dict(win_size=7), dict()):
                try:
                    fn(t, t, **kw)
                except TypeError as e:
                    assert "float32 for now" in str(e), str(e)
                else:
                    raise AssertionError("no TypeError")
    for fn in (torch_ops.ssim, torch_ops.ssim_map):                           # the 2-D names keep the fixed window with 16-bit tensors
        try:
            fn(x, y, win_size=7)
        except TypeError as e:
            assert "fixed window" in str(e), str(e)
        else:
            raise AssertionError("no TypeError")
    for fn in (torch_ops.ssim3d_amp, torch_ops.ssim3d_map_amp, torch_ops.SSIM3DLoss(win_size=7)):
        try:
            fn(x, y.float()) if not isinstance(fn, torch_ops.SSIM3DLoss) else fn(x, y.bfloat16())
        except TypeError:
            continue
        raise AssertionError("no TypeError for a mixed pair")


CHECKS = [value_and_gradient_are_the_float32_windowed_path_rounded_once, non_contiguous_expanded_and_y_only, side_stream,
          sum_of_the_map_and_a_scaled_loss, default_keywords_are_the_call_without_keywords, ssim3d_still_refuses_16_bit_tensors]


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
