#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_ssimhk.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

ssim_amp, ssim_map_amp and SSIMLoss with float16 / bfloat16 tensors under a non-default window: value and gradient are the bits of the
rmgr_ssim_hip_*_ssimh_win* entries called on the same memory, the value is ssim(x.float(), y.float(), ...) exactly, and the gradient has
the inputs' dtype and is that call's float32 gradient rounded once.

usage (GPU box):  python tests/tools/ssimhk_torch_checks.py
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
from ssim_amd import torch_ops                      # noqa: E402

DTYPES = ((torch.bfloat16, HM.BF16), (torch.float16, HM.F16))
WINDOWS = (dict(win_size=7, window="uniform"), dict(win_size=5, win_sigma=0.8), dict(win_size=3, window="uniform"), dict(win_sigma=2.0))


def u16(t):
    """The bit patterns of a float16 / bfloat16 tensor as a numpy uint16 array."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def rounded(t, g32, enc):
    """The 16-bit gradient t is the float32 gradient g32 rounded once."""
    return t.shape == g32.shape and HM.same(u16(t), HM.round_to(g32.detach().cpu().numpy(), enc), enc)


def planes(shape, seed, dtype):
    """x, y of `shape` (..., H, W): random planes in [0, 1] and a noisy copy, rounded to dtype."""
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(a).cuda().to(dtype), torch.from_numpy(b).cuda().to(dtype)


def window_of(kw):
    kind = kw.get("window", "gaussian")
    return ssim_amd.make_window(kw.get("win_size", 11), 1.5 if kind == "uniform" else kw.get("win_sigma", 1.5), kind)


def c_abi(x, y, enc, kw, g_out):
    """(values, dA, dB) of the contiguous (N, C, H, W) tensors x, y through rmgr_ssim_hip_enqueue_ssimh_win / _ssimh_win_grad on a context
    of its own: float32 values, uint16 bit patterns."""
    n, (h, w) = x.shape[0] * x.shape[1], x.shape[-2:]
    sums = torch.empty(n, dtype=torch.float64, device="cuda")
    go = torch.full((n,), g_out, dtype=torch.float32, device="cuda")
    ga, gb = torch.empty_like(x), torch.empty_like(y)
    torch.cuda.synchronize()
    with ssim_amd.Context(0) as ctx:
        ps, pa, pb = (ssim_amd.Params16 * n)(), (ssim_amd.GradH * n)(), (ssim_amd.GradH * n)()
        for i in range(n):
            off = 2 * i * h * w
            ps[i] = ssim_amd.make_params16(w, h, x.data_ptr() + off, 1, w, y.data_ptr() + off, 1, w)
            pa[i], pb[i] = ssim_amd.GradH(ga.data_ptr() + off, 1, w), ssim_amd.GradH(gb.data_ptr() + off, 1, w)
        ctx.enqueue_ssimh(ps, n, 1.0, enc, sums.data_ptr(), window=window_of(kw))
        ctx.enqueue_ssimh_grad(ps, n, 1.0, enc, go.data_ptr(), pa, pb, window=window_of(kw))
        ctx.synchronize()
    return (sums / (float(w) * float(h))).to(torch.float32).reshape(x.shape[:2]), u16(ga), u16(gb)


def value_and_gradient_are_the_c_abi_bit_for_bit():
    for dtype, enc in DTYPES:
        for kw in WINDOWS:
            x, y = planes((2, 2, 33, 129), 1, dtype)
            scale = float(33 * 129)                                           # keeps the float16 gradient in the normal range
            cv, ca, cb = c_abi(x, y, enc, kw, -scale)                         # the loss is 1 - ssim, reduction "none" summed: dLoss/dS = -scale
            x, y = x.requires_grad_(True), y.requires_grad_(True)
            xf, yf = x.detach().float().requires_grad_(True), y.detach().float().requires_grad_(True)
            s, sf = torch_ops.ssim_amp(x, y, **kw), torch_ops.ssim(xf, yf, **kw)
            assert s.shape == (2, 2) and s.dtype == torch.float32 and torch.equal(s.detach(), sf.detach()) and torch.equal(s.detach(), cv)
            assert not torch.equal(s.detach(), torch_ops.ssim_amp(x.detach(), y.detach()))      # the window is used
            loss, lf = torch_ops.SSIMLoss(reduction="none", **kw)(x, y), torch_ops.SSIMLoss(reduction="none", **kw)(xf, yf)
            assert loss.dtype == torch.float32 and torch.equal(loss.detach(), lf.detach()) and torch.equal(loss.detach(), 1.0 - cv)
            (loss.sum() * scale).backward()
            (lf.sum() * scale).backward()
            assert x.grad.dtype == dtype and y.grad.dtype == dtype and float(x.grad.float().abs().max()) > 0
            assert rounded(x.grad, xf.grad, enc) and rounded(y.grad, yf.grad, enc)
            assert HM.same(u16(x.grad), ca, enc) and HM.same(u16(y.grad), cb, enc)
            mean = torch_ops.SSIMLoss(**kw)(x.detach(), y.detach())
            assert mean.shape == () and torch.equal(mean, (1.0 - sf.detach()).mean())
            # the map and its backward for a per-pixel upstream gradient
            torch.manual_seed(2)
            w = torch.randn(x.shape, device="cuda") * 100.0
            x3, y3 = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
            xf3, yf3 = x.detach().float().requires_grad_(True), y.detach().float().requires_grad_(True)
            m, mf = torch_ops.ssim_map_amp(x3, y3, **kw), torch_ops.ssim_map(xf3, yf3, **kw)
            assert m.shape == x.shape and m.dtype == torch.float32 and torch.equal(m.detach(), mf.detach())
            m.backward(w)
            mf.backward(w)
            assert x3.grad.dtype == dtype and rounded(x3.grad, xf3.grad, enc) and rounded(y3.grad, yf3.grad, enc)
            # float32 tensors: exactly ssim
            assert torch.equal(torch_ops.ssim_amp(xf.detach(), yf.detach(), **kw), sf.detach())
            assert torch.equal(torch_ops.ssim_map_amp(xf.detach(), yf.detach(), **kw), mf.detach())


def non_contiguous_expanded_and_y_only():
    for dtype, enc in DTYPES:
        for kw in WINDOWS[:2]:
            torch.manual_seed(3)
            big_x, big_y = torch.rand(3, 4, 30, 41, device="cuda").to(dtype), torch.rand(40, 3, 26, device="cuda").to(dtype)
            x = big_x[0:2, 1:4:2, 3:27, 6:40:2]                            # (2, 2, 24, 17): an odd element offset, step 2
            y = big_y[3:37:2, 0:2, 2:26].permute(1, 2, 0)[:, None].expand(2, 2, 24, 17)      # W stored outermost; an expanded dimension
            assert not x.is_contiguous() and not y.is_contiguous() and y.stride(1) == 0 and x.data_ptr() % 4 == 2
            before = (big_x.clone(), big_y.clone())
            xs = x.detach().requires_grad_(True)
            assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride()
            xf = x.float().contiguous().requires_grad_(True)
            yf = y.float().contiguous()
            got, want = torch_ops.ssim_amp(xs, y, **kw), torch_ops.ssim(xf, yf, **kw)
            (got.sum() * 408.0).backward()
            (want.sum() * 408.0).backward()
            assert torch.equal(got.detach(), want.detach()) and xs.grad.dtype == dtype and rounded(xs.grad, xf.grad, enc)
            # an expanded upstream gradient of the map: read in place, one float behind strides 0
            seen = []
            xm, xmf = x.detach().clone().requires_grad_(True), x.float().contiguous().requires_grad_(True)
            m = torch_ops.ssim_map_amp(xm, y, **kw)
            m.register_hook(lambda g: seen.append(g))
            (m.sum() * 0.5).backward()
            (torch_ops.ssim_map(xmf, yf, **kw).sum() * 0.5).backward()
            assert len(seen) == 1 and seen[0].dtype == torch.float32 and rounded(xm.grad, xmf.grad, enc)
            print("sum: grad_out arrives with strides %r" % (tuple(seen[0].stride()),))
            # y only: only what needs a gradient gets one, with the same bits
            yc = y.contiguous().requires_grad_(True)
            yg = yf.clone().requires_grad_(True)
            (torch_ops.SSIMLoss(**kw)(x, yc) * 408.0).backward()
            (torch_ops.SSIMLoss(**kw)(xf.detach(), yg) * 408.0).backward()
            assert yc.grad.dtype == dtype and rounded(yc.grad, yg.grad, enc) and float(yc.grad.float().abs().max()) > 0
            assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])


def a_scaled_loss_is_rounded_once():
    """A loss scaled by torch.amp.GradScaler (65536) arrives in grad_out, which stays float32, before the single rounding:
    round(65536 g), not 65536 round(g)."""
    for dtype, enc in DTYPES:
        for kw in WINDOWS[:2]:
            x, y = planes((2, 1, 18, 21), 7, dtype)
            scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
            x2, xf2 = x.clone().requires_grad_(True), x.float().requires_grad_(True)
            scaler.scale(torch_ops.SSIMLoss(**kw)(x2, y)).backward()
            (torch_ops.SSIMLoss(**kw)(xf2, y.float()) * 65536.0).backward()
            assert rounded(x2.grad, xf2.grad, enc) and float(x2.grad.float().abs().max()) > 0     # round(65536 g)
            xu = x.clone().requires_grad_(True)
            torch_ops.SSIMLoss(**kw)(xu, y).backward()
            differ = int((u16((xu.grad.float() * 65536.0).to(dtype)) != u16(x2.grad)).sum())
            print("scaled loss, %s, %r: %d of %d pixels differ from 65536 * round(g)" % (enc, kw, differ, x.numel()))
            if enc == HM.F16:                                # bfloat16 has float32's exponent range: a power of two commutes with its rounding
                assert differ > 0


def side_stream():
    for dtype, enc in DTYPES:
        kw = WINDOWS[0]
        x, y = planes((2, 1, 18, 21), 4, dtype)
        torch.manual_seed(5)
        w = torch.randn(x.shape, device="cuda") * 100.0
        assert torch.cuda.current_stream().cuda_stream == 0                  # the legacy default stream
        xc = x.clone().requires_grad_(True)
        want_v = torch_ops.ssim_amp(xc, y, **kw)
        (want_v.sum() * 378.0).backward()
        gv = xc.grad.clone()
        xc.grad = None
        want_m = torch_ops.ssim_map_amp(xc, y, **kw)
        (w * want_m).sum().backward()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream().cuda_stream != 0
            xq = x.clone().requires_grad_(True)
            on_side = torch_ops.ssim_amp(xq, y, **kw)
            (on_side.sum() * 378.0).backward()
            gq = xq.grad.clone()
            xq.grad = None
            map_on_side = torch_ops.ssim_map_amp(xq, y, **kw)
            (w * map_on_side).sum().backward()
        side.synchronize()
        assert torch.equal(on_side, want_v) and HM.same(u16(gq), u16(gv), enc)
        assert torch.equal(map_on_side, want_m) and HM.same(u16(xq.grad), u16(xc.grad), enc) and float(gv.float().abs().max()) > 0


def default_keywords_are_ssim_bit_for_bit():
    for dtype, enc in DTYPES + ((torch.float32, None),):
        x, y = planes((1, 2, 20, 33), 8, dtype)
        x1, x2, x3 = (x.clone().requires_grad_(True) for _ in range(3))
        a = torch_ops.ssim(x1, y)
        b = torch_ops.ssim_amp(x2, y)
        c = torch_ops.ssim_amp(x3, y, win_size=11, win_sigma=1.5, window="gaussian")
        assert torch.equal(a.detach(), b.detach()) and torch.equal(a.detach(), c.detach()) and b.grad_fn is not None
        for t in (a, b, c):
            (t.sum() * 660.0).backward()
        assert torch.equal(x1.grad, x2.grad) and torch.equal(x1.grad, x3.grad) and x2.grad.dtype == dtype and float(x1.grad.float().abs().max()) > 0
        assert torch.equal(torch_ops.ssim_map(x, y), torch_ops.ssim_map_amp(x, y))
        assert torch.equal(torch_ops.ssim_map(x, y), torch_ops.ssim_map_amp(x, y, win_size=11, win_sigma=1.5, window="gaussian"))
        assert torch.equal(torch_ops.SSIMLoss()(x, y), (1.0 - a.detach()).mean())


def ssim_and_ssim_map_still_refuse_with_fixed_window():
    x, y = planes((1, 1, 8, 9), 9, torch.float16)
    for fn in (torch_ops.ssim, torch_ops.ssim_map):
        for t in (x, x.bfloat16()):
            for kw in (dict(win_size=7), dict(win_sigma=2.0), dict(win_size=3, window="uniform")):
                try:
                    fn(t, t, **kw)
                except TypeError as e:
                    assert "fixed window" in str(e), str(e)
                else:
                    raise AssertionError("no TypeError")
            assert fn(t, t).dtype == torch.float32                            # the fixed window still works
    for fn in (torch_ops.ssim_amp, torch_ops.ssim_map_amp, torch_ops.SSIMLoss(win_size=7)):
        for pair in ((x, y.float()), (x, y.bfloat16())):
            try:
                fn(*pair, win_size=7) if not isinstance(fn, torch_ops.SSIMLoss) else fn(*pair)
            except TypeError as e:
                assert "fixed window" not in str(e) and "two float32, two float16 or two bfloat16" in str(e), str(e)
            else:
                raise AssertionError("no TypeError for a mixed pair")
    try:
        torch_ops.SSIMLoss(win_size=7)(x, y.cpu())                            # not both on a GPU: what ssim raises
    except TypeError as e:
        assert "fixed window" in str(e), str(e)
    else:
        raise AssertionError("no TypeError")


CHECKS = [value_and_gradient_are_the_c_abi_bit_for_bit, non_contiguous_expanded_and_y_only, a_scaled_loss_is_rounded_once, side_stream,
          default_keywords_are_ssim_bit_for_bit, ssim_and_ssim_map_still_refuse_with_fixed_window]


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
