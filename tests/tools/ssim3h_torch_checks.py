#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_ssim3h.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/ssim3h_torch_checks.py
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
import halfmodel as HM                              # noqa: E402
from ssim_amd import torch_ops                      # noqa: E402

DTYPES = ((torch.float16, HM.F16), (torch.bfloat16, HM.BF16))


def u16(t):
    """The bit patterns of a float16 / bfloat16 tensor as a numpy uint16 array."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def same(t, want, enc):
    return HM.same(u16(t), u16(want) if isinstance(want, torch.Tensor) else want, enc)


def volumes(shape, seed, dtype):
    """x, y of `shape` (..., D, H, W): random volumes in [0, 1] and a noisy copy, rounded to dtype."""
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(a).cuda().to(dtype), torch.from_numpy(b).cuda().to(dtype)


def abi_of_tensors(ctx, x, y, enc, r, g_out, gmap=None):
    """The C ABI on the tensors' own memory (contiguous (N, C, D, H, W), 16-bit): values, maps, and the gradients of x and y for
    dLoss/dS_i = g_out (gmap None) or for the dense float32 upstream volume gmap."""
    torch.cuda.synchronize()
    n, (d, h, w) = x.shape[0] * x.shape[1], x.shape[-3:]
    vox = d * h * w
    m = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    ps = (ssim_amd.Params3H * n)()
    for i in range(n):
        ps[i] = ssim_amd.make_params3h(w, h, d, x.data_ptr() + 2 * i * vox, (1, w, w * h), y.data_ptr() + 2 * i * vox, (1, w, w * h), m.data_ptr() + 4 * i * vox)
    vals = ctx.ssim3h_device(ps, n, r, enc)
    gx, gy = torch.empty_like(x), torch.empty_like(y)
    ga, gb = (ssim_amd.Grad3H * n)(), (ssim_amd.Grad3H * n)()
    for i in range(n):
        ga[i], gb[i] = ssim_amd.Grad3H(gx.data_ptr() + 2 * i * vox, 1, w, w * h), ssim_amd.Grad3H(gy.data_ptr() + 2 * i * vox, 1, w, w * h)
    torch.cuda.synchronize()
    if gmap is None:
        go = torch.full((n,), g_out, dtype=torch.float32, device=x.device)
        ctx.enqueue_ssim3h_grad(ps, n, r, enc, go.data_ptr(), ga, gb)
    else:
        assert gmap.is_contiguous() and gmap.dtype == torch.float32 and gmap.shape == x.shape
        gm = (ssim_amd.GradOut3F * n)()
        for i in range(n):
            gm[i] = ssim_amd.GradOut3F(gmap.data_ptr() + 4 * i * vox, 1, w, w * h)
        ctx.enqueue_ssim3h_map_grad(ps, n, r, enc, gm, ga, gb)
    ctx.synchronize()
    return vals, m, gx, gy


def forward_and_backward_are_the_c_abi(ctx):
    for dtype, enc in DTYPES:
        x, y = volumes((2, 2, 9, 20, 33), 1, dtype)
        x, y = x.requires_grad_(True), y.requires_grad_(True)
        s = torch_ops.ssim3d_amp(x, y)
        assert s.shape == (2, 2) and s.dtype == torch.float32                # float32 at every input dtype
        scale = float(9 * 20 * 33)                                            # keeps the float16 gradient in the normal range
        loss = torch_ops.SSIM3DLoss()(x, y)
        assert loss.dtype == torch.float32
        (loss * scale).backward()
        assert x.grad.dtype == dtype and y.grad.dtype == dtype and x.grad.shape == x.shape      # the gradient has the inputs' dtype
        g_out = float(np.float32(-scale) / np.float32(4.0))                  # what autograd hands the backward: scale / 4 volumes, negated
        vals, m_abi, gx, gy = abi_of_tensors(ctx, x.detach(), y.detach(), enc, 1.0, g_out)
        assert np.array_equal(s.detach().cpu().numpy().reshape(-1).view(np.uint32), vals.view(np.uint32))
        assert same(x.grad, gx, enc) and same(y.grad, gy, enc) and float(x.grad.float().abs().max()) > 0
        # ... which is the float32 path on the widened tensors, rounded once
        xf, yf = x.detach().float().requires_grad_(True), y.detach().float().requires_grad_(True)
        sf = torch_ops.ssim3d(xf, yf)
        assert torch.equal(sf, s.detach())
        ((1.0 - sf).mean() * scale).backward()
        assert same(x.grad, HM.round_to(xf.grad.cpu().numpy(), enc), enc) and same(y.grad, HM.round_to(yf.grad.cpu().numpy(), enc), enc)
        # one input alone: only what needs a gradient gets one, with the same bits
        x2 = x.detach().clone().requires_grad_(True)
        (torch_ops.SSIM3DLoss()(x2, y.detach()) * scale).backward()
        assert same(x2.grad, gx, enc)
        # the map and its backward for a per-voxel upstream gradient
        torch.manual_seed(2)
        w = torch.randn(x.shape, device="cuda") * 100.0
        x3, y3 = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
        m = torch_ops.ssim3d_map_amp(x3, y3)
        assert m.shape == x.shape and m.dtype == torch.float32 and torch.equal(m.detach(), m_abi)
        assert torch.equal(m.detach(), torch_ops.ssim3d_map(x.detach().float(), y.detach().float()))
        saved = [t.data_ptr() for t in m.grad_fn.saved_tensors]
        assert sorted(saved) == sorted([x3.data_ptr(), y3.data_ptr()])      # x and y are saved, not the map
        m.backward(w)
        _, _, gx, gy = abi_of_tensors(ctx, x.detach(), y.detach(), enc, 1.0, None, gmap=w)
        assert same(x3.grad, gx, enc) and same(y3.grad, gy, enc) and x3.grad.dtype == dtype
        # float32 tensors: exactly ssim3d
        assert torch.equal(torch_ops.ssim3d_amp(xf.detach(), yf.detach()), sf.detach())
        none = torch_ops.SSIM3DLoss(reduction="none")(x.detach(), y.detach())
        assert none.shape == (2, 2) and none.dtype == torch.float32


def non_contiguous_and_expanded_inputs_are_read_in_place(ctx):
    for dtype, enc in DTYPES:
        torch.manual_seed(3)
        big_x, big_y = torch.rand(3, 4, 14, 30, 41, device="cuda").to(dtype), torch.rand(40, 3, 12, 26, device="cuda").to(dtype)
        x = big_x[0:2, 1:4:2, 2:12, 3:27, 6:40:2]                      # (2, 2, 10, 24, 17): an odd element offset, step 2
        y = big_y[3:37:2, 0:2, 1:11, 2:26].permute(1, 2, 3, 0)[:, None].expand(2, 2, 10, 24, 17)      # W stored outermost; the second dimension expanded
        assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape and y.stride(1) == 0
        assert x.data_ptr() % 4 == 2                                   # 2-byte but not 4-byte aligned
        big_w = torch.randn(2, 2, 24, 10, 40, device="cuda") * 100.0
        w = big_w[..., 3:37:2].permute(0, 1, 3, 2, 4)                  # (2, 2, 10, 24, 17): H and D exchanged in storage, step 2
        xc, yc = x.contiguous().requires_grad_(True), y.contiguous().requires_grad_(True)
        want_v = torch_ops.ssim3d_amp(xc, yc)
        (want_v.sum() * 4080.0).backward()
        gvx, gvy = xc.grad.clone(), yc.grad.clone()
        xc.grad = yc.grad = None
        want_m = torch_ops.ssim3d_map_amp(xc, yc)
        want_m.backward(w.contiguous())
        before = (big_x.clone(), big_y.clone(), big_w.clone())
        xs, ys = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
        assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride() and ys.data_ptr() == y.data_ptr() and ys.stride() == y.stride()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        got_v = torch_ops.ssim3d_amp(xs, ys)
        peak = torch.cuda.max_memory_allocated() - base
        assert peak < x.numel() * 2, peak                              # the sums and the result only: no contiguous copy of a volume
        (got_v.sum() * 4080.0).backward()
        assert torch.equal(got_v, want_v) and same(xs.grad, gvx, enc) and same(ys.grad, gvy, enc) and xs.grad.dtype == dtype
        xs.grad = ys.grad = None
        got_m = torch_ops.ssim3d_map_amp(xs, ys)
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        got_m.backward(w)                                              # a sliced, permuted grad_out, read in place
        peak = torch.cuda.max_memory_allocated() - base
        assert peak < 3 * x.numel() * 2, peak                          # the two 16-bit gradients only: no copy of grad_out, x or y
        assert torch.equal(got_m, want_m) and same(xs.grad, xc.grad, enc) and same(ys.grad, yc.grad, enc)
        assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1]) and torch.equal(big_w, before[2])


def loss_under_autocast(ctx):
    torch.manual_seed(5)
    conv = torch.nn.Conv3d(2, 2, 3, padding=1).cuda()
    vol, target = torch.rand(2, 2, 10, 24, 20, device="cuda"), torch.rand(2, 2, 10, 24, 20, device="cuda")
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out = conv(vol)
        assert out.dtype == torch.bfloat16
        loss = torch_ops.SSIM3DLoss()(out, target.to(torch.bfloat16))        # taken as it comes: not itself autocast
        assert loss.dtype == torch.float32
        want = (1.0 - torch_ops.ssim3d(out.detach().float(), target.to(torch.bfloat16).float())).mean()
        assert torch.equal(loss.detach(), want)
        try:
            torch_ops.ssim3d_amp(out, target)                                # a mixed pair stays a TypeError inside autocast
        except TypeError:
            pass
        else:
            raise AssertionError("no TypeError")
    loss.backward()
    g = conv.weight.grad
    assert g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert 0.0 < float(loss) < 2.0


def loss_scale_arrives_before_the_rounding(ctx):
    """A loss scaled by 65536 (what GradScaler does) arrives in grad_out, which stays float32, and is applied before the single rounding:
    round(65536 g), not 65536 round(g) -- in float16 the unscaled gradient of a mean over 4 x 5940 voxels is subnormal or zero."""
    for dtype, enc in DTYPES:
        x, y = volumes((2, 2, 9, 20, 33), 6, dtype)
        x = x.requires_grad_(True)
        (torch_ops.SSIM3DLoss()(x, y) * 65536.0).backward()
        xf = x.detach().float().requires_grad_(True)
        (torch_ops.SSIM3DLoss()(xf, y.float()) * 65536.0).backward()
        assert same(x.grad, HM.round_to(xf.grad.cpu().numpy(), enc), enc)                    # round(65536 g)
        xu = x.detach().clone().requires_grad_(True)
        torch_ops.SSIM3DLoss()(xu, y).backward()
        twice = (xu.grad.float() * 65536.0).to(dtype)                                        # 65536 round(g)
        differ = int((u16(twice) != u16(x.grad)).sum())
        print("scaled loss, %s: %d of %d voxels differ from 65536 * round(g)" % (enc, differ, x.numel()))
        if enc == HM.F16:                                    # bfloat16 has float32's exponent range: a power of two commutes with its rounding
            tiny = int(HM.is_subnormal(u16(xu.grad), enc).sum() + ((u16(xu.grad) & 0x7FFF) == 0).sum())
            print("scaled loss, float16: %d of %d unscaled gradient voxels are subnormal or zero" % (tiny, x.numel()))
            assert differ > 0 and tiny > 0                   # the unscaled float16 gradient has lost bits the scaled one keeps


def masked_map_loss(ctx):
    """1 - (mask * ssim3d_map_amp(x, y)).sum() / mask.sum(), and sum().backward(), whose grad_out is one expanded float."""
    for dtype, enc in DTYPES:
        x, y = volumes((2, 1, 12, 18, 21), 7, dtype)
        torch.manual_seed(8)
        mask = (torch.rand(x.shape, device="cuda") < 0.3).float()
        xs = x.clone().requires_grad_(True)
        loss = 1 - (mask * torch_ops.ssim3d_map_amp(xs, y)).sum() / mask.sum()
        assert loss.dtype == torch.float32
        (loss * 1024.0).backward()
        xf = x.float().requires_grad_(True)
        lf = 1 - (mask * torch_ops.ssim3d_map(xf, y.float())).sum() / mask.sum()
        (lf * 1024.0).backward()
        assert torch.equal(loss.detach(), lf.detach()) and xs.grad.dtype == dtype
        assert same(xs.grad, HM.round_to(xf.grad.cpu().numpy(), enc), enc) and float(xs.grad.float().abs().max()) > 0
        seen = []
        xs2, xf2 = x.clone().requires_grad_(True), x.float().requires_grad_(True)
        m = torch_ops.ssim3d_map_amp(xs2, y)
        m.register_hook(lambda g: seen.append(g))
        (m.sum() * 0.5).backward()
        assert len(seen) == 1 and seen[0].dtype == torch.float32
        print("sum: grad_out arrives with strides %r" % (tuple(seen[0].stride()),))
        (torch_ops.ssim3d_map(xf2, y.float()).sum() * 0.5).backward()
        assert same(xs2.grad, HM.round_to(xf2.grad.cpu().numpy(), enc), enc)


def mixed_pairs_are_refused(ctx):
    x, y = volumes((1, 1, 6, 8, 9), 9, torch.float16)
    for fn in (torch_ops.ssim3d_amp, torch_ops.ssim3d_map_amp, torch_ops.SSIM3DLoss()):
        for pair in ((x, y.float()), (x.float(), y), (x, y.bfloat16()), (x.bfloat16(), y.float())):
            try:
                fn(*pair)
            except TypeError:
                continue
            raise AssertionError("no TypeError for %s and %s" % (pair[0].dtype, pair[1].dtype))
        for pair, exc in (((x.cpu(), y.cpu()), TypeError), ((x, y.cpu()), ValueError), ((x, y[..., :-1]), ValueError), ((x.double(), y.double()), TypeError)):
            try:
                fn(*pair)
            except exc:
                continue
            raise AssertionError("no %s" % exc.__name__)
    for fn in (torch_ops.ssim3d, torch_ops.ssim3d_map):                       # the float32-only names keep their refusal on the GPU too
        try:
            fn(x, y)
        except TypeError as e:
            assert "float32 for now" in str(e)
        else:
            raise AssertionError("no TypeError")


def side_stream(ctx):
    for dtype, enc in DTYPES:
        x, y = volumes((2, 1, 12, 18, 21), 4, dtype)
        torch.manual_seed(5)
        w = torch.randn(x.shape, device="cuda") * 100.0
        assert torch.cuda.current_stream().cuda_stream == 0                  # the legacy default stream
        xc = x.clone().requires_grad_(True)
        want_v = torch_ops.ssim3d_amp(xc, y)
        (want_v.sum() * 4536.0).backward()
        gv = xc.grad.clone()
        xc.grad = None
        want_m = torch_ops.ssim3d_map_amp(xc, y)
        (w * want_m).sum().backward()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream().cuda_stream != 0
            xq = x.clone().requires_grad_(True)
            on_side = torch_ops.ssim3d_amp(xq, y)
            (on_side.sum() * 4536.0).backward()
            gq = xq.grad.clone()
            xq.grad = None
            map_on_side = torch_ops.ssim3d_map_amp(xq, y)
            (w * map_on_side).sum().backward()
        side.synchronize()
        assert torch.equal(on_side, want_v) and same(gq, gv, enc) and torch.equal(map_on_side, want_m) and same(xq.grad, xc.grad, enc)
        assert float(gv.float().abs().max()) > 0


CHECKS = [forward_and_backward_are_the_c_abi, non_contiguous_and_expanded_inputs_are_read_in_place, loss_under_autocast,
          loss_scale_arrives_before_the_rounding, masked_map_loss, mixed_pairs_are_refused, side_stream]


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
