#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_ssimf.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

usage (GPU box):  python tests/tools/ssimf_torch_checks.py
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
import ssimf_model as M                             # noqa: E402
from conftest import GOLDEN, image_entries, load_pair   # noqa: E402
from ssim_amd import torch_ops                      # noqa: E402
from ssimf_model import G_TOL, GRAD_TOL             # noqa: E402


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def torch_pair(man):
    """(2, 3, H, W) tensors from six of the einstein pairs."""
    pool = []
    for n in image_entries(man):
        if n.startswith("einstein_") and n != "einstein_einstein":
            a, b = load_pair(man[n])
            pool.append((a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)))
    a = np.stack([np.stack([pool[(3 * i + c) % len(pool)][0] for c in range(3)]) for i in range(2)])
    b = np.stack([np.stack([pool[(3 * i + c) % len(pool)][1] for c in range(3)]) for i in range(2)])
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def abi_of_tensors(ctx, x, y, r, g_out):
    """The C ABI on the tensors' own memory (contiguous (N, C, H, W)): values and the gradient of x for dLoss/dS_i = g_out."""
    torch.cuda.synchronize()
    n, (h, w) = x.shape[0] * x.shape[1], x.shape[-2:]
    ps = (ssim_amd.ParamsF * n)()
    for i in range(n):
        ps[i] = ssim_amd.make_params_f(w, h, x.data_ptr() + 4 * i * h * w, 1, w, y.data_ptr() + 4 * i * h * w, 1, w)
    vals = ctx.ssimf_device(ps, n, r)
    go = torch.full((n,), g_out, dtype=torch.float32, device=x.device)
    gx = torch.empty_like(x)
    ga = (ssim_amd.GradF * n)()
    for i in range(n):
        ga[i] = ssim_amd.GradF(gx.data_ptr() + 4 * i * h * w, 1, w)
    torch.cuda.synchronize()
    ctx.enqueue_ssimf_grad(ps, n, r, go.data_ptr(), ga, None)
    ctx.synchronize()
    return vals, gx


def forward_and_backward_are_the_c_abi_bit_for_bit(man, ctx):
    x, y = torch_pair(man)
    x = x.clone().requires_grad_(True)
    s = torch_ops.ssim(x, y)
    assert s.shape == (2, 3) and s.dtype == torch.float32
    loss = torch_ops.SSIMLoss()(x, y)
    loss.backward()
    vals, gx = abi_of_tensors(ctx, x.detach(), y, 1.0, -1.0 / 6.0)
    assert np.array_equal(bits(s.detach().cpu().numpy().reshape(-1)), bits(vals))
    assert abs(float(loss) - (1.0 - float(np.mean(vals.astype(np.float64))))) < 1e-6
    assert torch.equal(x.grad, gx)
    # y alone, and both: only what needs a gradient gets one, with the same bits
    x2, y2 = x.detach().clone().requires_grad_(True), y.clone().requires_grad_(True)
    torch_ops.SSIMLoss()(x2, y2).backward()
    assert torch.equal(x2.grad, gx)
    y3 = y.clone().requires_grad_(True)
    torch_ops.SSIMLoss()(x.detach(), y3).backward()
    assert torch.equal(y3.grad, y2.grad)
    none = torch_ops.SSIMLoss(reduction="none")(x.detach(), y)
    assert none.shape == (2, 3) and not none.requires_grad
    for bad in (lambda: torch_ops.ssim(x.detach(), y, data_range=0.0), lambda: torch_ops.ssim(x.detach(), y[:, :, :-1]),
                lambda: torch_ops.ssim(x.detach(), y.cpu())):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("no ValueError")


def _slices():
    torch.manual_seed(3)
    big_x, big_y = torch.rand(4, 8, 40, 50, device="cuda"), torch.rand(4, 8, 44, 50, device="cuda")
    x, y = big_x[1:3, 2:8:2, 3:35, 5:45:2], big_y[0:2, 1:4, 7:39, 6:26]
    assert not x.is_contiguous() and not y.is_contiguous() and x.shape == y.shape == (2, 3, 32, 20)
    return big_x, big_y, x, y


def non_contiguous_slice_without_a_copy(man, ctx):
    big_x, big_y, x, y = _slices()
    xc, yc = x.contiguous().requires_grad_(True), y.contiguous()
    want = torch_ops.ssim(xc, yc)
    want.sum().backward()
    xs = x.detach().requires_grad_(True)
    assert xs.data_ptr() == x.data_ptr() and xs.stride() == x.stride()
    before = (big_x.clone(), big_y.clone())
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = torch_ops.ssim(xs, y)
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < x.numel() * 4, peak                   # the sums and the result only: no contiguous copy of a plane was made
    got.sum().backward()
    assert torch.equal(got, want) and torch.equal(xs.grad, xc.grad)
    assert torch.equal(big_x, before[0]) and torch.equal(big_y, before[1])


def non_default_stream(man, ctx):
    _, _, x, y = _slices()
    xc, yc = x.contiguous().requires_grad_(True), y.contiguous()
    want = torch_ops.ssim(xc, yc)                        # on the default stream
    want.sum().backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xq = xc.detach().clone().requires_grad_(True)
        on_side = torch_ops.ssim(xq, yc)
        on_side.sum().backward()
    side.synchronize()
    assert torch.equal(on_side, want) and torch.equal(xq.grad, xc.grad)


def gradient_ascent_raises_ssim_at_every_step(man, ctx):
    a, b = load_pair(man["einstein_jpg"])
    ref = torch.from_numpy(a.astype(np.float32) / np.float32(255)).cuda()
    x = torch.from_numpy(b.astype(np.float32) / np.float32(255)).cuda().requires_grad_(True)
    values = []
    for _ in range(21):
        s = torch_ops.ssim(x, ref)
        values.append(float(s))
        if len(values) == 21:
            break
        g, = torch.autograd.grad(s, x)
        with torch.no_grad():
            x += 10.0 * g                    # max|step| about 5e-3 of the range
    print("ascent: %.6f -> %.6f" % (values[0], values[-1]))
    assert all(values[i + 1] > values[i] for i in range(20)), values
    assert values[-1] > values[0] + 0.2


def gradient_agrees_with_a_float64_conv2d_restatement(man, ctx):
    """The composite users build today, in float64: five grouped conv2d of replicate-padded planes and autograd."""
    import torch.nn.functional as F
    x32, y32 = torch_pair(man)
    x = x32.double().requires_grad_(True)
    y = y32.double()
    g1 = torch.tensor(M.gaussian_taps(), dtype=torch.float64, device="cuda")
    win = (g1[:, None] * g1[None, :]).expand(3, 1, 11, 11).contiguous()
    c1, c2 = M.constants(1.0)

    def G(t):
        return F.conv2d(F.pad(t, (5, 5, 5, 5), mode="replicate"), win, groups=3)
    mx, my = G(x), G(y)
    sxx, syy, sxy = G(x * x) - mx * mx, G(y * y) - my * my, G(x * y) - mx * my
    smap = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    want = smap.mean(dim=(-2, -1))
    w = torch.tensor([[1.0, -0.5, 0.25], [2.0, 0.75, -1.5]], dtype=torch.float64, device="cuda")
    (want * w).sum().backward()
    xs = x32.clone().requires_grad_(True)
    got = torch_ops.ssim(xs, y32)
    (got * w.float()).sum().backward()
    dv = float((got.double() - want).abs().max())
    print("conv2d restatement: value %.3g" % dv)
    assert dv <= G_TOL
    for i in range(2):
        for c in range(3):
            e = float((xs.grad[i, c].double() - x.grad[i, c]).abs().max() / x.grad[i, c].abs().max())
            print("conv2d restatement: plane %d,%d gradient %.3g of max|grad|" % (i, c, e))
            assert e <= GRAD_TOL, (i, c, e)


CHECKS = [forward_and_backward_are_the_c_abi_bit_for_bit, non_contiguous_slice_without_a_copy, non_default_stream,
          gradient_ascent_raises_ssim_at_every_step, gradient_agrees_with_a_float64_conv2d_restatement]


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
