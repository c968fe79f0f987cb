#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_mixed_step3.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

A combined step with the 3-D losses in it: eight losses -- SSIM of volumes at the engine's window, under a 7 x 7 x 7 box, a weighted sum
over the 3-D SSIM map under a 5-tap Gaussian of sigma 0.8, MS-SSIM of volumes at three scales, SSIM of bfloat16 volumes, a weighted sum
over the SSIM map of float16 volumes, and 2-D MS-SSIM at three scales and 2-D SSIM so that planes and volumes share the context -- each
on a leaf pair of its own (clones of the same data), summed, one backward(), no synchronise inside.  ssim_amd.torch_ops keeps one context
per (device, stream), so all of it lands on one context.  Every loss value and every leaf's gradient must have the bits of the same loss
computed and back-propagated ALONE after a torch.cuda.synchronize().

usage (GPU box):  python tests/tools/mixed_step3_torch_checks.py
"""
import json
import os
import sys
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ssim_amd import torch_ops                      # noqa: E402

VOLUMES = (2, 2, 13, 20, 33)                        # (N, C, D, H, W)
THIN = (2, 2, 40, 3, 5)                             # 5 x 3 x 40 volumes
PLANES = (2, 3, 65, 257)                            # (N, C, H, W)
MS3_WEIGHTS = (0.2, 0.3, 0.5)


def tensors(shape, seed):
    torch.manual_seed(seed)
    x = torch.rand(shape, device="cuda")
    y = (x + 0.1 * torch.randn(shape, device="cuda")).clamp(0, 1)
    w = torch.randn(shape, device="cuda")
    return x, y, w


def data(volumes=VOLUMES, planes=PLANES, seed=3):
    """{3: (x, y, w) of volumes, 2: (x, y, w) of planes}."""
    return {3: tensors(volumes, seed), 2: tensors(planes, seed + 100)}


def same(t, u):
    """The same bits (the tensors here hold no NaN)."""
    assert t.dtype == u.dtype and t.shape == u.shape, (t.dtype, u.dtype, t.shape, u.shape)
    as_int = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return torch.equal(t.contiguous().view(as_int), u.contiguous().view(as_int))


def losses(d):
    """(name, 3 for volumes / 2 for planes, dtype of the leaves, loss of a leaf pair)."""
    w3 = d[3][2]
    return (("ssim3d", 3, torch.float32, torch_ops.SSIM3DLoss()),
            ("ssim3d 7x7x7 box", 3, torch.float32, torch_ops.SSIM3DLoss(win_size=7, window="uniform")),
            ("map3d 5 taps sigma 0.8, weighted", 3, torch.float32, lambda x, y: (w3 * torch_ops.ssim3d_map(x, y, win_size=5, win_sigma=0.8)).sum()),
            ("ms-ssim3d 3 scales", 3, torch.float32, torch_ops.MSSSIM3DLoss(scales=3, weights=MS3_WEIGHTS)),
            ("ssim3d bfloat16", 3, torch.bfloat16, lambda x, y: 1.0 - torch_ops.ssim3d_amp(x, y).mean()),
            ("map3d float16, weighted", 3, torch.float16, lambda x, y: (w3 * torch_ops.ssim3d_map_amp(x, y)).sum()),
            ("ms-ssim 3 scales", 2, torch.float32, torch_ops.MSSSIMLoss(scales=3, weights=MS3_WEIGHTS)),
            ("ssim", 2, torch.float32, torch_ops.SSIMLoss()))


def leaves(x, y, dtype):
    return x.to(dtype).clone().requires_grad_(True), y.to(dtype).clone().requires_grad_(True)


def forward(d):
    """The eight losses on leaves of their own and their sum; nothing waits for the host."""
    made = [(name,) + leaves(d[dims][0], d[dims][1], dtype) + (fn,) for name, dims, dtype, fn in losses(d)]
    vals = [fn(lx, ly) for _, lx, ly, fn in made]
    total = vals[0]
    for v in vals[1:]:
        total = total + v
    return made, vals, total


def collect(made, vals):
    return [(name, v.detach(), lx.grad, ly.grad) for (name, lx, ly, _), v in zip(made, vals)]


def combined(d):
    made, vals, total = forward(d)
    total.backward()
    return collect(made, vals)


def alone(d):
    """Each loss by itself: a synchronise before it, its own backward, a synchronise after it."""
    out = []
    for name, dims, dtype, fn in losses(d):
        torch.cuda.synchronize()
        lx, ly = leaves(d[dims][0], d[dims][1], dtype)
        v = fn(lx, ly)
        v.backward()
        torch.cuda.synchronize()
        out.append((name, v.detach(), lx.grad, ly.grad))
    return out


def hold(got, want, what):
    assert len(got) == len(want) == 8
    for (name, v, gx, gy), (_, wv, wx, wy) in zip(got, want):
        assert v.dtype == torch.float32 and same(v, wv), (what, name, "loss", float(v), float(wv))
        assert gx is not None and gy is not None and same(gx, wx) and same(gy, wy), (what, name, "gradient")
        assert bool(torch.isfinite(gx.float()).all()) and bool(torch.isfinite(gy.float()).all()), (what, name)
        assert float(gx.float().abs().max()) > 0 and float(gy.float().abs().max()) > 0, (what, name)
    print("%s: %s" % (what, ", ".join("%s %.6f" % (name, float(v)) for name, v, _, _ in got)))


def combined_step_has_the_bits_of_each_loss_alone():
    d = data()
    torch.cuda.synchronize()
    got = combined(d)
    torch.cuda.synchronize()
    hold(got, alone(d), "combined step, volumes %r, planes %r" % (VOLUMES, PLANES))


def steps_of_changing_shape():
    """33 x 20 x 13 volumes (and 257 x 65 planes), then 5 x 3 x 40 volumes (and 33 x 17 planes), then the first shapes again: the
    context's scratch is reused by launches of another geometry and then by the first one again."""
    first, thin = data(seed=5), data(THIN, (2, 3, 17, 33), seed=6)
    torch.cuda.synchronize()
    got = [combined(d) for d in (first, thin, first)]            # back to back
    torch.cuda.synchronize()
    for step, (g, d) in enumerate(zip(got, (first, thin, first))):
        hold(g, alone(d), "step %d, %s" % (step, tuple(d[3][0].shape)))
    for (name, v, gx, gy), (_, v2, gx2, gy2) in zip(got[0], got[2]):
        assert same(v, v2) and same(gx, gx2) and same(gy, gy2), ("first and third step", name)


def two_streams():
    """A combined step on the default stream and another inside torch.cuda.stream(side), issued alternately: forward here, forward
    there, backward here, backward there."""
    here, there = data(seed=7), data(seed=8)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    f0 = forward(here)
    with torch.cuda.stream(side):
        f1 = forward(there)
    f0[2].backward()
    with torch.cuda.stream(side):
        f1[2].backward()
    torch.cuda.synchronize()
    assert len(set(k[1] for k in torch_ops._contexts)) >= 2, "the two steps ran on one context"
    hold(collect(f0[0], f0[1]), alone(here), "default stream")
    hold(collect(f1[0], f1[1]), alone(there), "side stream")


CHECKS = [combined_step_has_the_bits_of_each_loss_alone, steps_of_changing_shape, two_streams]


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
