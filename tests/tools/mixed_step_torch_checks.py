#!/usr/bin/env python3
"""The PyTorch checks of tests/test_gpu_mixed_step.py, run in a process of their own: torch is imported BEFORE the library, so that the
process holds one HIP runtime (torch's).  Prints what each check measures and one line `RESULT {json}`: "ok" or the traceback per check.

A combined step: six losses -- SSIM at the engine's window, SSIM under a 7 x 7 box, a weighted sum over the 3 x 3 box SSIM map, MS-SSIM
at three scales on float32, MS-SSIM at Wang's five scales on bfloat16 and SSIM on float16 -- each on a leaf pair of its own (clones of
the same data), summed, one backward(), no synchronise inside.  ssim_amd.torch_ops keeps one context per (device, stream), so all of it
lands on one context.  Every loss value and every leaf's gradient must have the bits of the same loss computed and back-propagated
ALONE after a torch.cuda.synchronize().

usage (GPU box):  python tests/tools/mixed_step_torch_checks.py
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

SHAPE = (2, 3, 65, 257)                             # (N, C, H, W)
MS3_WEIGHTS = (0.2, 0.3, 0.5)


def tensors(shape=SHAPE, seed=3):
    torch.manual_seed(seed)
    x = torch.rand(shape, device="cuda")
    y = (x + 0.1 * torch.randn(shape, device="cuda")).clamp(0, 1)
    w = torch.randn(shape, device="cuda")
    return x, y, w


def same(t, u):
    """The same bits (the tensors here hold no NaN)."""
    assert t.dtype == u.dtype and t.shape == u.shape, (t.dtype, u.dtype, t.shape, u.shape)
    as_int = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return torch.equal(t.contiguous().view(as_int), u.contiguous().view(as_int))


def losses(w):
    """(name, dtype of the leaves, loss of a leaf pair): none of them documented as refused by torch_ops (16-bit tensors keep the fixed
    window)."""
    return (("ssim", torch.float32, torch_ops.SSIMLoss()),
            ("ssim 7x7 box", torch.float32, torch_ops.SSIMLoss(win_size=7, window="uniform")),
            ("map 3x3 box, weighted", torch.float32, lambda x, y: (w * torch_ops.ssim_map(x, y, win_size=3, window="uniform")).sum()),
            ("ms-ssim 3 scales", torch.float32, torch_ops.MSSSIMLoss(scales=3, weights=MS3_WEIGHTS)),
            ("ms-ssim bfloat16", torch.bfloat16, torch_ops.MSSSIMLoss()),
            ("ssim float16", torch.float16, torch_ops.SSIMLoss()))


def leaves(x, y, dtype):
    return x.to(dtype).clone().requires_grad_(True), y.to(dtype).clone().requires_grad_(True)


def forward(x, y, w):
    """The six losses on leaves of their own and their sum; nothing waits for the host."""
    made = [(name,) + leaves(x, y, dtype) + (fn,) for name, dtype, fn in losses(w)]
    vals = [fn(lx, ly) for _, lx, ly, fn in made]
    total = vals[0]
    for v in vals[1:]:
        total = total + v
    return made, vals, total


def collect(made, vals):
    return [(name, v.detach(), lx.grad, ly.grad) for (name, lx, ly, _), v in zip(made, vals)]


def combined(x, y, w):
    made, vals, total = forward(x, y, w)
    total.backward()
    return collect(made, vals)


def alone(x, y, w):
    """Each loss by itself: a synchronise before it, its own backward, a synchronise after it."""
    out = []
    for name, dtype, fn in losses(w):
        torch.cuda.synchronize()
        lx, ly = leaves(x, y, dtype)
        v = fn(lx, ly)
        v.backward()
        torch.cuda.synchronize()
        out.append((name, v.detach(), lx.grad, ly.grad))
    return out


def hold(got, want, what):
    assert len(got) == len(want) == 6
    for (name, v, gx, gy), (_, wv, wx, wy) in zip(got, want):
        assert v.dtype == torch.float32 and same(v, wv), (what, name, "loss", float(v), float(wv))
        assert gx is not None and gy is not None and same(gx, wx) and same(gy, wy), (what, name, "gradient")
        assert bool(torch.isfinite(gx.float()).all()) and bool(torch.isfinite(gy.float()).all()), (what, name)
        if gx.dtype == torch.float32:
            assert float(gx.abs().max()) > 0 and float(gy.abs().max()) > 0, (what, name)
    print("%s: %s" % (what, ", ".join("%s %.6f" % (name, float(v)) for name, v, _, _ in got)))


def combined_step_has_the_bits_of_each_loss_alone():
    x, y, w = tensors()
    torch.cuda.synchronize()
    got = combined(x, y, w)
    torch.cuda.synchronize()
    hold(got, alone(x, y, w), "combined step, %d x %d x %d x %d" % SHAPE)


def steps_of_changing_shape():
    """33 x 17, then 2 x 3 x 300 x 260, then 33 x 17 again: the context's scratch grows and is then reused small."""
    small, big = tensors((2, 3, 17, 33), seed=5), tensors((2, 3, 300, 260), seed=6)
    torch.cuda.synchronize()
    got = [combined(*t) for t in (small, big, small)]            # back to back
    torch.cuda.synchronize()
    for step, (g, t) in enumerate(zip(got, (small, big, small))):
        hold(g, alone(*t), "step %d, %s" % (step, tuple(t[0].shape)))
    for (name, v, gx, gy), (_, v2, gx2, gy2) in zip(got[0], got[2]):
        assert same(v, v2) and same(gx, gx2) and same(gy, gy2), ("first and third step", name)


def two_streams():
    """A combined step on the default stream and another inside torch.cuda.stream(side), issued alternately: forward here, forward
    there, backward here, backward there."""
    here, there = tensors(seed=7), tensors(seed=8)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    f0 = forward(*here)
    with torch.cuda.stream(side):
        f1 = forward(*there)
    f0[2].backward()
    with torch.cuda.stream(side):
        f1[2].backward()
    torch.cuda.synchronize()
    assert len(set(k[1] for k in torch_ops._contexts)) >= 2, "the two steps ran on one context"
    hold(collect(f0[0], f0[1]), alone(*here), "default stream")
    hold(collect(f1[0], f1[1]), alone(*there), "side stream")


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
