"""CPU: SSIM of float32 volumes under the three-dimensional window and its gradient -- the definition and its boundaries
(include/rmgr/ssim-hip.h, rmgr_ssim_hip_*_ssim3f*).  Sizes are W x H x D; arrays are (D, H, W).

  * the float64 model (tests/ssim3f_model.py) agrees with an independent restatement -- torch float64, F.conv3d on replicate-padded
    input, autograd -- within 1e-9: value, map, both gradients, down to 1 x 1 x 1;
  * Gt is the adjoint of G, and the model on a volume of one slice whose window collapses is the 2-D model's limit;
  * the fp32 emulation of the kernels leaves the figures ssim3f_model.EMU_* hold, pinned from both sides;
  * the entry points are exported, every EINVAL comes before the device, a valid call without a device is ENODEV, and
    ssim_amd.torch_ops refuses what it documents before any GPU call;
  * the new kernels never spill, keep two waves per SIMD and 64 KiB of LDS per workgroup, and there are eight of them.
"""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import ssim3f_model as S
import ssim_amd
from conftest import ROOT

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_ssim3f", "rmgr_ssim_hip_compute_ssim3f_device", "rmgr_ssim_hip_compute_ssim3f_host",
                "rmgr_ssim_hip_enqueue_ssim3f_grad")
SIZES = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (5, 3, 4), (13, 12, 11)]


def _torch_restatement(a, b, data_range, g_out):
    """(value, map, dA, dB) by torch float64: 1-D conv3d per axis on replicate-padded volumes, the five statistics, autograd."""
    import torch
    import torch.nn.functional as Fn
    g = torch.tensor(S.gaussian_taps(), dtype=torch.float64)
    c1, c2 = S.constants(data_range)

    def blur(v):
        v = v[None, None]
        v = Fn.conv3d(Fn.pad(v, (5, 5, 0, 0, 0, 0), mode="replicate"), g.reshape(1, 1, 1, 1, 11))
        v = Fn.conv3d(Fn.pad(v, (0, 0, 5, 5, 0, 0), mode="replicate"), g.reshape(1, 1, 1, 11, 1))
        v = Fn.conv3d(Fn.pad(v, (0, 0, 0, 0, 5, 5), mode="replicate"), g.reshape(1, 1, 11, 1, 1))
        return v[0, 0]
    ta = torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    tb = torch.tensor(np.asarray(b, np.float64), requires_grad=True)
    ma, mb = blur(ta), blur(tb)
    s_aa, s_bb, s_ab = blur(ta * ta) - ma * ma, blur(tb * tb) - mb * mb, blur(ta * tb) - ma * mb
    m = (2 * ma * mb + c1) * (2 * s_ab + c2) / ((ma * ma + mb * mb + c1) * (s_aa + s_bb + c2))
    value = m.sum() / S.voxels(a.shape)
    (g_out * value).backward()
    return float(value.detach()), m.detach().numpy(), ta.grad.numpy(), tb.grad.numpy()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_model_is_the_conv3d_restatement(size):
    w, h, d = size
    rng = np.random.default_rng(w * 100 + h * 10 + d)
    a = rng.random((d, h, w)).astype(np.float32)
    b = np.clip(a + 0.1 * rng.standard_normal((d, h, w)), 0, 1).astype(np.float32)
    for r, sa, sb in ((1.0, a, b), (255.0, a * np.float32(255), b * np.float32(255))):
        value, m = S.ssim(sa, sb, r)
        da, db = S.grad(sa, sb, r, -0.75)
        tv, tm, tda, tdb = _torch_restatement(sa, sb, r, -0.75)
        assert abs(value - tv) <= 1e-9 and np.abs(m - tm).max() <= 1e-9, (size, r, value, tv)
        assert np.abs(da - tda).max() <= 1e-9 and np.abs(db - tdb).max() <= 1e-9, (size, r)
        assert np.abs(tda).max() > 1e-6 / r                      # a gradient worth comparing


def test_gt_is_the_adjoint_of_g():
    rng = np.random.default_rng(11)
    for shape in [(12, 14, 16), (1, 1, 1), (1, 7, 3), (3, 1, 20), (6, 6, 6), (2, 5, 1)]:
        u, v = rng.standard_normal(shape), rng.standard_normal(shape)
        lhs, rhs = float(np.sum(S.blur(u) * v)), float(np.sum(u * S.blur_t(v)))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-3), (shape, lhs, rhs)


def test_a_stack_of_equal_slices_is_the_2d_model_up_to_the_taps_sum():
    """Every slice the same: the z pass multiplies by the sum of the eleven float taps, which is 1 to 3e-8."""
    import ssimf_model as M
    rng = np.random.default_rng(3)
    a, b = rng.random((9, 11)), rng.random((9, 11))
    v3, m3 = S.ssim(np.stack([a] * 4), np.stack([b] * 4), 1.0)
    v2, m2 = M.ssim(a, b, 1.0)
    assert abs(v3 - v2) < 1e-6 and np.abs(m3 - m2[None]).max() < 1e-6


def test_centre_is_one_per_volume_and_bounded_by_the_range():
    vol = np.arange(4 * 5 * 300, dtype=np.float32).reshape(4, 5, 300)
    assert S.centre(vol, 1e6) == vol[1, 2, 149]
    assert S.centre(vol, 10.0) == 0.0
    vol[1, 2, 149] = np.nan
    assert S.centre(vol, 1e6) == 0.0
    assert S.centre(np.full((1, 1, 1), 0.5, np.float32), 1.0) == np.float32(0.5)


def test_fp32_emulation_leaves_the_pinned_figures(manifest):
    """emulate_fp32 against the float64 model on the golden volumes (slice z of a volume is the crop img[z : z + H - 11, 2z : 2z + W - 22],
    z = 0 .. 11; the four bbb channel-1 pairs and einstein_blur; forms unit and raw; every fixture's A against itself for the identical
    pair).  Measured: 5.29e-4 per voxel, 4.73e-6 global, 9.45e-5 of the volume's largest float64 gradient magnitude, 4.06e-4 for
    max|grad| * W * H * D * R on identical volumes.  tests/test_gpu_ssim3f.py asserts twice ssim3f_model.EMU_*."""
    got = S.measure(manifest)
    print("emulation: px %.3g global %.3g grad %.3g identical %.3g" % got)
    for v, emu, tol in zip(got, (S.EMU_PX, S.EMU_G, S.EMU_GRAD, S.EMU_IDENT), S.tolerances()):
        assert v <= emu, (got, emu)
        # pinned from below as well: a figure that moved far away means the emulation no longer restates these kernels
        assert v >= emu / 2, (got, emu)
        assert tol == 2.0 * emu


# ---- the C ABI's validation (no device needed) ----

def _params(a, b, n=1, **over):
    ps = (ssim_amd.Params3F * n)()
    d, h, w = a.shape
    for i in range(n):
        ps[i] = ssim_amd.make_params3f(w, h, d, a.ctypes.data, (1, w, w * h), b.ctypes.data, (1, w, w * h))
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _grads(a, n=1):
    gs = (ssim_amd.Grad3F * n)()
    for i in range(n):
        gs[i] = ssim_amd.Grad3F(a.ctypes.data, 1, a.shape[2], a.shape[2] * a.shape[1])
    return gs


def test_entry_points_are_exported(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS
    for name in ("Img3F", "Params3F", "Grad3F", "make_params3f", "compute_ssim3f", "compute_ssim3f_batch"):
        assert hasattr(ssim_amd, name)
    for name in ("ssim3f_device", "enqueue_ssim3f", "enqueue_ssim3f_grad"):
        assert hasattr(ssim_amd.Context, name)
    assert lib.rmgr_ssim_hip_get_abi_version() == 6
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS + ("rmgr_ssim_hip_Img3F", "rmgr_ssim_hip_Params3F", "rmgr_ssim_hip_Grad3F"):
        assert name in header


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    a = np.zeros((6, 20, 30), np.float32)
    b = np.zeros((6, 20, 30), np.float32)
    ga = np.zeros((6, 20, 30), np.float32)
    grad = fn.endswith("_grad")
    out = (ctypes.c_float * 4)() if not fn.startswith("rmgr_ssim_hip_enqueue") else ctypes.c_void_p(16)   # never dereferenced
    fake_ctx = None if fn.endswith("_host") else ctypes.c_void_p(1)                                     # never dereferenced
    E = errno.EINVAL
    f = getattr(lib, fn)

    def rc(count=1, params=None, r=1.0, o=out, ctx=fake_ctx, grads=None):
        ps = _params(a, b, max(count, 1)) if params is None else params
        if grad:
            ga_, gb_ = (_grads(ga, max(count, 1)), None) if grads is None else grads
            return f(ctx, count, ps, r, o, ga_, gb_)
        return f(ctx, count, ps, r, o)
    assert rc(count=0) == E
    assert (f(fake_ctx, 1, None, 1.0, out, _grads(ga), None) if grad else f(fake_ctx, 1, None, 1.0, out)) == E      # params NULL
    assert rc(o=None) == E                                                     # ssim / sumsDevice / gradOutDevice NULL
    for dim in ("width", "height", "depth"):
        assert rc(params=_params(a, b, **{dim: 0})) == E
        assert rc(params=_params(a, b, **{dim: 0x7FFF0001})) == E              # above the kernels' limit
        two = _params(a, b, 2)
        setattr(two[1], dim, getattr(two[1], dim) - 1)
        assert rc(count=2, params=two) == E                                    # sizes differ
    bad = _params(a, b)
    bad[0].imgA.topLeft = None
    assert rc(params=bad) == E
    bad = _params(a, b, 2)
    bad[1].imgB.topLeft = None
    assert rc(count=2, params=bad) == E
    for off in (1, 2, 3):
        bad = _params(a, b)
        bad[0].imgA.topLeft = a.ctypes.data + off                              # not 4-byte aligned
        assert rc(params=bad) == E
        bad = _params(a, b, 2)
        bad[1].imgB.topLeft = b.ctypes.data + off
        assert rc(count=2, params=bad) == E
        if not grad:
            bad = _params(a, b)
            bad[0].ssimMap = ga.ctypes.data + off
            assert rc(params=bad) == E
    for r in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert rc(r=r) == E
    if not fn.endswith("_host"):
        assert rc(ctx=None) == E                                               # these entries need a context
        assert rc(ctx=None, r=255.0) == E
    if grad:
        assert rc(grads=(None, None)) == E                                     # both gradient arrays NULL
        g = _grads(ga, 2)
        g[1].topLeft = None
        assert rc(count=2, grads=(g, None)) == E and rc(count=2, grads=(None, g)) == E
        g = _grads(ga)
        g[0].topLeft = ga.ctypes.data + 2
        assert rc(grads=(g, None)) == E and rc(grads=(_grads(ga), g)) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    if ssim_amd.device_count() > 0:
        v, _ = ssim_amd.compute_ssim3f(np.full((4, 8, 8), 0.25, np.float32), np.full((4, 8, 8), 0.25, np.float32), 1.0)
        assert abs(float(v) - 1.0) < 1e-6
        return
    a = np.zeros((6, 20, 30), np.float32)
    out = (ctypes.c_float * 1)()
    for r in (1.0, 255.0, 1000.0):
        assert lib.rmgr_ssim_hip_compute_ssim3f_host(None, 1, _params(a, a), r, out) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssim3f(a, a, 1.0)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssim3f_batch([(a, a), (a, a)], 1.0)


def test_make_params3f_takes_the_strides_of_any_view():
    base = np.zeros((5, 6, 14), np.float32)
    v = base[::-1, :, ::2].transpose(1, 0, 2)                                   # (6, 5, 7): negative and permuted strides, step 2
    p = ssim_amd.api._params3f_of(v, v)
    assert (p.width, p.height, p.depth) == (7, 5, 6)
    assert (p.imgA.step, p.imgA.stride, p.imgA.sliceStride) == (2, -6 * 14, 14)
    assert p.imgA.topLeft == v.ctypes.data and (p.ssimStep, p.ssimStride, p.ssimSliceStride) == (1, 7, 35)


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 1, 8, 16, 16)
    with pytest.raises(ValueError, match="GPU"):
        torch_ops.ssim3d(x, x)                                                 # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        torch_ops.SSIM3DLoss()(x, x)
    with pytest.raises(TypeError):
        torch_ops.ssim3d(x.double(), x.double())
    for t in (x.half(), x.bfloat16()):
        with pytest.raises(TypeError, match="float32 for now"):
            torch_ops.ssim3d(t, t)
        with pytest.raises(TypeError, match="float32 for now"):
            torch_ops.ssim3d(x, t)
    with pytest.raises(TypeError):
        torch_ops.ssim3d(x.numpy(), x.numpy())
    with pytest.raises(ValueError):
        torch_ops.ssim3d(x, torch.zeros(2, 1, 8, 16, 15))
    with pytest.raises(ValueError, match="D, H, W"):
        torch_ops.ssim3d(torch.zeros(16, 16), torch.zeros(16, 16))             # fewer than 3 dimensions
    with pytest.raises(ValueError):
        torch_ops.ssim3d(torch.zeros(2, 0, 4, 4), torch.zeros(2, 0, 4, 4))     # empty volumes
    for r in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            torch_ops.ssim3d(x, x, r)
    with pytest.raises(ValueError):
        torch_ops.SSIM3DLoss(reduction="sum")


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; "
                        "ssim_amd.torch_ops.SSIM3DLoss(); assert 'torch' not in sys.modules" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


WALK_KERNELS, ADJOINT_KERNELS = 4, 3        # value / dA / dB / both; dA / dB / both


def test_volume_kernels_never_spill_and_keep_their_occupancy():
    """Build-time guard, as tests/test_ssimk_cpu.py has for ssimk_kernels.hip: nothing spills, every kernel keeps at least two waves per
    SIMD and at most 64 KiB of LDS per workgroup, and the file holds the eight kernels DESIGN.md section 18 lists with the budgets it
    lists: the walks at most 112 VGPRs and 17504 B of LDS, the adjoint walks at most 168 VGPRs and 17472 B."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "ssim3f_kernels.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src), "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key in ("VGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]", "LDS Size \\[bytes/block\\]"):
            m = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if m and name:
                kernels[name][key.split(" ")[0]] = int(m.group(1))
    walk = {k: v for k, v in kernels.items() if "ssim3f_walk" in k}
    adjoint = {k: v for k, v in kernels.items() if "ssim3f_adjoint" in k}
    assert len(walk) == WALK_KERNELS and len(adjoint) == ADJOINT_KERNELS and len(kernels) == WALK_KERNELS + ADJOINT_KERNELS + 1, sorted(kernels)   # + the reduction
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2 and v["LDS"] <= 65536, (k, v)
    for k, v in walk.items():
        assert v["VGPRs"] <= 112 and v["Occupancy"] >= 4 and v["LDS"] <= 17504, (k, v)
    for k, v in adjoint.items():
        assert v["VGPRs"] <= 168 and v["Occupancy"] >= 3 and v["LDS"] <= 17472, (k, v)
