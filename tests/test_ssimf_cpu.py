"""CPU: SSIM of float32 samples and its gradient -- the definition and its boundaries (include/rmgr/ssim-hip.h, rmgr_ssim_hip_*_ssimf*).

  * the float64 model (tests/ssimf_model.py) with the double constants and the float64 Gaussian IS the reference's fp64 oracle, for the
    samples as they are at range 255 and, scale invariance, for a / 255, b / 255 at range 1;
  * the model's gradient is the derivative of the model's mean (central differences, corners, edges, a crop narrower than the window's
    half width and a 1 x 1 image), and Gt is the adjoint of G;
  * the fp32 emulation of the kernels stays inside the bounds tests/test_gpu_ssimf.py asserts;
  * the entry points are exported, every EINVAL comes before the device, a valid call without a device is ENODEV, and
    ssim_amd.torch_ops refuses what it documents before any GPU call;
  * the new kernels never spill.
"""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import ssimf_model as M
import ssim_amd
from conftest import ROOT, image_entries, load_pair

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_ssimf", "rmgr_ssim_hip_compute_ssimf_device", "rmgr_ssim_hip_compute_ssimf_host",
                "rmgr_ssim_hip_enqueue_ssimf_grad")

def test_model_is_the_reference_double_oracle_and_scale_invariant(oracle, manifest):
    g64 = M.gaussian_taps(f32=False)
    assert np.abs(M.gaussian_taps() - g64).max() < 1e-8
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        want, _, _ = oracle.ssim_naive_f64(a, b)
        got, _ = M.ssim(a, b, 255.0, *M.constants(255.0, f32=False), g=g64)
        assert abs(got - want) <= 1e-12, (n, got, want)
        unit, _ = M.ssim(a / 255.0, b / 255.0, 1.0, *M.constants(1.0, f32=False), g=g64)
        assert abs(unit - want) <= 1e-12, (n, unit, want)


def test_constants():
    assert M.constants(255.0) == (float(np.float32(6.5025)), float(np.float32(58.5225)))
    for r in (1.0, 255.0, 1000.0, 0.5):
        c1, c2 = M.constants(r, f32=False)
        assert c1 == (0.01 * r) * (0.01 * r) and c2 == (0.03 * r) * (0.03 * r)


def test_gt_is_the_adjoint_of_g():
    rng = np.random.default_rng(11)
    for shape in [(40, 48), (64, 3), (3, 7), (5, 1), (1, 1), (12, 4), (6, 6)]:
        u, v = rng.standard_normal(shape), rng.standard_normal(shape)
        lhs, rhs = float(np.sum(M.blur(u) * v)), float(np.sum(u * M.blur_t(v)))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (shape, lhs, rhs)
    # in the interior Gt is G; the end pixels collect what the forward pass clamped onto them: Gt 1 = the column sums of G
    t = M.blur_t(np.ones((1, 30)))
    s = M.gaussian_taps().sum()                      # the single row collects all eleven taps of its axis
    assert np.abs(t[0, 5:25] - s * s).max() < 1e-15 and t[0, 0] > 1.2 and abs(t.sum() - 30 * s * s) < 1e-12


def _fd_points(h, w, rng):
    pts = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1)}
    while len(pts) < min(14, h * w):
        pts.add((int(rng.integers(0, h)), int(rng.integers(0, w))))
    return sorted(pts)


def test_gradient_is_the_derivative_of_the_mean(manifest):
    """Central differences of the model's own mean at step 1e-5 (range 1) agree with grad() within 1e-7 of the plane's largest
    gradient magnitude; measured 7e-9 at 1e-5 and 2e-9 at 5e-6 -- halving the step does not change the verdict."""
    rng = np.random.default_rng(5)
    crops = []
    for n, (y0, x0, h, w) in (("einstein_jpg", (0, 0, 40, 48)), ("einstein_blur", (100, 60, 40, 48)), ("bbb257x65_q50_ch1", (25, 209, 40, 48)),
                              ("einstein_contrast", (216, 208, 40, 48)), ("einstein_jpg", (30, 30, 20, 4)), ("einstein_blur", (7, 9, 3, 5)),
                              ("einstein_jpg", (50, 50, 1, 1))):
        a, b = load_pair(manifest[n])
        crops.append((n, a[y0:y0 + h, x0:x0 + w] / 255.0, b[y0:y0 + h, x0:x0 + w] / 255.0))
    for n, a, b in crops:
        assert a.shape == b.shape and a.size > 0
        g_out = -0.75
        ga, gb = M.grad(a, b, 1.0, g_out)
        for which, gr in ((0, ga), (1, gb)):
            scale = np.abs(gr).max()
            for eps in (1e-5, 5e-6):
                for (y, x) in _fd_points(a.shape[0], a.shape[1], rng):
                    p, m = [a.copy(), b.copy()], [a.copy(), b.copy()]
                    p[which][y, x] += eps
                    m[which][y, x] -= eps
                    fd = g_out * (M.ssim(p[0], p[1], 1.0)[0] - M.ssim(m[0], m[1], 1.0)[0]) / (2 * eps)
                    assert abs(fd - gr[y, x]) <= 1e-7 * scale, (n, a.shape, which, y, x, eps, fd, gr[y, x])


def test_fp32_emulation_is_inside_the_gpu_bounds(manifest):
    """emulate_fp32 against the float64 model on every golden pair in the three forms (/ 255 at range 1, as stored at range 255, scaled
    by a non-integer factor to range 1000), every pixel, value, map and both gradients.  Measured: 2.38e-4 per pixel, 1.17e-6 global,
    8.37e-5 of the plane's largest float64 gradient magnitude; the pair of identical images (exact gradient 0) apart: max|grad| * W * H
    * R = 3.65e-4 (the gradient scales with 1 / R; at range 1 this is max|grad| * W * H).  tests/test_gpu_ssimf.py asserts about twice
    these: 5e-4, 2.5e-6, 1.7e-4 and 7.5e-4 -- the margin covers the order of the fp64 sum, the 1-ulp reciprocal and fma contraction,
    which the emulation does not restate."""
    worst_px = worst_g = worst_grad = worst_ident = 0.0
    identical = 0
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        for form, fa, fb, r in M.forms(a, b):
            gv, gm = M.ssim(fa, fb, r)
            ev, em, ea, eb = M.emulate_fp32(fa, fb, r, 1.0)
            worst_px = max(worst_px, float(np.abs(em - gm).max()))
            worst_g = max(worst_g, abs(ev - gv))
            ga, gb = M.grad(fa, fb, r, 1.0)
            for e, g in ((ea, ga), (eb, gb)):
                if np.array_equal(a, b):
                    assert np.abs(g).max() < 1e-15 / r
                    identical += 1
                    worst_ident = max(worst_ident, float(np.abs(e).max()) * fa.size * r)
                else:
                    worst_grad = max(worst_grad, float(np.abs(e - g).max() / np.abs(g).max()))
    assert identical == 6       # einstein_einstein, both gradients, three forms
    print("emulation: px %.3g global %.3g grad %.3g identical %.3g" % (worst_px, worst_g, worst_grad, worst_ident))
    assert worst_px <= M.EMU_PX and worst_g <= M.EMU_G and worst_grad <= M.EMU_GRAD and worst_ident <= M.EMU_IDENT, (worst_px, worst_g, worst_grad, worst_ident)
    # pinned from below as well: a figure that moved far away means the emulation no longer restates these kernels
    assert worst_px >= M.EMU_PX / 2 and worst_g >= M.EMU_G / 2 and worst_grad >= M.EMU_GRAD / 2 and worst_ident >= M.EMU_IDENT / 2
    for tol, emu in ((M.PX_TOL, M.EMU_PX), (M.G_TOL, M.EMU_G), (M.GRAD_TOL, M.EMU_GRAD), (M.IDENT_TOL, M.EMU_IDENT)):
        assert 1.9 <= tol / emu <= 2.2


def test_centres_are_per_strip_column_and_bounded_by_the_range():
    img = np.arange(7 * 300, dtype=np.float32).reshape(7, 300)
    assert list(M.centres(img, 4000.0)) == [img[3, 64], img[3, 192], img[3, 299]]
    assert list(M.centres(img, 1000.0)) == [img[3, 64], 0.0, 0.0]
    img[3, 64] = np.nan
    assert list(M.centres(img, 4000.0)) == [0.0, img[3, 192], img[3, 299]]


def test_adjoint_weights_sum_like_the_clamped_window():
    g = M.gaussian_taps().astype(np.float32)[5:]
    for n in (1, 2, 4, 5, 6, 11, 40):
        w = M.adjoint_weights(n, g).astype(np.float64)
        # column q of the dense adjoint: weight of v(p) in out(q), p = q + j
        dense = np.zeros((n, n))
        for j in range(-5, 6):
            for q in range(n):
                if 0 <= q + j < n:
                    dense[q, q + j] += w[j + 5, q]
        want = np.zeros((n, n))
        for p in range(n):
            for t in range(-5, 6):
                want[min(max(p + t, 0), n - 1), p] += float(g[abs(t)])
        assert np.abs(dense - want).max() < 1e-7, n


# ---- the C ABI's validation (no device needed) ----

def _params(a, b, n=1, **over):
    ps = (ssim_amd.ParamsF * n)()
    h, w = a.shape
    for i in range(n):
        ps[i] = ssim_amd.make_params_f(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w)
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _grads(a, n=1):
    gs = (ssim_amd.GradF * n)()
    for i in range(n):
        gs[i] = ssim_amd.GradF(a.ctypes.data, 1, a.shape[1])
    return gs


def test_entry_points_are_exported(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS
    for name in ("ImgF", "ParamsF", "GradF", "make_params_f", "compute_ssimf", "compute_ssimf_batch"):
        assert hasattr(ssim_amd, name)
    for name in ("ssimf_device", "enqueue_ssimf", "enqueue_ssimf_grad"):
        assert hasattr(ssim_amd.Context, name)
    assert lib.rmgr_ssim_hip_get_abi_version() == 6


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    a = np.zeros((20, 30), np.float32)
    b = np.zeros((20, 30), np.float32)
    ga = np.zeros((20, 30), np.float32)
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
    assert rc(params=_params(a, b, width=0)) == E
    assert rc(params=_params(a, b, height=0)) == E
    assert rc(params=_params(a, b, width=0x7FFF0001)) == E                     # above the kernels' limit
    two = _params(a, b, 2)
    two[1].width = 29
    assert rc(count=2, params=two) == E                                        # sizes differ
    two = _params(a, b, 2)
    two[1].height = 19
    assert rc(count=2, params=two) == E
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
        v, _ = ssim_amd.compute_ssimf(np.full((8, 8), 0.25, np.float32), np.full((8, 8), 0.25, np.float32), 1.0)
        assert abs(float(v) - 1.0) < 1e-6
        return
    a = np.zeros((20, 30), np.float32)
    out = (ctypes.c_float * 1)()
    for r in (1.0, 255.0, 1000.0):
        assert lib.rmgr_ssim_hip_compute_ssimf_host(None, 1, _params(a, a), r, out) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssimf(a, a, 1.0)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssimf_batch([(a, a), (a, a)], 1.0)


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError):
        torch_ops.ssim(x, x)                                                   # CPU tensors
    with pytest.raises(ValueError):
        torch_ops.SSIMLoss()(x, x)
    with pytest.raises(TypeError):
        torch_ops.ssim(x.double(), x.double())
    with pytest.raises(TypeError):
        torch_ops.ssim(x, x.half())
    with pytest.raises(TypeError):
        torch_ops.ssim(x.numpy(), x.numpy())
    with pytest.raises(ValueError):
        torch_ops.ssim(x, torch.zeros(2, 3, 16, 15))
    with pytest.raises(ValueError):
        torch_ops.ssim(torch.zeros(16), torch.zeros(16))
    with pytest.raises(ValueError):
        torch_ops.SSIMLoss(reduction="sum")


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; assert 'torch' not in sys.modules" % ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_float_kernels_never_spill_and_keep_their_occupancy():
    """Build-time guard, as tests/test_abi_cpu.py has for ssim_kernels.hip: the forward strip kernels keep three waves per SIMD (the
    ssim16 budget: at most 168 VGPRs, LDS for 12 waves per CU), the gradient kernel two workgroups of 256 lanes per CU (at most 128 VGPRs,
    at most 64 KiB of the CU's 160 KiB of LDS per workgroup), and nothing spills."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "ssimf_kernels.hip")
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
    strip = {k: v for k, v in kernels.items() if "ssimf_strip" in k}
    grad = {k: v for k, v in kernels.items() if "ssimf_grad" in k}
    assert len(strip) == 5 and len(grad) == 3 and len(kernels) == 9, sorted(kernels)       # + the reduction
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in strip.items():
        assert v["VGPRs"] <= 168 and v["Occupancy"] >= 3 and v["LDS"] <= 13312, (k, v)
    for k, v in grad.items():
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 2 and v["LDS"] <= 65536, (k, v)
