"""CPU: multi-scale SSIM's definition and its C ABI boundary (include/rmgr/ssim-hip.h, rmgr_ssim_hip_compute_msssim_*).

  * the float64 model (tests/msssim_model.py) at one scale IS the reference's SSIM: it equals the reference's own fp64 oracle
    (oracle.ssim_naive_f64: the normalised 121-tap Gaussian with clamped borders, which is the product of two normalised 1-D
    Gaussians, so the separable model agrees to rounding) on the golden fixtures;
  * the clamped 2 x 2 pyramid is exact in fp32 at every scale, whatever the size (odd, 1 x N, N x 1, 1 x 1);
  * every EINVAL of the two entry points comes before any device is touched;
  * `rmgr-ssim -m` with a map argument is refused while the arguments are parsed.
"""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import msssim_model as M
import ssim_amd
from conftest import ROOT, image_entries, load_pair

CLI = os.environ.get("RMGR_SSIM_CLI") or os.path.join(ROOT, "ssim_amd", "bin", "rmgr-ssim")


def test_model_at_one_scale_is_the_reference_double_oracle(oracle, manifest):
    names = [n for n in image_entries(manifest) if n.startswith(("bbb255x63", "bbb257x65", "einstein"))]
    assert len(names) == 18
    for n in names:
        a, b = load_pair(manifest[n])
        want, _, _ = oracle.ssim_naive_f64(a, b)
        got, means = M.msssim(a, b, scales=1, weights=[1.0], c1=M.C1_F64, c2=M.C2_F64)
        assert abs(got - want) <= 1e-9, (n, got, want)
        assert abs(means[0][1] - want) <= 1e-9, n


def test_model_taps_are_the_engines():
    g = M.gaussian_taps()
    assert abs(g.sum() - 1.0) < 1e-15 and np.allclose(g, g[::-1])
    # outer product of the 1-D taps = the normalised 2-D Gaussian of the reference's oracle
    i = np.arange(-5, 6, dtype=np.float64)
    k2 = np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2 * 1.5 * 1.5))
    assert np.abs(np.outer(g, g) - k2 / k2.sum()).max() < 1e-17


@pytest.mark.parametrize("shape", [(63, 255), (65, 257), (1, 1), (1, 37), (37, 1), (1, 1000), (999, 3), (129, 131)])
def test_pyramid_is_exact_in_fp32(shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, shape).astype(np.uint8)
    img[0, 0], img[-1, -1] = 255, 0
    p64 = M.pyramid(img, M.MAX_SCALES)
    p32 = img.astype(np.float32)
    h, w = shape
    for s in range(M.MAX_SCALES):
        assert p64[s].shape == (h, w), (s, p64[s].shape)
        assert np.array_equal(p32.astype(np.float64), p64[s]), s          # fp32 arithmetic == float64 arithmetic, bit for bit
        q = p64[s] * 4.0 ** s
        assert np.array_equal(q, np.round(q)) and p64[s].min() >= 0 and p64[s].max() <= 255
        # the fp32 step written exactly as the kernel does it
        hh, ww = p32.shape
        y0 = np.minimum(2 * np.arange((hh + 1) // 2), hh - 1); y1 = np.minimum(y0 + 1, hh - 1)
        x0 = np.minimum(2 * np.arange((ww + 1) // 2), ww - 1); x1 = np.minimum(x0 + 1, ww - 1)
        p32 = ((p32[np.ix_(y0, x0)] + p32[np.ix_(y0, x1)]) + (p32[np.ix_(y1, x0)] + p32[np.ix_(y1, x1)])) * np.float32(0.25)
        assert p32.dtype == np.float32
        h, w = (h + 1) // 2, (w + 1) // 2


def test_model_on_identical_images_is_one():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (40, 70)).astype(np.uint8)
    v, means = M.msssim(a, a)
    assert abs(v - 1.0) < 1e-12 and np.abs(means - 1.0).max() < 1e-12


def test_model_relu_keeps_negative_means_from_nan():
    assert M.combine(np.array([[-0.2, -0.1], [0.5, 0.4]]), [0.5, 0.5]) == 0.0
    assert M.combine(np.array([[-0.2, -0.1], [0.5, 0.4]]), [0.0, 1.0]) == 0.4


# ---- the C ABI's validation (no device needed) ----

def _params(a, b, n=1, **over):
    ps = (ssim_amd.Params * n)()
    h, w = a.shape
    for i in range(n):
        ps[i] = ssim_amd.make_params(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w)
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _call(lib, fn, ctx, count, params, scales, weights, out):
    w = (ctypes.c_double * len(weights))(*weights) if weights is not None else None
    return getattr(lib, fn)(ctx, count, params, scales, w, out, None)


def test_entry_points_are_exported(lib):
    for name in ("rmgr_ssim_hip_compute_msssim_device", "rmgr_ssim_hip_compute_msssim_host"):
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS


@pytest.mark.parametrize("fn", ["rmgr_ssim_hip_compute_msssim_host", "rmgr_ssim_hip_compute_msssim_device"])
def test_every_einval_comes_before_the_device(lib, fn):
    a = np.zeros((20, 30), np.uint8)
    b = np.zeros((20, 30), np.uint8)
    out = (ctypes.c_float * 4)()
    fake_ctx = None if fn.endswith("_host") else ctypes.c_void_p(1)       # never dereferenced: validation comes first
    E = errno.EINVAL

    def rc(count=1, params=None, scales=5, weights=None, o=out, ctx=fake_ctx):
        return _call(lib, fn, ctx, count, _params(a, b, max(count, 1)) if params is None else params, scales, weights, o)
    assert rc(count=0) == E
    assert getattr(lib, fn)(fake_ctx, 1, None, 5, None, out, None) == E            # params NULL
    assert rc(o=None) == E                                                         # msssim NULL
    assert rc(params=_params(a, b, width=0)) == E
    assert rc(params=_params(a, b, height=0)) == E
    two = _params(a, b, 2)
    two[1].width = 29
    assert rc(count=2, params=two) == E                                            # sizes differ
    two = _params(a, b, 2)
    two[1].height = 19
    assert rc(count=2, params=two) == E
    bad = _params(a, b)
    bad[0].imgA.topLeft = None
    assert rc(params=bad) == E
    bad = _params(a, b, 2)
    bad[1].imgB.topLeft = None
    assert rc(count=2, params=bad) == E
    m = np.zeros((20, 30), np.float32)
    assert rc(params=_params(a, b, ssimMap=m.ctypes.data)) == E                    # no per-pixel map
    assert rc(scales=0) == E
    assert rc(scales=9) == E
    assert rc(scales=0, weights=[]) == E
    assert rc(scales=9, weights=[0.1] * 9) == E
    for s in (1, 2, 3, 4, 6, 7, 8):
        assert rc(scales=s) == E                                                   # Wang's weights are for five scales
    assert rc(scales=2, weights=[0.5, -0.1]) == E
    assert rc(scales=2, weights=[0.5, float("nan")]) == E
    assert rc(scales=2, weights=[float("inf"), 0.5]) == E
    if fn.endswith("_device"):
        assert rc(ctx=None) == E                                                   # the device entry needs a context
        assert rc(ctx=None, scales=2, weights=[0.5, 0.5]) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    if ssim_amd.device_count() > 0:
        v = ssim_amd.compute_msssim(np.full((8, 8), 7, np.uint8), np.full((8, 8), 7, np.uint8))
        assert abs(float(v) - 1.0) < 1e-6
        return
    a = np.zeros((20, 30), np.uint8)
    out = (ctypes.c_float * 1)()
    assert _call(lib, "rmgr_ssim_hip_compute_msssim_host", None, 1, _params(a, a), 5, None, out) == errno.ENODEV
    assert _call(lib, "rmgr_ssim_hip_compute_msssim_host", None, 1, _params(a, a), 2, [0.3, 0.7], out) == errno.ENODEV


# ---- the command-line tool ----

def test_cli_refuses_a_map_with_msssim_before_touching_anything(tmp_path):
    r = subprocess.run([CLI, "-m", str(tmp_path / "missing_a.ppm"), str(tmp_path / "missing_b.ppm"), str(tmp_path / "map.pgm")],
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "no per-pixel map" in r.stderr
    assert "Failed to open" not in r.stderr and "device" not in r.stderr           # refused while parsing: no file read, no GPU
    assert not (tmp_path / "map.pgm").exists()


def test_cli_help_names_msssim():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("Usage: rmgr-ssim [options] img1 img2 [map]")
    assert "  -m  " in r.stdout
