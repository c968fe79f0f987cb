"""float64 model of the gradient of the SSIM MAP for a per-pixel upstream gradient (the definition in include/rmgr/ssim-hip.h,
rmgr_ssim_hip_enqueue_ssimf_map_grad / _ssimh_map_grad), on top of tests/ssimf_model.py, which stays as it is.

The yardstick of tests/test_ssimw_cpu.py and tests/test_gpu_ssimw.py: grad_map() is ssimf_model.grad() with the uniform k = gOut / (W H)
replaced by the plane k(p) = gMap(p), INSIDE the adjoint Gt: the derivative of sum_p gMap(p) ssim(p).

emulate_fp32_map_grad() restates the KERNEL's arithmetic (ssimw_kernels.hip: grad_body of ssim2_walk.h with the per-pixel k): the gradient half of ssimf_model.emulate_fp32, statement for
statement, with the plane k.  With the constant plane float(gOut / (W H)) it reproduces emulate_fp32's gradients bit for bit.
"""
import numpy as np

import ssimf_model as M
from ssimf_model import F, STRIP_W, _adjoint32, _blur32, _fma32

# What the fp32 emulation below measures against grad_map(), the worst over every golden pair in the three forms of ssimf_model.forms()
# and the three weight planes of weight_planes() (tests/test_ssimw_cpu.py pins the figures): the gradient error over the plane's
# largest float64 gradient magnitude, and, where the exact gradient is 0 (is_null() below), max|grad| * R / max|gMap|.  The GPU tests
# assert about twice these: the margin covers the reciprocal's last ulp and fma contraction, which the emulation does not restate.
EMU_WGRAD, EMU_WIDENT = 1.07e-4, 9.0e-5
WGRAD_TOL, WIDENT_TOL = 2.1e-4, 1.8e-4


def is_null(grad64, gmap, data_range):
    """The exact gradient is 0 up to float64 rounding: the images agree wherever a window reaches a non-zero weight (the pair of
    identical images under any plane; a one-hot weight in an area the distortion left alone).  max|grad| R / max|gMap| is of order 1
    otherwise; the relative error has no meaning here and the absolute figure EMU_WIDENT takes its place."""
    return float(np.abs(grad64).max()) * float(data_range) <= 1e-9 * float(np.abs(gmap).max())


def weight_planes(h, w, seed=0):
    """The three weight planes the emulation and the GPU are measured with: (name, float32 plane).  Seeded standard normal; seeded uniform
    [0, 1) under a 0 / 1 mask of about half the pixels; one-hot at (31, 31) (the last pixel of the first tile), clipped into the plane."""
    rng = np.random.default_rng(1000 + seed)
    yield "normal", rng.standard_normal((h, w)).astype(F)
    yield "masked", (rng.random((h, w), dtype=F) * (rng.random((h, w)) < 0.5)).astype(F)
    yield "one-hot", one_hot(h, w, 31, 31)


def one_hot(h, w, y, x):
    p = np.zeros((h, w), F)
    p[min(y, h - 1), min(x, w - 1)] = 1
    return p


def constant_plane(g_out, h, w):
    """The plane of the header's identity clause: every element float(double(gOut) / (double(W) * double(H)))."""
    return np.full((h, w), F(float(F(g_out)) / (float(w) * float(h))), F)


def grad_map(a, b, data_range, gmap, c1=None, c2=None, g=None):
    """(dLoss/da, dLoss/db) in float64 for dLoss/dssim(p) = gmap(p): the header's formulas, k = gmap inside Gt."""
    if c1 is None:
        c1, c2 = M.constants(data_range)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    k = np.asarray(gmap, np.float64)
    assert k.shape == a.shape == b.shape
    ma, mb, A1, A2, B1, B2 = M._terms(a, b, c1, c2, g)
    s = A1 * A2 / (B1 * B2)
    d_ab = 2.0 * A1 / (B1 * B2)
    d_aa = -s / B2
    d_mu_a = 2.0 * mb * A2 / (B1 * B2) - 2.0 * ma * s / B1 - 2.0 * ma * d_aa - mb * d_ab
    d_mu_b = 2.0 * ma * A2 / (B1 * B2) - 2.0 * mb * s / B1 - 2.0 * mb * d_aa - ma * d_ab
    t_aa, t_ab = M.blur_t(k * d_aa, g), M.blur_t(k * d_ab, g)
    return M.blur_t(k * d_mu_a, g) + 2.0 * a * t_aa + b * t_ab, M.blur_t(k * d_mu_b, g) + 2.0 * b * t_aa + a * t_ab


def emulate_fp32_map_grad(a, b, data_range, gmap):
    """(dLoss/da, dLoss/db) as float32, as ssimw_grad_kernel computes them, strip column by strip column: ssimf_model.emulate_fp32's
    gradient half with k a float32 plane."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    k = np.asarray(gmap, F)
    H, W = a.shape
    assert k.shape == (H, W)
    c1, c2 = (F(x) for x in M.constants(data_range))
    g = M.gaussian_taps().astype(F)[5:]          # centre .. edge
    cA, cB = M.centres(a, data_range), M.centres(b, data_range)
    pa, pb = np.pad(a, 5, mode="edge"), np.pad(b, 5, mode="edge")
    ga, gb = np.empty((H, W), F), np.empty((H, W), F)
    wx, wy = M.adjoint_weights(W, g), M.adjoint_weights(H, g)
    two = F(2.0)
    with np.errstate(all="ignore"):
        for i, x0 in enumerate(range(0, W, STRIP_W)):
            x1 = min(x0 + STRIP_W, W)
            # the statistics 5 columns beyond the strip column, under its centre: the whole width is blurred with this centre
            sa = (pa - cA[i]).astype(F)
            sb = (pb - cB[i]).astype(F)
            aa = (sa * sa).astype(F)
            qs = _fma32(sb, sb, aa)                                          # fma(b', b', a'^2)
            x = (sa * sb).astype(F)
            mA, mB, eS, eX = _blur32(sa, g), _blur32(sb, g), _blur32(qs, g), _blur32(x, g)
            pc = (mA * mB).astype(F)
            tc = ((mA * mA).astype(F) + (mB * mB).astype(F)).astype(F)
            sS = (eS - tc).astype(F)
            sAB = (eX - pc).astype(F)
            uA, uB = (mA + cA[i]).astype(F), (mB + cB[i]).astype(F)
            muAB = (uA * uB).astype(F)
            tm = ((uA * uA).astype(F) + (uB * uB).astype(F)).astype(F)
            A1, A2 = _fma32(muAB, two, np.full_like(muAB, c1)), _fma32(sAB, two, np.full_like(sAB, c2))
            B1, B2 = (tm + c1).astype(F), (sS + c2).astype(F)
            n = (A1 * A2).astype(F)
            r1, r2 = (F(1.0) / B1).astype(F), (F(1.0) / B2).astype(F)
            r12 = (r1 * r2).astype(F)
            s = (n * r12).astype(F)
            dab = ((two * A1).astype(F) * r12).astype(F)
            daa = -(s * r2).astype(F)
            f1, f2 = (A2 * r12).astype(F), (s * r1).astype(F)

            def d_mu(u_other, u_self, m_self, m_other):
                t = ((two * u_other).astype(F) * f1).astype(F) - ((two * u_self).astype(F) * f2).astype(F)
                t = t.astype(F) - ((two * m_self).astype(F) * daa).astype(F)
                return (t.astype(F) - (m_other * dab).astype(F)).astype(F)

            def gt(v):
                return _adjoint32(_adjoint32((k * v).astype(F), wx, 1), wy, 0)
            r_a, r_b, r_aa, r_ab = gt(d_mu(uB, uA, mA, mB)), gt(d_mu(uA, uB, mB, mA)), gt(daa), gt(dab)
            ca, cb = sa[5:5 + H, 5:5 + W], sb[5:5 + H, 5:5 + W]              # a', b' at the pixel
            va = ((r_a + ((two * ca).astype(F) * r_aa).astype(F)).astype(F) + (cb * r_ab).astype(F)).astype(F)
            vb = ((r_b + ((two * cb).astype(F) * r_aa).astype(F)).astype(F) + (ca * r_ab).astype(F)).astype(F)
            ga[:, x0:x1], gb[:, x0:x1] = va[:, x0:x1], vb[:, x0:x1]
    return ga, gb
