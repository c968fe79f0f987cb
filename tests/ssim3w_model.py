"""float64 model of the gradient of the 3-D SSIM MAP for a per-voxel upstream gradient (the definition in include/rmgr/ssim-hip.h,
rmgr_ssim_hip_enqueue_ssim3f_map_grad), and an fp32 emulation of the kernels behind it (ssim3w_kernels.hip's walk, then ssim3f_kernels.hip's
adjoint walk).

The yardstick of tests/test_ssim3w_cpu.py and tests/test_gpu_ssim3w.py.  Volumes are (D, H, W) arrays.  Built on ssim3f_model: its blur G,
its adjoint Gt and its five statistics; the one change is that k is a volume and sits INSIDE Gt:

    dLoss/da = Gt(k d_mu_a) + 2 a Gt(k d_aa) + b Gt(k d_ab),        k(p) = gMap(p) = dLoss/dssim(p), no division by W H D.

emulate_fp32_map_grad() is ssim3f_model.emulate_fp32's gradient half with k a float32 volume: the same centre, statistics, derivative and
adjoint gathers, operation by operation, and the plain fp32 product k(p) d(p).  With the constant volume of the header's identity clause it
gives ssim3f_model.emulate_fp32's gradients bit for bit.
"""
import numpy as np

import ssim3f_model as S
from ssim3f_model import F, FIXTURES, FORMS  # noqa: F401  (re-exported for the tests)

# What emulate_fp32_map_grad measures against grad_map, the worst over FIXTURES x FORMS x weight_volumes(): the gradient error over the
# volume's largest float64 gradient magnitude (tests/test_ssim3w_cpu.py pins the figure from both sides).  Measured 3.04e-4: dLoss/db of
# bbb255x63_q50_ch1 raw under the standard-normal weights, whose signs cancel inside Gt; the masked uniform weights measure 1.74e-4, the
# one-hot 4.04e-5, and the uniform k of ssim3f 9.45e-5 on the same volumes.  The GPU tests assert twice it: the project's standing margin
# for the 1-ulp reciprocal, which the emulation does not restate.
EMU_GRAD = 3.1e-4
TOL_FACTOR = 2.0


def tolerances():
    """GRAD_TOL: twice EMU_GRAD."""
    return TOL_FACTOR * EMU_GRAD


def one_hot(shape, z, y, x):
    d, h, w = shape
    p = np.zeros(shape, F)
    p[min(z, d - 1), min(y, h - 1), min(x, w - 1)] = 1
    return p


def weight_volumes(shape, seed=0):
    """The three weight volumes the emulation and the GPU are measured with: (name, float32 volume).  Seeded standard normal; seeded
    uniform [0, 1) under a 0 / 1 mask of about half the voxels; one-hot at (z, y, x) = (D // 2, 15, 15) (the last column of the first
    tile), clipped into the volume."""
    rng = np.random.default_rng(3000 + seed)
    yield "normal", rng.standard_normal(shape).astype(F)
    yield "masked", (rng.random(shape, dtype=F) * (rng.random(shape) < 0.5)).astype(F)
    yield "one-hot", one_hot(shape, shape[0] // 2, 15, 15)


def constant_volume(g_out, shape):
    """The volume of the header's identity clause: every element float(double(gOut) / (double(W) * double(H) * double(D)))."""
    return np.full(shape, F(float(F(g_out)) / S.voxels(shape)), F)


def grad_map(a, b, data_range, gmap, g=None):
    """(dLoss/da, dLoss/db) in float64 for dLoss/dssim(p) = gmap(p): the header's formulas, k = gmap inside Gt."""
    c1, c2 = S.constants(data_range)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    k = np.asarray(gmap, np.float64)
    assert k.shape == a.shape
    ma, mb, A1, A2, B1, B2 = S._terms(a, b, c1, c2, g)
    s = A1 * A2 / (B1 * B2)
    d_ab = 2.0 * A1 / (B1 * B2)
    d_aa = -s / B2
    d_mu_a = 2.0 * mb * A2 / (B1 * B2) - 2.0 * ma * s / B1 - 2.0 * ma * d_aa - mb * d_ab
    d_mu_b = 2.0 * ma * A2 / (B1 * B2) - 2.0 * mb * s / B1 - 2.0 * mb * d_aa - ma * d_ab
    t_aa, t_ab = S.blur_t(k * d_aa, g), S.blur_t(k * d_ab, g)
    return S.blur_t(k * d_mu_a, g) + 2.0 * a * t_aa + b * t_ab, S.blur_t(k * d_mu_b, g) + 2.0 * b * t_aa + a * t_ab


# ---- fp32 emulation of ssim3w_kernels.hip + the adjoint walk of ssim3f_kernels.hip ----------------------------------------------


def derivatives_fp32(a, b, data_range):
    """What the walk computes per voxel before it weights it, as ssim3f_model.emulate_fp32 does: (d_mu_a, d_mu_b, d_aa, d_ab, a', b'), the
    centred samples on the volume itself."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    D, H, W = a.shape
    c1, c2 = (F(x) for x in S.constants(data_range))
    g = S.gaussian_taps().astype(F)[5:]          # centre .. edge
    cA, cB = S.centre(a, data_range), S.centre(b, data_range)
    two = F(2.0)
    with np.errstate(all="ignore"):
        sa = (np.pad(a, 5, mode="edge") - cA).astype(F)
        sb = (np.pad(b, 5, mode="edge") - cB).astype(F)
        qs = S._fma32(sb, sb, (sa * sa).astype(F))                             # fma(b', b', a'^2)
        x = (sa * sb).astype(F)
        mA, mB, eS, eX = S._blur32(sa, g), S._blur32(sb, g), S._blur32(qs, g), S._blur32(x, g)
        pc = (mA * mB).astype(F)
        tc = ((mA * mA).astype(F) + (mB * mB).astype(F)).astype(F)
        sS = (eS - tc).astype(F)
        sAB = (eX - pc).astype(F)
        uA, uB = (mA + cA).astype(F), (mB + cB).astype(F)
        muAB = (uA * uB).astype(F)
        tm = ((uA * uA).astype(F) + (uB * uB).astype(F)).astype(F)
        A1, A2 = S._fma32(muAB, two, np.full_like(muAB, c1)), S._fma32(sAB, two, np.full_like(sAB, c2))
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
        ca, cb = sa[5:5 + D, 5:5 + H, 5:5 + W], sb[5:5 + D, 5:5 + H, 5:5 + W]
        return d_mu(uB, uA, mA, mB), d_mu(uA, uB, mB, mA), daa, dab, ca, cb


def apply_fp32(derivatives, gmap):
    """The rest of the backward for one weight volume: k(p) d(p) as plain fp32 products, the adjoint gathers on x, then y, then z, and the
    gradient in the centred variables.  (dLoss/da, dLoss/db) as float32."""
    dmA, dmB, daa, dab, ca, cb = derivatives
    k = np.asarray(gmap, F)
    D, H, W = ca.shape
    assert k.shape == (D, H, W)
    g = S.gaussian_taps().astype(F)[5:]
    wx, wy, wz = S.adjoint_weights(W, g), S.adjoint_weights(H, g), S.adjoint_weights(D, g)
    two = F(2.0)
    with np.errstate(all="ignore"):
        def gt(v):
            return S._adjoint32(S._adjoint32(S._adjoint32((k * v).astype(F), wx, 2), wy, 1), wz, 0)
        r_a, r_b, r_aa, r_ab = gt(dmA), gt(dmB), gt(daa), gt(dab)
        ga = ((r_a + ((two * ca).astype(F) * r_aa).astype(F)).astype(F) + (cb * r_ab).astype(F)).astype(F)
        gb = ((r_b + ((two * cb).astype(F) * r_aa).astype(F)).astype(F) + (ca * r_ab).astype(F)).astype(F)
    return ga, gb


def emulate_fp32_map_grad(a, b, data_range, gmap):
    """(dLoss/da, dLoss/db) as float32, as the two walks compute them."""
    return apply_fp32(derivatives_fp32(a, b, data_range), gmap)


def measure(manifest, fixtures=FIXTURES):
    """The worst gradient error of emulate_fp32_map_grad over the volume's largest float64 gradient magnitude, across fixtures x FORMS x
    weight_volumes (fixed seeds: the fixture's index)."""
    worst = 0.0
    for seed, name in enumerate(fixtures):
        for _, fa, fb, r in S.fixture_forms(manifest, name):
            der = derivatives_fp32(fa, fb, r)
            for _, k in weight_volumes(fa.shape, seed):
                for e, w in zip(apply_fp32(der, k), grad_map(fa, fb, r, k)):
                    worst = max(worst, float(np.abs(e - w).max() / np.abs(w).max()))
    return worst
