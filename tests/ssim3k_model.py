"""float64 model of the library's SSIM of float32 VOLUMES under a caller-chosen window, of its gradient and of the gradient of its map
(the definition in include/rmgr/ssim-hip.h, rmgr_ssim_hip_*_ssim3f_win*), and an fp32 emulation of the kernels behind them.

The yardstick of tests/test_ssim3k_cpu.py and tests/test_gpu_ssim3k.py.  It is ssim3f_model / ssim3w_model generalised to the taps
g[0 .. R] of a window (size, sigma, kind) -- the vocabulary and the taps of ssimk_model, the same window on all three axes: volumes are
(D, H, W) arrays, C1 / C2 from the data range, the clamped separable blur G over x, y and z, the SSIM formula per voxel, the fp64 mean over
double(W) * double(H) * double(D), and the exact derivative with Gt, the ADJOINT of the clamped window, built as defined: a scatter-add
of w_t v(p) onto clamp(p + t), one axis after the other.  The upstream gradient is a scalar (k = g_out / (W H D)) or a volume (k = gmap),
in both cases INSIDE Gt.  Plain numpy, no reference to the GPU code.

emulate_fp32() restates the KERNELS' arithmetic (ssim3k_kernels.hip for R = 1 .. 4; ssim3f_kernels.hip / ssim3w_kernels.hip with the
window's taps for R = 5) operation by operation: ONE centre per volume, fp32 volumes, the x pass centre tap first on folded sums, the y
pass and the z pass in source order with the first product plain, fma where the kernels fuse, the plain fp32 product k(p) d(p), the
adjoint as a weighted gather on x, then y, then z: what the GPU should produce up to the order of the fp64 sum and the 1-ulp reciprocal.
"""
import numpy as np

import ssim3f_model as S
import ssim3w_model as W3
import ssimk_model as K
from ssim3f_model import F, FIXTURES, FORMS, centre, constants, fixture_forms, golden_volume, voxels  # noqa: F401  (re-exported)
from ssimk_model import DEFAULT, WINDOWS, adjoint_weights, name_of, radius, taps  # noqa: F401  (re-exported)
from ssimf_model import _fma32

# What the fp32 emulation below measures against the float64 model, per window the worst over FIXTURES x FORMS (tests/test_ssim3k_cpu.py
# pins the figures from both sides): per voxel, global, gradient error over the volume's largest float64 gradient magnitude for the scalar
# upstream form, max|grad| * W * H * D * R on the pair of identical volumes (exact gradient 0), and the gradient error of the map gradient,
# the worst over the three weight volumes of ssim3w_model.  The GPU tests assert twice these: the project's standing margin for the 1-ulp
# reciprocal and the order of the fp64 sum, which the emulation does not restate.
EMU = {
    # window: (EMU_PX, EMU_G, EMU_GRAD, EMU_IDENT, EMU_MAPGRAD)
    (3, 0.0, 'uniform'): (4.0e-04, 1.2e-05, 1.0e-04, 4.1e-04, 2.3e-04),
    (5, 0.8, 'gaussian'): (5.0e-04, 7.4e-06, 1.3e-04, 4.1e-04, 2.1e-04),
    (7, 0.0, 'uniform'): (4.7e-04, 1.5e-05, 2.4e-04, 5.4e-04, 3.4e-04),
    (7, 1.5, 'gaussian'): (5.4e-04, 1.0e-05, 1.4e-04, 5.5e-04, 2.4e-04),
    (9, 1.5, 'gaussian'): (5.3e-04, 1.0e-05, 1.4e-04, 4.1e-04, 3.6e-04),
    (11, 2.0, 'gaussian'): (6.0e-04, 1.0e-05, 2.1e-04, 4.1e-04, 3.8e-04),
    (11, 0.0, 'uniform'): (6.0e-04, 1.2e-05, 2.1e-04, 5.7e-04, 3.5e-04),
}
TOL_FACTOR = 2.0


def tolerances(window):
    """(PX_TOL, G_TOL, GRAD_TOL, IDENT_TOL, MAPGRAD_TOL) of a window: twice its EMU_* figures."""
    return tuple(TOL_FACTOR * v for v in EMU[tuple(window)])


def full_taps(window=DEFAULT):
    """The 2R + 1 taps of the window as float64, edge .. centre .. edge: the float32 taps, widened."""
    return K.full_taps(window)


def blur(p, window=DEFAULT):
    """G: separable blur with clamped edges on every axis, same-size output, float64."""
    g, R = full_taps(window), radius(window)
    for axis in (2, 1, 0):
        n = p.shape[axis]
        q = np.pad(p, [(R, R) if a == axis else (0, 0) for a in range(3)], mode="edge")
        p = sum(g[k] * np.take(q, np.arange(k, k + n), axis=axis) for k in range(2 * R + 1))
    return p


def blur_t(v, window=DEFAULT):
    """Gt: (Gt v)(q) = sum of w_t v(p) over every (p, t) with clamp(p + t) = q, one axis after the other, by scatter-add."""
    g, R = full_taps(window), radius(window)
    t = np.arange(-R, R + 1)
    for axis in (2, 1, 0):
        n = v.shape[axis]
        idx = np.clip(np.arange(n)[:, None] + t[None, :], 0, n - 1)
        src = np.moveaxis(v, axis, 0)
        out = np.zeros_like(src)
        for k in range(2 * R + 1):
            np.add.at(out, idx[:, k], g[k] * src)
        v = np.moveaxis(out, 0, axis)
    return v


def _terms(a, b, c1, c2, window):
    ma, mb = blur(a, window), blur(b, window)
    s_aa = blur(a * a, window) - ma * ma
    s_bb = blur(b * b, window) - mb * mb
    s_ab = blur(a * b, window) - ma * mb
    A1, A2 = 2.0 * ma * mb + c1, 2.0 * s_ab + c2
    B1, B2 = ma * ma + mb * mb + c1, s_aa + s_bb + c2
    return ma, mb, A1, A2, B1, B2


def ssim_map(a, b, data_range, window=DEFAULT):
    """Per-voxel SSIM in float64."""
    c1, c2 = constants(data_range)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    _, _, A1, A2, B1, B2 = _terms(a, b, c1, c2, window)
    return A1 * A2 / (B1 * B2)


def ssim(a, b, data_range, window=DEFAULT):
    """(global SSIM as float64 -- the fp64 sum over double(W) * double(H) * double(D) --, float64 map)."""
    m = ssim_map(a, b, data_range, window)
    return float(np.sum(m) / voxels(m.shape)), m


def derivatives(a, b, data_range, window=DEFAULT):
    """What the gradient needs of one pair, in float64, whatever the upstream gradient: (a, b, d_mu_a, d_mu_b, d_aa, d_ab)."""
    c1, c2 = constants(data_range)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ma, mb, A1, A2, B1, B2 = _terms(a, b, c1, c2, window)
    s = A1 * A2 / (B1 * B2)
    d_ab = 2.0 * A1 / (B1 * B2)
    d_aa = -s / B2
    d_mu_a = 2.0 * mb * A2 / (B1 * B2) - 2.0 * ma * s / B1 - 2.0 * ma * d_aa - mb * d_ab
    d_mu_b = 2.0 * ma * A2 / (B1 * B2) - 2.0 * mb * s / B1 - 2.0 * mb * d_aa - ma * d_ab
    return a, b, d_mu_a, d_mu_b, d_aa, d_ab


def apply(der, gmap, window=DEFAULT):
    """(dLoss/da, dLoss/db) in float64 from derivatives() for dLoss/dssim(p) = gmap(p): k = gmap inside Gt."""
    a, b, d_mu_a, d_mu_b, d_aa, d_ab = der
    k = np.asarray(gmap, np.float64)
    t_aa, t_ab = blur_t(k * d_aa, window), blur_t(k * d_ab, window)
    return blur_t(k * d_mu_a, window) + 2.0 * a * t_aa + b * t_ab, blur_t(k * d_mu_b, window) + 2.0 * b * t_aa + a * t_ab


def grad_map(a, b, data_range, gmap, window=DEFAULT):
    """(dLoss/da, dLoss/db) in float64 for dLoss/dssim(p) = gmap(p) (a volume, or a scalar that stands for one): the header's
    formulas, k = gmap inside Gt."""
    return apply(derivatives(a, b, data_range, window), gmap, window)


def grad(a, b, data_range, g_out, window=DEFAULT):
    """(dLoss/da, dLoss/db) in float64 for dLoss/dS = g_out (S the global value): the uniform k = g_out / (W H D)."""
    return grad_map(a, b, data_range, float(g_out) / voxels(np.shape(a)), window)


constant_volume = W3.constant_volume
weight_volumes = W3.weight_volumes


# ---- fp32 emulation of the kernels ---------------------------------------------------------------------------------------------------


def _sl(axis, lo, n):
    s = [slice(None)] * 3
    s[axis] = slice(lo, lo + n)
    return tuple(s)


def _blur32(p, g):
    """The kernels' blur of one centred fp32 volume (already padded by R on every side, edge-clamped), g the R + 1 taps centre first.  x:
    the folded sums s_i = p[x+i] + p[x-i], h = s_0 g_0 then fma(s_i, g_i, h).  y, then z: the values of positions -R .. +R in that order,
    the first one multiplied into zero, the others fused."""
    R = len(g) - 1
    W = p.shape[2] - 2 * R
    h = (p[_sl(2, R, W)] * F(g[0])).astype(F)
    for i in range(1, R + 1):
        s = (p[_sl(2, R + i, W)] + p[_sl(2, R - i, W)]).astype(F)
        h = _fma32(s, g[i], h)
    for axis in (1, 0):
        n = h.shape[axis] - 2 * R
        v = (h[_sl(axis, 0, n)] * F(g[R])).astype(F)
        for j in range(-R + 1, R + 1):
            v = _fma32(h[_sl(axis, R + j, n)], g[abs(j)], v)
        h = v
    return h


def _adjoint32(v, w, axis):
    """The kernels' adjoint pass along one axis: out(q) = w(q, -R) v(q - R), then fma(v(q + j), w(q, j), .) for j = -R + 1 .. R; v is
    zero outside the volume."""
    R = (w.shape[0] - 1) // 2
    n = v.shape[axis]
    p = np.pad(v, [(R, R) if a == axis else (0, 0) for a in range(3)])
    shape = [1, 1, 1]
    shape[axis] = n
    acc = (p[_sl(axis, 0, n)] * w[0].reshape(shape)).astype(F)
    for t in range(1, 2 * R + 1):
        acc = _fma32(p[_sl(axis, t, n)], w[t].reshape(shape), acc)
    return acc


def forward_fp32(a, b, data_range, window=DEFAULT):
    """What the walk computes per voxel, as float32 volumes: (value as float64, map, and the derivative's terms (d_mu_a, d_mu_b, d_aa,
    d_ab, a', b') with the centred samples on the volume itself)."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    D, H, W = a.shape
    c1, c2 = (F(x) for x in constants(data_range))
    g = taps(window)
    R = len(g) - 1
    cA, cB = centre(a, data_range), centre(b, data_range)
    two = F(2.0)
    with np.errstate(all="ignore"):
        sa = (np.pad(a, R, mode="edge") - cA).astype(F)
        sb = (np.pad(b, R, mode="edge") - cB).astype(F)
        qs = _fma32(sb, sb, (sa * sa).astype(F))                             # fma(b', b', a'^2)
        x = (sa * sb).astype(F)
        mA, mB, eS, eX = _blur32(sa, g), _blur32(sb, g), _blur32(qs, g), _blur32(x, g)
        pc = (mA * mB).astype(F)
        tc = ((mA * mA).astype(F) + (mB * mB).astype(F)).astype(F)
        sS = (eS - tc).astype(F)
        sAB = (eX - pc).astype(F)
        uA, uB = (mA + cA).astype(F), (mB + cB).astype(F)
        muAB = (uA * uB).astype(F)
        tm = ((uA * uA).astype(F) + (uB * uB).astype(F)).astype(F)
        A1, A2 = _fma32(muAB, two, np.full_like(muAB, c1)), _fma32(sAB, two, np.full_like(sAB, c2))
        B1, B2 = (tm + c1).astype(F), (sS + c2).astype(F)
        n = (A1 * A2).astype(F)
        den = (B1 * B2).astype(F)
        out = (n * (F(1.0) / den).astype(F)).astype(F)
        value = float(np.sum(out.astype(np.float64)) / voxels(a.shape))
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
        ca, cb = sa[R:R + D, R:R + H, R:R + W], sb[R:R + D, R:R + H, R:R + W]
        return value, out, (d_mu(uB, uA, mA, mB), d_mu(uA, uB, mB, mA), daa, dab, ca, cb)


def apply_fp32(derivatives, k, window=DEFAULT):
    """The rest of the backward for one weight k (a float32 volume, or a float32 scalar that stands for one): k(p) d(p) as plain fp32
    products, the adjoint gathers on x, then y, then z, and the gradient in the centred variables.  (dLoss/da, dLoss/db) as float32."""
    dmA, dmB, daa, dab, ca, cb = derivatives
    k = np.asarray(k, F)
    D, H, W = ca.shape
    g = taps(window)
    wx, wy, wz = adjoint_weights(W, g), adjoint_weights(H, g), adjoint_weights(D, g)
    two = F(2.0)
    with np.errstate(all="ignore"):
        def gt(v):
            return _adjoint32(_adjoint32(_adjoint32((k * v).astype(F), wx, 2), wy, 1), wz, 0)
        r_a, r_b, r_aa, r_ab = gt(dmA), gt(dmB), gt(daa), gt(dab)
        ga = ((r_a + ((two * ca).astype(F) * r_aa).astype(F)).astype(F) + (cb * r_ab).astype(F)).astype(F)
        gb = ((r_b + ((two * cb).astype(F) * r_aa).astype(F)).astype(F) + (ca * r_ab).astype(F)).astype(F)
    return ga, gb


def emulate_fp32(a, b, data_range, window=DEFAULT, g_out=None, gmap=None):
    """(global value as float64, float32 map) as the kernels compute them; with g_out (a scalar dLoss/dS) or gmap (a float32 volume
    dLoss/dssim(p)) also the float32 gradients: (value, map, dLoss/da, dLoss/db)."""
    value, out, der = forward_fp32(a, b, data_range, window)
    if g_out is None and gmap is None:
        return value, out
    k = F(float(F(g_out)) / voxels(np.shape(a))) if gmap is None else np.asarray(gmap, F)
    ga, gb = apply_fp32(der, k, window)
    return value, out, ga, gb


def measure(manifest, window, fixtures=FIXTURES):
    """(px, global, grad, ident, mapgrad) of emulate_fp32 against the float64 model for one window: the worst over fixtures x FORMS (see
    EMU); mapgrad also over ssim3w_model's weight volumes (fixed seeds: the fixture's index)."""
    px = gl = gr = ident = mg = 0.0
    for seed, name in enumerate(fixtures):
        for _, fa, fb, r in fixture_forms(manifest, name):
            gv, gm = ssim(fa, fb, r, window)
            ev, em, der = forward_fp32(fa, fb, r, window)
            px = max(px, float(np.abs(em - gm).max()))
            gl = max(gl, abs(ev - gv))
            k = F(1.0 / voxels(fa.shape))
            der64 = derivatives(fa, fb, r, window)
            for e, w in zip(apply_fp32(der, k, window), apply(der64, 1.0 / voxels(fa.shape), window)):
                gr = max(gr, float(np.abs(e - w).max() / np.abs(w).max()))
            for _, kv in weight_volumes(fa.shape, seed):
                for e, w in zip(apply_fp32(der, kv, window), apply(der64, kv, window)):
                    mg = max(mg, float(np.abs(e - w).max() / np.abs(w).max()))
            _, _, ea, eb = emulate_fp32(fa, fa, r, window, g_out=1.0)
            ident = max(ident, float(max(np.abs(ea).max(), np.abs(eb).max())) * voxels(fa.shape) * r)
    return px, gl, gr, ident, mg
