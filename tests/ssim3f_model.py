"""float64 model of the library's SSIM of float32 VOLUMES under the three-dimensional window and of its gradient (the definition in
include/rmgr/ssim-hip.h, rmgr_ssim_hip_*_ssim3f*).

The yardstick of tests/test_ssim3f_cpu.py and tests/test_gpu_ssim3f.py.  Volumes are (D, H, W) arrays.  C1 / C2 from the data range
(ssimf_model.constants), the clamped separable 11-tap Gaussian G (sigma 1.5, the engine's fp32 taps) over x, y and z, the SSIM formula per
voxel, the fp64 mean over double(W) * double(H) * double(D), and the exact derivative with Gt, the ADJOINT of the clamped window, built as
defined: a scatter-add of w_t v(p) onto clamp(p + t), one axis after the other.  Plain numpy, no reference to the GPU code.

emulate_fp32() restates the KERNELS' arithmetic (ssim3f_kernels.hip): ONE centre per volume -- the sample at ((W - 1) / 2, (H - 1) / 2,
(D - 1) / 2) when its magnitude is at most the data range, else 0 --, fp32 volumes, the x pass centre tap first on folded sums, the y pass
and the z pass in source order with the first product plain, fma where the kernels fuse, the gradient in the centred variables with the
adjoint as a weighted gather on x, then y, then z: what the GPU should produce up to the order of the fp64 sum and the 1-ulp reciprocal.
"""
import numpy as np

import ssimf_model as M
from ssimf_model import F, _fma32, adjoint_weights, constants, gaussian_taps  # noqa: F401  (re-exported for the tests)

# The golden pairs the emulation and the GPU are measured on, as volumes (golden_volume), in the forms of ssimf_model.forms().
FIXTURES = ("bbb255x63_q00_ch1", "bbb255x63_q50_ch1", "bbb257x65_q00_ch1", "bbb257x65_q50_ch1", "einstein_blur")
FORMS = ("unit", "raw")
SLICES = 12

# What the fp32 emulation below measures against the float64 model, the worst over FIXTURES x FORMS (tests/test_ssim3f_cpu.py pins the
# figures from both sides): per voxel, global, gradient error over the volume's largest float64 gradient magnitude, and max|grad| * W * H
# * D * R on the pair of identical volumes (every fixture's A against itself: exact gradient 0).  The GPU tests assert twice these: the
# project's standing margin for the 1-ulp reciprocal and the order of the fp64 sum, which the emulation does not restate.
EMU_PX, EMU_G, EMU_GRAD, EMU_IDENT = 5.3e-4, 4.8e-6, 9.5e-5, 4.1e-4
TOL_FACTOR = 2.0


def tolerances():
    """(PX_TOL, G_TOL, GRAD_TOL, IDENT_TOL): twice the EMU_* figures."""
    return tuple(TOL_FACTOR * v for v in (EMU_PX, EMU_G, EMU_GRAD, EMU_IDENT))


def golden_volume(img):
    """The volume cut from one golden image (H x W): slice z is the crop img[z : z + H - 11, 2z : 2z + W - 22], z = 0 .. 11."""
    h, w = img.shape
    return np.stack([img[z:z + h - 11, 2 * z:2 * z + w - 22] for z in range(SLICES)])


def fixture_forms(manifest, name, forms=FORMS):
    """The forms of one golden pair as volumes: (form, float32 a, float32 b, data range)."""
    from conftest import load_pair
    a, b = load_pair(manifest[name])
    return [(f, np.ascontiguousarray(golden_volume(fa)), np.ascontiguousarray(golden_volume(fb)), r) for f, fa, fb, r in M.forms(a, b) if f in forms]


def blur(p, g=None):
    """G: separable 11 + 11 + 11 blur with clamped edges on every axis, same-size output, float64."""
    g = gaussian_taps() if g is None else g
    for axis in (2, 1, 0):
        n = p.shape[axis]
        q = np.pad(p, [(5, 5) if a == axis else (0, 0) for a in range(3)], mode="edge")
        p = sum(g[k] * np.take(q, np.arange(k, k + n), axis=axis) for k in range(11))
    return p


def blur_t(v, g=None):
    """Gt: (Gt v)(q) = sum of w_t v(p) over every (p, t) with clamp(p + t) = q, one axis after the other, by scatter-add."""
    g = gaussian_taps() if g is None else g
    t = np.arange(-5, 6)
    for axis in (2, 1, 0):
        n = v.shape[axis]
        idx = np.clip(np.arange(n)[:, None] + t[None, :], 0, n - 1)
        src = np.moveaxis(v, axis, 0)
        out = np.zeros_like(src)
        for k in range(11):
            np.add.at(out, idx[:, k], g[k] * src)
        v = np.moveaxis(out, 0, axis)
    return v


def _terms(a, b, c1, c2, g):
    ma, mb = blur(a, g), blur(b, g)
    s_aa = blur(a * a, g) - ma * ma
    s_bb = blur(b * b, g) - mb * mb
    s_ab = blur(a * b, g) - ma * mb
    A1, A2 = 2.0 * ma * mb + c1, 2.0 * s_ab + c2
    B1, B2 = ma * ma + mb * mb + c1, s_aa + s_bb + c2
    return ma, mb, A1, A2, B1, B2


def ssim_map(a, b, data_range, g=None):
    """Per-voxel SSIM in float64."""
    c1, c2 = constants(data_range)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    _, _, A1, A2, B1, B2 = _terms(a, b, c1, c2, g)
    return A1 * A2 / (B1 * B2)


def voxels(shape):
    d, h, w = shape
    return float(w) * float(h) * float(d)


def ssim(a, b, data_range, g=None):
    """(global SSIM as float64 -- the fp64 sum over double(W) * double(H) * double(D) --, float64 map)."""
    m = ssim_map(a, b, data_range, g)
    return float(np.sum(m) / voxels(m.shape)), m


def grad(a, b, data_range, g_out, g=None):
    """(dLoss/da, dLoss/db) in float64 for dLoss/dS = g_out: the header's formulas."""
    c1, c2 = constants(data_range)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ma, mb, A1, A2, B1, B2 = _terms(a, b, c1, c2, g)
    s = A1 * A2 / (B1 * B2)
    k = float(g_out) / voxels(a.shape)
    d_ab = 2.0 * A1 / (B1 * B2)
    d_aa = -s / B2
    d_mu_a = 2.0 * mb * A2 / (B1 * B2) - 2.0 * ma * s / B1 - 2.0 * ma * d_aa - mb * d_ab
    d_mu_b = 2.0 * ma * A2 / (B1 * B2) - 2.0 * mb * s / B1 - 2.0 * mb * d_aa - ma * d_ab
    t_aa, t_ab = blur_t(k * d_aa, g), blur_t(k * d_ab, g)
    return blur_t(k * d_mu_a, g) + 2.0 * a * t_aa + b * t_ab, blur_t(k * d_mu_b, g) + 2.0 * b * t_aa + a * t_ab


# ---- fp32 emulation of ssim3f_kernels.hip ---------------------------------------------------------------------------------


def centre(vol, data_range):
    """The volume's centre: the sample at ((W - 1) // 2, (H - 1) // 2, (D - 1) // 2) when its magnitude is at most the data range, else 0."""
    vol = np.asarray(vol, F)
    d, h, w = vol.shape
    c = vol[(d - 1) // 2, (h - 1) // 2, (w - 1) // 2]
    with np.errstate(invalid="ignore"):
        return c if np.abs(c) <= F(data_range) else F(0)


def _sl(axis, lo, n):
    s = [slice(None)] * 3
    s[axis] = slice(lo, lo + n)
    return tuple(s)


def _blur32(p, g):
    """The kernels' blur of one centred fp32 volume (already padded by 5 on every side, edge-clamped).  x: the folded sums s_i = p[x+i] +
    p[x-i], h = s_0 g_0 then fma(s_i, g_i, h).  y, then z: the values of positions -5 .. +5 in that order, the first one multiplied into
    zero, the others fused."""
    W = p.shape[2] - 10
    h = (p[_sl(2, 5, W)] * F(g[0])).astype(F)
    for i in range(1, 6):
        s = (p[_sl(2, 5 + i, W)] + p[_sl(2, 5 - i, W)]).astype(F)
        h = _fma32(s, g[i], h)
    for axis in (1, 0):
        n = h.shape[axis] - 10
        v = (h[_sl(axis, 0, n)] * F(g[5])).astype(F)
        for j in range(-4, 6):
            v = _fma32(h[_sl(axis, 5 + j, n)], g[abs(j)], v)
        h = v
    return h


def _adjoint32(v, w, axis):
    """The kernels' adjoint pass along one axis: out(q) = w(q, -5) v(q - 5), then fma(v(q + j), w(q, j), .) for j = -4 .. 5; v is zero
    outside the volume."""
    n = v.shape[axis]
    p = np.pad(v, [(5, 5) if a == axis else (0, 0) for a in range(3)])
    shape = [1, 1, 1]
    shape[axis] = n
    acc = (p[_sl(axis, 0, n)] * w[0].reshape(shape)).astype(F)
    for t in range(1, 11):
        acc = _fma32(p[_sl(axis, t, n)], w[t].reshape(shape), acc)
    return acc


def emulate_fp32(a, b, data_range, g_out=None):
    """(global value as float64, float32 map) as the kernels compute them; with g_out also the float32 gradients: (value, map, dLoss/da,
    dLoss/db)."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    D, H, W = a.shape
    c1, c2 = (F(x) for x in constants(data_range))
    g = gaussian_taps().astype(F)[5:]          # centre .. edge
    cA, cB = centre(a, data_range), centre(b, data_range)
    two = F(2.0)
    with np.errstate(all="ignore"):
        sa = (np.pad(a, 5, mode="edge") - cA).astype(F)
        sb = (np.pad(b, 5, mode="edge") - cB).astype(F)
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
        if g_out is None:
            return value, out
        k = F(float(F(g_out)) / voxels(a.shape))
        wx, wy, wz = adjoint_weights(W, g), adjoint_weights(H, g), adjoint_weights(D, g)
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
            return _adjoint32(_adjoint32(_adjoint32((k * v).astype(F), wx, 2), wy, 1), wz, 0)
        r_a, r_b, r_aa, r_ab = gt(d_mu(uB, uA, mA, mB)), gt(d_mu(uA, uB, mB, mA)), gt(daa), gt(dab)
        ca, cb = sa[5:5 + D, 5:5 + H, 5:5 + W], sb[5:5 + D, 5:5 + H, 5:5 + W]      # a', b' at the voxel
        ga = ((r_a + ((two * ca).astype(F) * r_aa).astype(F)).astype(F) + (cb * r_ab).astype(F)).astype(F)
        gb = ((r_b + ((two * cb).astype(F) * r_aa).astype(F)).astype(F) + (ca * r_ab).astype(F)).astype(F)
    return value, out, ga, gb


def measure(manifest, fixtures=FIXTURES):
    """(px, global, grad, ident) of emulate_fp32 against the float64 model: the worst over fixtures x FORMS (see EMU_*)."""
    px = gl = gr = ident = 0.0
    for name in fixtures:
        for _, fa, fb, r in fixture_forms(manifest, name):
            gv, gm = ssim(fa, fb, r)
            ev, em, ea, eb = emulate_fp32(fa, fb, r, g_out=1.0)
            wa, wb = grad(fa, fb, r, 1.0)
            px = max(px, float(np.abs(em - gm).max()))
            gl = max(gl, abs(ev - gv))
            for e, w in ((ea, wa), (eb, wb)):
                gr = max(gr, float(np.abs(e - w).max() / np.abs(w).max()))
            _, _, ea, eb = emulate_fp32(fa, fa, r, g_out=1.0)
            ident = max(ident, float(max(np.abs(ea).max(), np.abs(eb).max())) * voxels(fa.shape) * r)
    return px, gl, gr, ident
