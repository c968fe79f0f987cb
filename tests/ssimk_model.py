"""float64 model of the library's SSIM of float32 samples under a caller-chosen window (the definition in include/rmgr/ssim-hip.h,
rmgr_ssim_hip_Window and the rmgr_ssim_hip_*_ssimf_win* entries), on top of tests/ssimf_model.py and tests/ssimw_model.py, which stay as
they are.

The yardstick of tests/test_ssimk_cpu.py and tests/test_gpu_ssimk.py.  A window is (size, sigma, kind): taps() restates the header's rule
for its taps; blur / blur_t / ssim_map / ssim / grad / grad_map are ssimf_model's and ssimw_model's functions with 5 replaced by the
window's radius R = (size - 1) / 2 -- the clamped separable window G, the per-pixel formula, the fp64 mean over double(W) * double(H), and
the exact derivative with Gt, the ADJOINT of the clamped window, built as defined: a scatter-add of w_t v(p) onto clamp(p + t).  At the
default window (11, 1.5, "gaussian") every function returns exactly what ssimf_model / ssimw_model return.

emulate_fp32() restates the KERNELS' arithmetic (strip_body and grad_body of ssim2_walk.h: instantiated by ssimk_kernels.hip for R = 1 .. 4, by
ssimf_kernels.hip / ssimw_kernels.hip with the window's taps for R = 5): ssimf_model.emulate_fp32 and ssimw_model.emulate_fp32_map_grad with 5 replaced by R.
"""
import numpy as np

import ssimf_model as M
from ssimf_model import F, STRIP_W, _fma32, centres, constants  # noqa: F401  (re-exported for the tests)

DEFAULT = (11, 1.5, "gaussian")
SIZES = (3, 5, 7, 9, 11)
# The windows the emulation and the GPU are measured with.
WINDOWS = ((3, 0.0, "uniform"), (5, 0.8, "gaussian"), (7, 0.0, "uniform"), (7, 1.5, "gaussian"), (9, 1.5, "gaussian"),
           (11, 2.0, "gaussian"), (11, 0.0, "uniform"))
# The golden pairs they are measured on, in the forms "unit" (/ 255, range 1) and "raw" (as stored, range 255) of ssimf_model.forms().
FIXTURES = ("bbb255x63_q00_ch1", "bbb255x63_q50_ch1", "bbb257x65_q00_ch1", "bbb257x65_q50_ch1", "einstein_blur")
FORMS = ("unit", "raw")

# What the fp32 emulation below measures against the float64 model, per window the worst over FIXTURES x FORMS (tests/test_ssimk_cpu.py
# pins the figures): per pixel, global, gradient error over the plane's largest float64 gradient magnitude -- for the scalar upstream
# gradient and for the standard-normal and one-hot planes of upstream_planes() --, and max|grad| * W * H * R on the pair of identical
# images (every fixture's A against itself: exact gradient 0).  The GPU tests assert about twice these (*_TOL): the project's standing
# margin for the 1-ulp reciprocal and the order of the fp64 sum, which the emulation does not restate.
EMU = {
    # window: (EMU_PX, EMU_G, EMU_GRAD, EMU_IDENT)
    (3, 0.0, 'uniform'): (1.8e-04, 2.7e-06, 9.8e-05, 3.7e-04),
    (5, 0.8, 'gaussian'): (1.9e-04, 1.5e-06, 9.3e-05, 2.5e-04),
    (7, 0.0, 'uniform'): (1.9e-04, 2.4e-06, 5.9e-05, 3.7e-04),
    (7, 1.5, 'gaussian'): (2.1e-04, 6.7e-07, 5.3e-05, 2.5e-04),
    (9, 1.5, 'gaussian'): (2.8e-04, 1.4e-06, 6.1e-05, 3.7e-04),
    (11, 2.0, 'gaussian'): (2.3e-04, 5.5e-07, 6.1e-05, 3.7e-04),
    (11, 0.0, 'uniform'): (2.1e-04, 1.2e-06, 7.2e-05, 2.5e-04),
}
TOL_FACTOR = 2.0


def tolerances(window):
    """(PX_TOL, G_TOL, GRAD_TOL, IDENT_TOL) of a window: twice its EMU_* figures."""
    return tuple(TOL_FACTOR * v for v in EMU[tuple(window)])


def name_of(window):
    size, sigma, kind = window
    return "%d box" % size if kind == "uniform" else "%d Gaussian %g" % (size, sigma)


def radius(window):
    return (window[0] - 1) // 2


def taps(window=DEFAULT):
    """The window's taps, centre first (R + 1 float32 values), by the header's rule.  Gaussian: s = double(float(sigma)),
    g_i = exp(-(i i) / (2 s s)), the norm accumulated in double in the order i = 0 .. R with g_0 once and the others twice, tap i =
    float(g_i / norm).  Uniform: every tap float(1.0 / size)."""
    size, sigma, kind = window
    assert size in SIZES and kind in ("gaussian", "uniform")
    R = (size - 1) // 2
    if kind == "uniform":
        return np.full(R + 1, F(1.0 / float(size)), F)
    s = float(F(sigma))
    assert s > 0.0 and np.isfinite(s)
    g = [float(np.exp(-float(i * i) / (2.0 * s * s))) for i in range(R + 1)]
    norm = 0.0
    for i in range(R + 1):
        norm += g[i] if i == 0 else 2.0 * g[i]
    return np.array([F(g[i] / norm) for i in range(R + 1)], F)


def full_taps(window=DEFAULT):
    """The 2R + 1 taps of the window as float64, edge .. centre .. edge: the float32 taps, widened (the engine's taps)."""
    g = taps(window).astype(np.float64)
    return np.concatenate([g[:0:-1], g])


def blur(p, window=DEFAULT):
    """G: separable blur with clamped edges, same-size output, float64."""
    g = full_taps(window)
    R = radius(window)
    h, w = p.shape
    q = np.pad(p, R, mode="edge")
    rows = sum(g[k] * q[:, k:k + w] for k in range(2 * R + 1))
    return sum(g[k] * rows[k:k + h, :] for k in range(2 * R + 1))


def blur_t(v, window=DEFAULT):
    """Gt: (Gt v)(q) = sum of w_t v(p) over every (p, t) with clamp(p + t) = q, one axis after the other, by scatter-add."""
    g = full_taps(window)
    R = radius(window)
    h, w = v.shape
    t = np.arange(-R, R + 1)
    iy = np.clip(np.arange(h)[:, None] + t[None, :], 0, h - 1)
    ix = np.clip(np.arange(w)[:, None] + t[None, :], 0, w - 1)
    rows = np.zeros((h, w), np.float64)
    for k in range(2 * R + 1):
        np.add.at(rows, iy[:, k], g[k] * v)
    out = np.zeros((h, w), np.float64)
    for k in range(2 * R + 1):
        np.add.at(out, (slice(None), ix[:, k]), g[k] * rows)
    return out


def _terms(a, b, c1, c2, window):
    ma, mb = blur(a, window), blur(b, window)
    s_aa = blur(a * a, window) - ma * ma
    s_bb = blur(b * b, window) - mb * mb
    s_ab = blur(a * b, window) - ma * mb
    A1, A2 = 2.0 * ma * mb + c1, 2.0 * s_ab + c2
    B1, B2 = ma * ma + mb * mb + c1, s_aa + s_bb + c2
    return ma, mb, A1, A2, B1, B2


def ssim_map(a, b, data_range, window=DEFAULT):
    """Per-pixel SSIM in float64."""
    c1, c2 = constants(data_range)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    _, _, A1, A2, B1, B2 = _terms(a, b, c1, c2, window)
    return A1 * A2 / (B1 * B2)


def ssim(a, b, data_range, window=DEFAULT):
    """(global SSIM as float64 -- the fp64 sum over double(W) * double(H) --, float64 map)."""
    m = ssim_map(a, b, data_range, window)
    return float(np.sum(m) / (float(m.shape[1]) * float(m.shape[0]))), m


def grad_map(a, b, data_range, gmap, window=DEFAULT):
    """(dLoss/da, dLoss/db) in float64 for dLoss/dssim(p) = gmap(p): the header's formulas, k = gmap inside Gt."""
    c1, c2 = constants(data_range)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    k = np.asarray(gmap, np.float64)
    assert k.shape == a.shape == b.shape
    ma, mb, A1, A2, B1, B2 = _terms(a, b, c1, c2, window)
    s = A1 * A2 / (B1 * B2)
    d_ab = 2.0 * A1 / (B1 * B2)
    d_aa = -s / B2
    d_mu_a = 2.0 * mb * A2 / (B1 * B2) - 2.0 * ma * s / B1 - 2.0 * ma * d_aa - mb * d_ab
    d_mu_b = 2.0 * ma * A2 / (B1 * B2) - 2.0 * mb * s / B1 - 2.0 * mb * d_aa - ma * d_ab
    t_aa, t_ab = blur_t(k * d_aa, window), blur_t(k * d_ab, window)
    return blur_t(k * d_mu_a, window) + 2.0 * a * t_aa + b * t_ab, blur_t(k * d_mu_b, window) + 2.0 * b * t_aa + a * t_ab


def grad(a, b, data_range, g_out, window=DEFAULT):
    """(dLoss/da, dLoss/db) in float64 for dLoss/dS = g_out (S the global value): the uniform k = g_out / (W H).  A scalar k stands
    for the plane: the same products in the same order."""
    a = np.asarray(a, np.float64)
    k = float(g_out) / (float(a.shape[1]) * float(a.shape[0]))
    return grad_map(a, b, data_range, np.full(a.shape, k), window)


def constant_plane(g_out, h, w):
    """The plane of the header's identity clause: every element float(double(gOut) / (double(W) * double(H)))."""
    return np.full((h, w), F(float(F(g_out)) / (float(w) * float(h))), F)


def upstream_planes(h, w, seed=0):
    """The per-pixel upstream gradients the emulation and the GPU are measured with: (name, float32 plane).  Seeded standard normal;
    one-hot at (31, 31) (the last pixel of the first gradient tile), clipped into the plane."""
    rng = np.random.default_rng(2000 + seed)
    yield "normal", rng.standard_normal((h, w)).astype(F)
    p = np.zeros((h, w), F)
    p[min(31, h - 1), min(31, w - 1)] = 1
    yield "one-hot", p


# ---- fp32 emulation of the kernels ---------------------------------------------------------------------------------------------------

def _blur32(p, g):
    """The kernels' blur of one centred fp32 plane (already padded by R on every side, edge-clamped), g the R + 1 taps centre first:
    per column m the folded sums s_i = p[m+i] + p[m-i], h = s_0 g_0 then fma(s_i, g_i, h); per output row y the column pass adds h
    of rows y-R .. y+R in that order, the first one multiplied into zero."""
    R = len(g) - 1
    H, W = p.shape[0] - 2 * R, p.shape[1] - 2 * R
    c = p[:, R:R + W]
    h = (c * F(g[0])).astype(F)
    for i in range(1, R + 1):
        s = (p[:, R + i:R + i + W] + p[:, R - i:R - i + W]).astype(F)
        h = _fma32(s, g[i], h)
    v = (h[0:H] * F(g[R])).astype(F)
    for j in range(-R + 1, R + 1):
        v = _fma32(h[R + j:R + j + H], g[abs(j)], v)
    return v


def adjoint_weights(n, g):
    """w[j + R][q], j = -R .. R: what gradient pixel q of an axis of n pixels collects from p = q + j.  The tap g|j| in the interior;
    on the first (last) pixel tail[|j|] = g|j| + ... + gR for j >= 0 (j <= 0) -- the taps the forward pass clamped onto it --; the
    sum of all taps when n == 1.  tail and the total: sums of the float taps in double, rounded once."""
    g = np.asarray(g, F)
    R = len(g) - 1
    tail = np.cumsum(g[::-1].astype(np.float64))[::-1].astype(F)
    total = F(2.0 * float(np.sum(g.astype(np.float64))) - float(g[0]))
    w = np.zeros((2 * R + 1, n), F)
    for j in range(-R, R + 1):
        w[j + R, :] = g[abs(j)]
        w[j + R, 0] = tail[abs(j)] if j >= 0 else 0
        if n > 1:
            w[j + R, n - 1] = tail[abs(j)] if j <= 0 else 0
        else:
            w[j + R, 0] = total if j == 0 else 0
    return w


def _adjoint32(v, w, axis):
    """The kernels' adjoint pass along one axis: out(q) = w(q, -R) v(q - R), then fma(v(q + j), w(q, j), .) for j = -R + 1 .. R; v is
    zero outside the image."""
    if axis == 0:
        return _adjoint32(v.T, w, 1).T
    R = (w.shape[0] - 1) // 2
    n = v.shape[1]
    p = np.pad(v, ((0, 0), (R, R)))
    acc = (p[:, 0:n] * w[0][None, :]).astype(F)
    for t in range(1, 2 * R + 1):
        acc = _fma32(p[:, t:t + n], w[t][None, :], acc)
    return acc


def emulate_fp32(a, b, data_range, window=DEFAULT, g_out=None, gmap=None):
    """(global value as float64, float32 map) as the kernels compute them, strip column by strip column; with g_out (a scalar dLoss/dS)
    or gmap (a float32 plane dLoss/dssim(p)) also the float32 gradients: (value, map, dLoss/da, dLoss/db)."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    H, W = a.shape
    c1, c2 = (F(x) for x in constants(data_range))
    g = taps(window)
    R = len(g) - 1
    cA, cB = centres(a, data_range), centres(b, data_range)
    pa, pb = np.pad(a, R, mode="edge"), np.pad(b, R, mode="edge")
    out = np.empty((H, W), F)
    want_grad = g_out is not None or gmap is not None
    if want_grad:
        ga, gb = np.empty((H, W), F), np.empty((H, W), F)
        k = np.asarray(gmap, F) if gmap is not None else F(float(F(g_out)) / (float(W) * float(H)))
        wx, wy = adjoint_weights(W, g), adjoint_weights(H, g)
    two = F(2.0)
    with np.errstate(all="ignore"):
        for i, x0 in enumerate(range(0, W, STRIP_W)):
            x1 = min(x0 + STRIP_W, W)
            # the forward kernel blurs its own columns only; the gradient kernel needs the statistics R columns beyond them, under
            # the same centre: the whole width is blurred with this strip column's centre and the columns wanted are taken
            lo, hi = (0, W) if want_grad else (x0, x1)
            sa = (pa[:, lo:hi + 2 * R] - cA[i]).astype(F)
            sb = (pb[:, lo:hi + 2 * R] - cB[i]).astype(F)
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
            den = (B1 * B2).astype(F)
            out[:, x0:x1] = (n * (F(1.0) / den).astype(F)).astype(F)[:, x0 - lo:x1 - lo]
            if not want_grad:
                continue
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
            ca, cb = sa[R:R + H, R:R + W], sb[R:R + H, R:R + W]              # a', b' at the pixel
            va = ((r_a + ((two * ca).astype(F) * r_aa).astype(F)).astype(F) + (cb * r_ab).astype(F)).astype(F)
            vb = ((r_b + ((two * cb).astype(F) * r_aa).astype(F)).astype(F) + (ca * r_ab).astype(F)).astype(F)
            ga[:, x0:x1], gb[:, x0:x1] = va[:, x0:x1], vb[:, x0:x1]
    value = float(np.sum(out.astype(np.float64)) / (float(W) * float(H)))
    return (value, out, ga, gb) if want_grad else (value, out)


def fixture_forms(manifest, name):
    """The forms of FORMS of one golden pair: (form, float32 a, float32 b, data range)."""
    from conftest import load_pair
    a, b = load_pair(manifest[name])
    return [f for f in M.forms(a, b) if f[0] in FORMS]


def measure(manifest, window, fixtures=FIXTURES):
    """(px, global, grad, ident) of emulate_fp32 against the float64 model for one window: the worst over fixtures x FORMS (see EMU)."""
    px = gl = gr = ident = 0.0
    for name in fixtures:
        for _, fa, fb, r in fixture_forms(manifest, name):
            h, w = fa.shape
            gv, gm = ssim(fa, fb, r, window)
            ups = [("scalar", None)] + list(upstream_planes(h, w))
            for uname, plane in ups:
                if plane is None:
                    ev, em, ea, eb = emulate_fp32(fa, fb, r, window, g_out=1.0)
                    wa, wb = grad(fa, fb, r, 1.0, window)
                    px = max(px, float(np.abs(em - gm).max()))
                    gl = max(gl, abs(ev - gv))
                else:
                    _, _, ea, eb = emulate_fp32(fa, fb, r, window, gmap=plane)
                    wa, wb = grad_map(fa, fb, r, plane, window)
                for e, g in ((ea, wa), (eb, wb)):
                    gr = max(gr, float(np.abs(e - g).max() / np.abs(g).max()))
            _, _, ea, eb = emulate_fp32(fa, fa, r, window, g_out=1.0)
            ident = max(ident, float(max(np.abs(ea).max(), np.abs(eb).max())) * h * w * r)
    return px, gl, gr, ident
