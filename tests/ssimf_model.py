"""float64 model of the library's SSIM of float32 samples and of its gradient (the definition in include/rmgr/ssim-hip.h,
rmgr_ssim_hip_*_ssimf*).

The yardstick of tests/test_ssimf_cpu.py and tests/test_gpu_ssimf.py: C1 / C2 from the data range, the clamped separable 11-tap Gaussian
G (sigma 1.5), the SSIM formula per pixel, the fp64 mean over double(W) * double(H), and the exact derivative with Gt, the ADJOINT of the
clamped window, built as defined: a scatter-add of w_t v(p) onto clamp(p + t).  Plain numpy, no reference to the GPU code.

c1 / c2: the kernels use the float-rounded constants (constants(R, f32=True)); the reference's double oracle (oracle.ssim_naive_f64)
uses the double ones, which tests pass in when they tie the model to that oracle at range 255.

emulate_fp32() restates the KERNELS' arithmetic (centre per 128-column strip column, fp32 planes, row pass then column pass in the
kernels' order, fma where the kernels fuse, the gradient in the centred variables with the adjoint as a weighted gather): what the GPU
should produce up to the order of the fp64 sum and the 1-ulp reciprocal.
"""
import numpy as np

STRIP_W = 128

# What the fp32 emulation below measures against the float64 model, the worst over every golden pair in the three forms of forms()
# (tests/test_ssimf_cpu.py pins the figures): per pixel, global, gradient error over the plane's largest float64 gradient magnitude,
# and max|grad| * W * H * R on the pair of identical images (exact gradient 0).  The GPU tests assert about twice these.
EMU_PX, EMU_G, EMU_GRAD, EMU_IDENT = 2.4e-4, 1.2e-6, 8.4e-5, 3.7e-4
PX_TOL, G_TOL, GRAD_TOL, IDENT_TOL = 5e-4, 2.5e-6, 1.7e-4, 7.5e-4
SCALE = np.float32(1000.0 / 255.0 * 0.9973)       # the third form: a non-integer factor towards range 1000


def forms(a, b):
    """The three forms every golden (uint8) pair is compared in: (name, float32 a, float32 b, data range)."""
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    yield "unit", fa / np.float32(255), fb / np.float32(255), 1.0
    yield "raw", fa, fb, 255.0
    yield "scaled", fa * SCALE, fb * SCALE, 1000.0


def constants(data_range, f32=True):
    """(C1, C2) of a data range: (0.01 R)^2, (0.03 R)^2 with the products in double, rounded to float when f32."""
    R = float(np.float32(data_range))
    c1, c2 = (0.01 * R) * (0.01 * R), (0.03 * R) * (0.03 * R)
    if f32:
        return float(np.float32(c1)), float(np.float32(c2))
    return c1, c2


def gaussian_taps(f32=True):
    """The true 1-D Gaussian, sigma 1.5, normalised over its 11 taps, as float64; f32: rounded to float first (the engine's taps)."""
    i = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    g = g / g.sum()
    return g.astype(np.float32).astype(np.float64) if f32 else g


def blur(p, g=None):
    """G: separable 11 + 11 blur with clamped edges, same-size output, float64."""
    g = gaussian_taps() if g is None else g
    h, w = p.shape
    q = np.pad(p, 5, mode="edge")
    rows = sum(g[k] * q[:, k:k + w] for k in range(11))
    return sum(g[k] * rows[k:k + h, :] for k in range(11))


def blur_t(v, g=None):
    """Gt: (Gt v)(q) = sum of w_t v(p) over every (p, t) with clamp(p + t) = q, one axis after the other, by scatter-add."""
    g = gaussian_taps() if g is None else g
    h, w = v.shape
    t = np.arange(-5, 6)
    iy = np.clip(np.arange(h)[:, None] + t[None, :], 0, h - 1)
    ix = np.clip(np.arange(w)[:, None] + t[None, :], 0, w - 1)
    rows = np.zeros((h, w), np.float64)
    for k in range(11):
        np.add.at(rows, iy[:, k], g[k] * v)
    out = np.zeros((h, w), np.float64)
    for k in range(11):
        np.add.at(out, (slice(None), ix[:, k]), g[k] * rows)
    return out


def _terms(a, b, c1, c2, g):
    ma, mb = blur(a, g), blur(b, g)
    s_aa = blur(a * a, g) - ma * ma
    s_bb = blur(b * b, g) - mb * mb
    s_ab = blur(a * b, g) - ma * mb
    A1, A2 = 2.0 * ma * mb + c1, 2.0 * s_ab + c2
    B1, B2 = ma * ma + mb * mb + c1, s_aa + s_bb + c2
    return ma, mb, A1, A2, B1, B2


def ssim_map(a, b, data_range, c1=None, c2=None, g=None):
    """Per-pixel SSIM in float64."""
    if c1 is None:
        c1, c2 = constants(data_range)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    _, _, A1, A2, B1, B2 = _terms(a, b, c1, c2, g)
    return A1 * A2 / (B1 * B2)


def ssim(a, b, data_range, c1=None, c2=None, g=None):
    """(global SSIM as float64 -- the fp64 sum over double(W) * double(H) --, float64 map)."""
    m = ssim_map(a, b, data_range, c1, c2, g)
    return float(np.sum(m) / (float(m.shape[1]) * float(m.shape[0]))), m


def grad(a, b, data_range, g_out, c1=None, c2=None, g=None):
    """(dLoss/da, dLoss/db) in float64 for dLoss/dS = g_out: the header's formulas."""
    if c1 is None:
        c1, c2 = constants(data_range)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ma, mb, A1, A2, B1, B2 = _terms(a, b, c1, c2, g)
    s = A1 * A2 / (B1 * B2)
    k = float(g_out) / (float(a.shape[1]) * float(a.shape[0]))
    d_ab = 2.0 * A1 / (B1 * B2)
    d_aa = -s / B2
    d_mu_a = 2.0 * mb * A2 / (B1 * B2) - 2.0 * ma * s / B1 - 2.0 * ma * d_aa - mb * d_ab
    d_mu_b = 2.0 * ma * A2 / (B1 * B2) - 2.0 * mb * s / B1 - 2.0 * mb * d_aa - ma * d_ab
    t_aa, t_ab = blur_t(k * d_aa, g), blur_t(k * d_ab, g)
    return blur_t(k * d_mu_a, g) + 2.0 * a * t_aa + b * t_ab, blur_t(k * d_mu_b, g) + 2.0 * b * t_aa + a * t_ab


# ---- fp32 emulation of ssimf_kernels.hip (ssim2_walk.h) -------------------------------------------------------------------------------

F = np.float32


def _fma32(x, y, z):
    """float32 fma: the product is exact in float64 (24 + 24 bits); one rounding of the sum (to float64, then float32)."""
    return (np.asarray(x, F).astype(np.float64) * np.asarray(y, F).astype(np.float64) + np.asarray(z, F).astype(np.float64)).astype(F)


def centres(img, data_range):
    """The centre of every 128-column strip column: the sample at (min(x0 + 64, W - 1), (H - 1) // 2) when its magnitude is at most
    the data range, else 0."""
    img = np.asarray(img, F)
    h, w = img.shape
    xs = np.minimum(np.arange(0, w, STRIP_W) + 64, w - 1)
    c = img[(h - 1) // 2, xs].copy()
    with np.errstate(invalid="ignore"):
        c[~(np.abs(c) <= F(data_range))] = 0
    return c


def _blur32(p, g):
    """The kernels' blur of one centred fp32 plane (already padded by 5 on every side, edge-clamped): per column m the folded
    sums s_i = p[m+i] + p[m-i], h = s_0 g_0 then fma(s_i, g_i, h); per output row y the column pass adds h of rows y-5 .. y+5 in
    that order, the first one multiplied into zero."""
    H, W = p.shape[0] - 10, p.shape[1] - 10
    c = p[:, 5:5 + W]
    h = (c * F(g[0])).astype(F)
    for i in range(1, 6):
        s = (p[:, 5 + i:5 + i + W] + p[:, 5 - i:5 - i + W]).astype(F)
        h = _fma32(s, g[i], h)
    v = (h[0:H] * F(g[5])).astype(F)
    for j in range(-4, 6):
        v = _fma32(h[5 + j:5 + j + H], g[abs(j)], v)
    return v


def adjoint_weights(n, g):
    """w[j + 5][q], j = -5 .. 5: what gradient pixel q of an axis of n pixels collects from p = q + j.  The tap g|j| in the interior;
    on the first (last) pixel tail[|j|] = g|j| + ... + g5 for j >= 0 (j <= 0) -- the taps the forward pass clamped onto it --; the
    sum of all eleven taps when n == 1.  tail and the total: sums of the float taps in double, rounded once."""
    g = np.asarray(g, F)
    tail = np.cumsum(g[::-1].astype(np.float64))[::-1].astype(F)
    total = F(2.0 * float(np.sum(g.astype(np.float64))) - float(g[0]))
    w = np.zeros((11, n), F)
    for j in range(-5, 6):
        w[j + 5, :] = g[abs(j)]
        w[j + 5, 0] = tail[abs(j)] if j >= 0 else 0
        if n > 1:
            w[j + 5, n - 1] = tail[abs(j)] if j <= 0 else 0
        else:
            w[j + 5, 0] = total if j == 0 else 0
    return w


def _adjoint32(v, w, axis):
    """The kernels' adjoint pass along one axis: out(q) = w(q, -5) v(q - 5), then fma(v(q + j), w(q, j), .) for j = -4 .. 5; v is
    zero outside the image."""
    if axis == 0:
        return _adjoint32(v.T, w, 1).T
    n = v.shape[1]
    p = np.pad(v, ((0, 0), (5, 5)))
    acc = (p[:, 0:n] * w[0][None, :]).astype(F)
    for t in range(1, 11):
        acc = _fma32(p[:, t:t + n], w[t][None, :], acc)
    return acc


def emulate_fp32(a, b, data_range, g_out=None):
    """(global value as float64, float32 map) as the kernels compute them, strip column by strip column; with g_out also the float32
    gradients: (value, map, dLoss/da, dLoss/db)."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    H, W = a.shape
    c1, c2 = (F(x) for x in constants(data_range))
    g = gaussian_taps().astype(F)[5:]          # centre .. edge
    cA, cB = centres(a, data_range), centres(b, data_range)
    pa, pb = np.pad(a, 5, mode="edge"), np.pad(b, 5, mode="edge")
    out = np.empty((H, W), F)
    want_grad = g_out is not None
    if want_grad:
        ga, gb = np.empty((H, W), F), np.empty((H, W), F)
        k = F(float(F(g_out)) / (float(W) * float(H)))
        wx, wy = adjoint_weights(W, g), adjoint_weights(H, g)
    two = F(2.0)
    with np.errstate(all="ignore"):
        for i, x0 in enumerate(range(0, W, STRIP_W)):
            x1 = min(x0 + STRIP_W, W)
            # the forward kernel blurs its own columns only; the gradient kernel needs the statistics 5 columns beyond them, under
            # the same centre: the whole width is blurred with this strip column's centre and the columns wanted are taken
            lo, hi = (0, W) if want_grad else (x0, x1)
            sa = (pa[:, lo:hi + 10] - cA[i]).astype(F)
            sb = (pb[:, lo:hi + 10] - cB[i]).astype(F)
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
            ca, cb = sa[5:5 + H, 5:5 + W], sb[5:5 + H, 5:5 + W]              # a', b' at the pixel
            va = ((r_a + ((two * ca).astype(F) * r_aa).astype(F)).astype(F) + (cb * r_ab).astype(F)).astype(F)
            vb = ((r_b + ((two * cb).astype(F) * r_aa).astype(F)).astype(F) + (ca * r_ab).astype(F)).astype(F)
            ga[:, x0:x1], gb[:, x0:x1] = va[:, x0:x1], vb[:, x0:x1]
    value = float(np.sum(out.astype(np.float64)) / (float(W) * float(H)))
    return (value, out, ga, gb) if want_grad else (value, out)
