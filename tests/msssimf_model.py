"""float64 model of the library's multi-scale SSIM of float32 samples and of its gradient (the definition in include/rmgr/ssim-hip.h,
rmgr_ssim_hip_*_msssimf*), and an fp32 emulation of the kernels that compute it.

The yardstick of tests/test_msssimf_cpu.py, tests/test_gpu_msssimf.py and tests/test_gpu_msssimf_content.py.  Built on tests/ssimf_model.py's blur / blur_t / constants:
the clamped 2 x 2 pyramid, cs = A2 / B2 and ssim = A1 A2 / (B1 B2) per pixel and scale, fp64 means over double(W_s) * double(H_s), the
ReLU'd weighted product with x^0 = 1, and the exact derivative: the ssimf formula per scale (its cs form on every scale but the
last) with k_s = gOut w_s MS / m_s / (W_s H_s), accumulated from the coarsest scale down through downsample_t, the ADJOINT of the
clamped box filter.  Plain numpy, no reference to the GPU code.

Model(a, b, R) caches what does not depend on the number of scales or the weights (pyramid, per-scale maps, the unit local gradients
Gt(d_mu) + 2 a Gt(d_aa) + b Gt(d_ab) of both forms: the local gradient is linear in k_s), so that a test can walk scales 1 .. 8 cheaply.

Emulation(a, b, R) restates the KERNELS' arithmetic (msssimf_kernels.hip; the strip and gradient bodies are ssim2_walk.h's multi-scale forms): the fp32 pyramid in its defined order, the centre of every
128-column strip column of EVERY scale taken from that scale's plane, the fp32 statistics and gradient of ssimf_model.emulate_fp32
with the cs form added, k_s rounded to float once, and g_s = fp32(local_s + fp32(0.25 c g_{s+1})).  What the GPU should produce up to
the order of the fp64 sums, the 1-ulp reciprocal, fma contraction and the device's pow.
"""
import numpy as np

import content_classes as C
import ssimf_model as SF
from ssimf_model import F, STRIP_W, constants, forms, gaussian_taps  # noqa: F401  (re-exported for the tests)

WANG_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_SCALES = 8

# What the fp32 emulation measures against the float64 model, the worst over every golden pair in the three forms of
# ssimf_model.forms() x {Wang's 5 scales, uniform weights at 1 .. 8 scales} (tests/test_msssimf_cpu.py pins the figures): the value,
# any per-scale mean, the gradient error over the plane's largest float64 gradient magnitude, and max|grad| * W * H * R / |gOut| on the
# pair of identical images (exact gradient 0).  The GPU tests assert 1.9 to 2.2 x these, the margin ssimf uses for what the emulation
# does not restate.
# Measured: 1.172e-6, 1.602e-6, 2.648e-4 (einstein_meanshift) and 3.648e-4.
EMU_VALUE, EMU_MEAN, EMU_GRAD, EMU_IDENT = 1.2e-6, 1.65e-6, 2.7e-4, 3.7e-4
VALUE_TOL, MEAN_TOL, GRAD_TOL, IDENT_TOL = 2.5e-6, 3.4e-6, 5.5e-4, 7.5e-4

# Sample content (tests/content_classes.py as planes; tests/test_gpu_msssimf_content.py): a plane of 300 x 40 (W x H), 4 scales with
# uniform weights, gOut = -0.75, and one scale-0 position per scale that is the centre of a strip column of that scale and of no other
# (centre_scales; tests/test_msssimf_cpu.py asserts it).
CONTENT_SHAPE, CONTENT_SCALES, CONTENT_G_OUT = (40, 300), 4, -0.75
CONTENT_WEIGHTS = (0.25,) * 4
CONTENT_POSITIONS = ((19, 192), (18, 128), (16, 256), (20, 296))          # (y, x) for scale 0, 1, 2, 3

# The classes whose emulation leaves more than 85 % of an EMU figure there, each with its OWN (value, mean, gradient) figures: measured on
# the CPU, rounded up, pinned from both sides by tests/test_msssimf_cpu.py.  These are measured limits of centring, not of the kernels'
# other arithmetic: with every sample above the range the centre is 0 and nothing is centred; a step on a strip column's edge (x = 128 k) is
# a step ON the centre sample two scales down, where the flat side is blurred at a' = -cA and E[a'^2] - mu'^2 cancels against C2; at range
# 1e-6, C1 and C2 are of order 1e-16 under samples of order 1.  The GPU bound of such a class is its figure times the family's own ratio
# TOL / EMU (class_bounds); every other class is held to VALUE_TOL, MEAN_TOL, GRAD_TOL and IDENT_TOL.
# Measured: 2.452e-6, 1.151e-5, 2.086e-4; 4.960e-6, 1.993e-5, 4.280e-6; 8.378e-7, 3.123e-6, 7.537e-5.
CLASS_EMU = {
    "offset above the range": (2.5e-6, 1.2e-5, 2.1e-4),
    "step on x = 256": (5.0e-6, 2.0e-5, 4.3e-6),
    "unit data at range 1e-6": (8.4e-7, 3.2e-6, 7.6e-5),
}


def class_bounds(name):
    """(value, per-scale mean, gradient, exact-gradient-0) bounds of a class of the catalogue on the GPU."""
    if name not in CLASS_EMU:
        return VALUE_TOL, MEAN_TOL, GRAD_TOL, IDENT_TOL
    v, m, g = CLASS_EMU[name]
    return v * (VALUE_TOL / EMU_VALUE), m * (MEAN_TOL / EMU_MEAN), g * (GRAD_TOL / EMU_GRAD), IDENT_TOL


def base_pair():
    """The catalogue's base pair on CONTENT_SHAPE: content_classes.random_pair under the seed of plane_classes."""
    return C.random_pair(CONTENT_SHAPE, 4200)


def planted_pair(pos, side, value):
    """base_pair() with `value` at `pos` of A or of B."""
    a, b = (x.copy() for x in base_pair())
    (a if side == "A" else b)[pos] = value
    return a, b


def content_figures(name, got_value, got_means, got_grads, mod, r, g_out, scales, weights):
    """What a value, (scales, 2) means and a pair of gradients leave against the float64 Model `mod`: (value error, largest per-scale mean
    error, largest gradient error over the plane's largest float64 gradient magnitude, largest max|grad| * W * H * R / |gOut| of a gradient
    whose exact value is 0 -- content_classes.grad_figures decides which)."""
    mv, mm = mod.msssim(scales, weights)
    want = mod.grad(g_out, scales, weights)
    h, w = want[0].shape
    figs = C.grad_figures(name, got_grads, want, None, abs(g_out) / (float(w) * float(h)), r)
    return abs(float(got_value) - mv), float(np.abs(np.asarray(got_means, np.float64) - mm).max()), C.worst(figs, False), C.worst(figs, True)


def scale_dims(width, height, scales):
    dims = [(width, height)]
    for _ in range(1, scales):
        w, h = dims[-1]
        dims.append(((w + 1) // 2, (h + 1) // 2))
    return dims


def scale_centres(shape, s):
    """[(y, x)] of the centre sample of every strip column of scale s of a plane of `shape` = (H, W), in that scale's coordinates:
    content_classes.plane_centres on that scale's dimensions."""
    w, h = scale_dims(shape[1], shape[0], s + 1)[s]
    return C.plane_centres((h, w))


def centre_position(shape, s, column=-1, dy=0, dx=0):
    """The scale-0 position (y, x) of a plane of `shape` = (H, W) whose 2^s block -- the scale-0 samples that pyramid pixel (y >> s,
    x >> s) of scale s averages -- lands on the centre of strip column `column` of scale s: the block's first sample moved on by
    (dy, dx) inside the block and the plane."""
    cy, cx = scale_centres(shape, s)[column]
    y, x = (cy << s) + dy, (cx << s) + dx
    assert 0 <= dy < (1 << s) and 0 <= dx < (1 << s) and y < shape[0] and x < shape[1], (shape, s, column, dy, dx)
    return y, x


def centre_scales(shape, pos, scales):
    """The scales s < `scales` at which the pyramid pixel over scale-0 position `pos` is the centre of a strip column of scale s."""
    return [s for s in range(scales) if (pos[0] >> s, pos[1] >> s) in scale_centres(shape, s)]


def _taps(h, w):
    ys, xs = np.arange((h + 1) // 2), np.arange((w + 1) // 2)
    return (np.minimum(2 * ys, h - 1), np.minimum(2 * ys + 1, h - 1)), (np.minimum(2 * xs, w - 1), np.minimum(2 * xs + 1, w - 1))


def downsample(p):
    """D: scale s -> s + 1, ((P(2x,2y) + P(2x+1,2y)) + (P(2x,2y+1) + P(2x+1,2y+1))) * 0.25, coordinates clamped to scale s; in the
    dtype of p (float64: the model; float32: every operation rounded in that order, the kernels' pyramid)."""
    (y0, y1), (x0, x1) = _taps(*p.shape)
    return ((p[np.ix_(y0, x0)] + p[np.ix_(y0, x1)]) + (p[np.ix_(y1, x0)] + p[np.ix_(y1, x1)])) * p.dtype.type(0.25)


def downsample_t(g, h, w):
    """Dt: the adjoint of D for a scale of h x w, by scatter-add: every coarse pixel gives 0.25 of itself to each of the four
    (clamped) positions it read."""
    (y0, y1), (x0, x1) = _taps(h, w)
    out = np.zeros((h, w), np.float64)
    for ys in (y0, y1):
        for xs in (x0, x1):
            np.add.at(out, (ys[:, None], xs[None, :]), 0.25 * g)
    return out


def box_adjoint_weight(n):
    """0.25 c of the definition along one axis of n pixels, as the per-pixel factor of the gather g_{s+1}(x >> 1): 2 on the last pixel
    of an odd axis (n = 1 included), else 1."""
    c = np.ones(n)
    if n % 2:
        c[n - 1] = 2.0
    return c


def pyramid(img, scales, dtype=np.float64):
    out = [np.asarray(img, dtype)]
    for _ in range(1, scales):
        out.append(downsample(out[-1]))
    return out


def check_weights(scales, weights):
    if weights is None:
        assert scales == 5, "Wang's weights are five"
        return WANG_WEIGHTS
    assert 1 <= scales <= MAX_SCALES and len(weights) == scales
    return tuple(float(w) for w in weights)


def combine(means, weights):
    """prod max(m_s, 0)^w_s with x^0 = 1; m_s = mcs_s, or mssim_s for the last scale.  A NaN mean gives NaN."""
    scales = len(weights)
    r = 1.0
    for s in range(scales):
        if weights[s] == 0.0:
            continue
        m = float(means[s][1] if s == scales - 1 else means[s][0])
        r *= (0.0 if m <= 0.0 else m) ** weights[s]
    return r


def coefficients(means, weights, g_out, dims):
    """k_s of the definition for every scale: gOut w_s MS / m_s / (double(W_s) double(H_s)); all 0 when MS = 0, 0 where w_s = 0."""
    scales = len(weights)
    ms = combine(means, weights)
    k = []
    for s in range(scales):
        m = float(means[s][1] if s == scales - 1 else means[s][0])
        if ms != 0.0 and weights[s] != 0.0:
            k.append(float(g_out) * weights[s] * ms / m / (float(dims[s][0]) * float(dims[s][1])))
        else:
            k.append(0.0)
    return k


class Model(object):
    """The float64 definition for one pair at data range R; c1 / c2 / g default to the kernels' (float-rounded constants and taps)."""

    def __init__(self, a, b, data_range, c1=None, c2=None, g=None):
        if c1 is None:
            c1, c2 = constants(data_range)
        self.c1, self.c2, self.g = c1, c2, g
        self.pa, self.pb = [np.asarray(a, np.float64)], [np.asarray(b, np.float64)]
        self._terms, self._local = {}, {}

    def planes(self, s):
        while len(self.pa) <= s:
            self.pa.append(downsample(self.pa[-1]))
            self.pb.append(downsample(self.pb[-1]))
        return self.pa[s], self.pb[s]

    def terms(self, s):
        if s not in self._terms:
            a, b = self.planes(s)
            self._terms[s] = SF._terms(a, b, self.c1, self.c2, self.g)
        return self._terms[s]

    def scale_means(self, s):
        _, _, A1, A2, B1, B2 = self.terms(s)
        n = float(A1.shape[1]) * float(A1.shape[0])
        return float(np.sum(A2 / B2) / n), float(np.sum(A1 * A2 / (B1 * B2)) / n)

    def means(self, scales):
        return np.array([self.scale_means(s) for s in range(scales)], np.float64)

    def msssim(self, scales=5, weights=None):
        """(MS as float64, (scales, 2) means {mcs, mssim})."""
        w = check_weights(scales, weights)
        m = self.means(scales)
        return combine(m, w), m

    def local(self, s, last):
        """The local gradient of scale s for k = 1, (d/da, d/db): the ssim form (last) or the cs form."""
        key = (s, bool(last))
        if key not in self._local:
            a, b = self.planes(s)
            ma, mb, A1, A2, B1, B2 = self.terms(s)
            if last:
                v = A1 * A2 / (B1 * B2)
                d_ab, d_aa = 2.0 * A1 / (B1 * B2), -v / B2
                d_mu_a = 2.0 * mb * A2 / (B1 * B2) - 2.0 * ma * v / B1 - 2.0 * ma * d_aa - mb * d_ab
                d_mu_b = 2.0 * ma * A2 / (B1 * B2) - 2.0 * mb * v / B1 - 2.0 * mb * d_aa - ma * d_ab
            else:
                cs = A2 / B2
                d_ab, d_aa = 2.0 / B2, -cs / B2
                d_mu_a = -2.0 * ma * d_aa - mb * d_ab
                d_mu_b = -2.0 * mb * d_aa - ma * d_ab
            t_aa, t_ab = SF.blur_t(d_aa, self.g), SF.blur_t(d_ab, self.g)
            self._local[key] = (SF.blur_t(d_mu_a, self.g) + 2.0 * a * t_aa + b * t_ab, SF.blur_t(d_mu_b, self.g) + 2.0 * b * t_aa + a * t_ab)
        return self._local[key]

    def grad(self, g_out, scales=5, weights=None, means=None):
        """(dLoss/da, dLoss/db) in float64 for dLoss/dMS = g_out.  means: a (scales, 2) array that forms k_s in place of the model's
        own (what rmgr_ssim_hip_enqueue_msssimf_grad is handed: the means of another pair, when this one's are NaN)."""
        w = check_weights(scales, weights)
        m = self.means(scales) if means is None else np.asarray(means, np.float64).reshape(scales, 2)
        dims = [(self.planes(s)[0].shape[1], self.planes(s)[0].shape[0]) for s in range(scales)]
        k = coefficients(m, w, g_out, dims)
        ga = gb = None
        for s in range(scales - 1, -1, -1):
            h, wd = self.planes(s)[0].shape
            if k[s] != 0.0:
                la, lb = self.local(s, s == scales - 1)
                la, lb = k[s] * la, k[s] * lb
            else:
                la, lb = np.zeros((h, wd)), np.zeros((h, wd))
            if ga is not None:
                la, lb = la + downsample_t(ga, h, wd), lb + downsample_t(gb, h, wd)
            ga, gb = la, lb
        return ga, gb


def msssim(a, b, data_range, scales=5, weights=None, c1=None, c2=None, g=None):
    """(MS-SSIM as float64, per-scale means as a (scales, 2) array of {mcs, mssim})."""
    return Model(a, b, data_range, c1, c2, g).msssim(scales, weights)


def grad(a, b, data_range, g_out, scales=5, weights=None, c1=None, c2=None, g=None):
    """(dLoss/da, dLoss/db) in float64."""
    return Model(a, b, data_range, c1, c2, g).grad(g_out, scales, weights)


# ---- fp32 emulation of msssimf_kernels.hip (ssim2_walk.h) --------------------------------------------------------------------------------------------

class _ScaleEmu(object):
    """One scale of one pair as the kernels compute it: the cs and ssim maps (float32), and per strip column the unscaled partials of
    both gradient forms, everything under that strip column's centre."""

    def __init__(self, a, b, data_range):
        self.a, self.b = a, b
        H, W = a.shape
        c1, c2 = (F(x) for x in constants(data_range))
        g = gaussian_taps().astype(F)[5:]          # centre .. edge
        self.g = g
        cA, cB = SF.centres(a, data_range), SF.centres(b, data_range)
        pa, pb = np.pad(a, 5, mode="edge"), np.pad(b, 5, mode="edge")
        self.cs, self.ssim = np.empty((H, W), F), np.empty((H, W), F)
        self.strips = []
        two, one = F(2.0), F(1.0)
        with np.errstate(all="ignore"):
            for i, x0 in enumerate(range(0, W, STRIP_W)):
                x1 = min(x0 + STRIP_W, W)
                # the gradient kernel needs the statistics 5 columns beyond the strip column, under the same centre: the whole width
                # is computed with this strip column's centre and the columns wanted are taken (as ssimf_model.emulate_fp32)
                sa = (pa - cA[i]).astype(F)
                sb = (pb - cB[i]).astype(F)
                qs = SF._fma32(sb, sb, (sa * sa).astype(F))
                x = (sa * sb).astype(F)
                mA, mB, eS, eX = SF._blur32(sa, g), SF._blur32(sb, g), SF._blur32(qs, g), SF._blur32(x, g)
                pc = (mA * mB).astype(F)
                tc = ((mA * mA).astype(F) + (mB * mB).astype(F)).astype(F)
                sS, sAB = (eS - tc).astype(F), (eX - pc).astype(F)
                uA, uB = (mA + cA[i]).astype(F), (mB + cB[i]).astype(F)
                muAB = (uA * uB).astype(F)
                tm = ((uA * uA).astype(F) + (uB * uB).astype(F)).astype(F)
                A1, A2 = SF._fma32(muAB, two, np.full_like(muAB, c1)), SF._fma32(sAB, two, np.full_like(sAB, c2))
                B1, B2 = (tm + c1).astype(F), (sS + c2).astype(F)
                n, den = (A1 * A2).astype(F), (B1 * B2).astype(F)
                r1, r2 = (one / B1).astype(F), (one / B2).astype(F)
                self.ssim[:, x0:x1] = (n * (one / den).astype(F)).astype(F)[:, x0:x1]
                self.cs[:, x0:x1] = (A2 * r2).astype(F)[:, x0:x1]
                # the ssim form (ssimf_grad_kernel)
                r12 = (r1 * r2).astype(F)
                s = (n * r12).astype(F)
                dab = ((two * A1).astype(F) * r12).astype(F)
                daa = -(s * r2).astype(F)
                f1, f2 = (A2 * r12).astype(F), (s * r1).astype(F)

                def d_mu(u_other, u_self, m_self, m_other):
                    t = ((two * u_other).astype(F) * f1).astype(F) - ((two * u_self).astype(F) * f2).astype(F)
                    t = t.astype(F) - ((two * m_self).astype(F) * daa).astype(F)
                    return (t.astype(F) - (m_other * dab).astype(F)).astype(F)
                last = (d_mu(uB, uA, mA, mB), d_mu(uA, uB, mB, mA), daa, dab)
                # the cs form
                csv = (A2 * r2).astype(F)
                cab = (two * r2).astype(F)
                caa = -(csv * r2).astype(F)
                cmA = (-((two * mA).astype(F) * caa).astype(F) - (mB * cab).astype(F)).astype(F)
                cmB = (-((two * mB).astype(F) * caa).astype(F) - (mA * cab).astype(F)).astype(F)
                self.strips.append((x0, x1, sa[5:5 + H, 5:5 + W], sb[5:5 + H, 5:5 + W], last, (cmA, cmB, caa, cab)))

    def means(self):
        n = float(self.a.shape[1]) * float(self.a.shape[0])
        return float(np.sum(self.cs.astype(np.float64)) / n), float(np.sum(self.ssim.astype(np.float64)) / n)

    def local(self, k, last):
        """The float32 local gradient (d/da, d/db) for the float coefficient k."""
        H, W = self.a.shape
        ga, gb = np.zeros((H, W), F), np.zeros((H, W), F)
        if k == 0:
            return ga, gb
        wx, wy = SF.adjoint_weights(W, self.g), SF.adjoint_weights(H, self.g)
        two = F(2.0)
        with np.errstate(all="ignore"):
            for x0, x1, ca, cb, p_last, p_cs in self.strips:
                dmA, dmB, daa, dab = p_last if last else p_cs

                def gt(v):
                    return SF._adjoint32(SF._adjoint32((k * v).astype(F), wx, 1), wy, 0)
                r_a, r_b, r_aa, r_ab = gt(dmA), gt(dmB), gt(daa), gt(dab)
                va = ((r_a + ((two * ca).astype(F) * r_aa).astype(F)).astype(F) + (cb * r_ab).astype(F)).astype(F)
                vb = ((r_b + ((two * cb).astype(F) * r_aa).astype(F)).astype(F) + (ca * r_ab).astype(F)).astype(F)
                ga[:, x0:x1], gb[:, x0:x1] = va[:, x0:x1], vb[:, x0:x1]
        return ga, gb


class Emulation(object):
    """The kernels' arithmetic for one pair at data range R."""

    def __init__(self, a, b, data_range):
        self.r = data_range
        self.pa, self.pb = [np.asarray(a, F)], [np.asarray(b, F)]
        self._scale = {}

    def scale(self, s):
        while len(self.pa) <= s:
            with np.errstate(all="ignore"):
                self.pa.append(downsample(self.pa[-1]))
                self.pb.append(downsample(self.pb[-1]))
        if s not in self._scale:
            self._scale[s] = _ScaleEmu(self.pa[s], self.pb[s], self.r)
        return self._scale[s]

    def means(self, scales):
        return np.array([self.scale(s).means() for s in range(scales)], np.float64)

    def msssim(self, scales=5, weights=None):
        w = check_weights(scales, weights)
        m = self.means(scales)
        return combine(m, w), m

    def grad(self, g_out, scales=5, weights=None, means=None):
        """(float32 dLoss/da, float32 dLoss/db): k_s from the emulation's own means (or from `means`, a (scales, 2) array), rounded to
        float once; scale by scale fp32(local + fp32(0.25 c g_{s+1}(x >> 1, y >> 1)))."""
        w = check_weights(scales, weights)
        m = self.means(scales) if means is None else np.asarray(means, np.float64).reshape(scales, 2)
        dims = [(self.scale(s).a.shape[1], self.scale(s).a.shape[0]) for s in range(scales)]
        with np.errstate(all="ignore"):
            k = [F(x) for x in coefficients(m, w, float(F(g_out)), dims)]
        ga = gb = None
        for s in range(scales - 1, -1, -1):
            la, lb = self.scale(s).local(k[s], s == scales - 1)
            if ga is not None:
                h, wd = la.shape
                c = (F(0.25) * np.outer(box_adjoint_weight(h), box_adjoint_weight(wd))).astype(F)
                iy, ix = np.arange(h) >> 1, np.arange(wd) >> 1
                with np.errstate(all="ignore"):
                    la = (la + (c * ga[np.ix_(iy, ix)]).astype(F)).astype(F)
                    lb = (lb + (c * gb[np.ix_(iy, ix)]).astype(F)).astype(F)
            ga, gb = la, lb
        return ga, gb
