"""float64 model of the library's multi-scale SSIM of float32 VOLUMES and of its gradient (the definition in include/rmgr/ssim-hip.h,
rmgr_ssim_hip_*_msssim3f*), and an fp32 emulation of the kernels that compute it.

The yardstick of tests/test_msssim3f_cpu.py and tests/test_gpu_msssim3f.py.  Volumes are (D, H, W) arrays.  Built on
tests/ssim3f_model.py's blur / blur_t / constants: the clamped 2 x 2 x 2 pyramid, cs = A2 / B2 and ssim = A1 A2 / (B1 B2) per voxel and
scale, fp64 means over double(W_s) * double(H_s) * double(D_s), the ReLU'd weighted product with x^0 = 1 (msssimf_model.combine), and the
exact derivative: the ssim3f formula per scale (its cs form on every scale but the last) with k_s = gOut w_s MS / m_s / (W_s H_s D_s),
accumulated from the coarsest scale down through downsample_t, the ADJOINT of the clamped box filter.  Plain numpy, no reference to the
GPU code.

Model(a, b, R) caches what does not depend on the number of scales or the weights (pyramid, per-scale terms, the unit local gradients of
both forms: the local gradient is linear in k_s), so that a test can walk scales 1 .. 8 cheaply.

Emulation(a, b, R) restates the KERNELS' arithmetic (msssim3f_kernels.hip, ssim3_walk.h): the fp32 pyramid in its defined order, ONE centre
per volume at EVERY scale taken from that scale's own volume, the fp32 statistics and gradient of ssim3f_model.emulate_fp32 with the cs
form added (cs = A2 rcp(B2); d_ab = 2 rcp(B2), d_aa = -(cs rcp(B2)), d_mu = -((2 mu_a') d_aa) - (mu_b' d_ab)), k_s rounded to float once,
and g_s = fp32(local_s + fp32(0.125 c g_{s+1})), one rounding per scale.  What the GPU should produce up to the order of the fp64 sums,
the 1-ulp reciprocal and the device's pow.
"""
import numpy as np

import ssim3f_model as S
from msssimf_model import MAX_SCALES, WANG_WEIGHTS, check_weights, combine  # noqa: F401  (re-exported for the tests)
from ssim3f_model import F, FIXTURES, FORMS, _fma32, adjoint_weights, constants, gaussian_taps  # noqa: F401

# What the fp32 emulation measures against the float64 model, the worst over ssim3f_model.FIXTURES x FORMS x {Wang's 5 scales, uniform
# weights at 1 .. 8 scales} (tests/test_msssim3f_cpu.py pins the figures from both sides): the value, any per-scale mean, the gradient
# error over the volume's largest float64 gradient magnitude, and max|grad| * W * H * D * R / |gOut| on the pair of identical volumes
# (every fixture's A against itself: exact gradient 0).  The GPU tests assert TOL_FACTOR times these: the project's standing margin for
# the 1-ulp reciprocal and the order of the fp64 sums, which the emulation does not restate.
# Measured: 5.52e-6, 6.39e-6, 9.45e-5 and 4.06e-4 (the last two are ssim3f's: one scale with weight 1 is that family).
EMU_VALUE, EMU_MEAN, EMU_GRAD, EMU_IDENT = 5.6e-6, 6.5e-6, 9.5e-5, 4.1e-4
TOL_FACTOR = 2.0


def tolerances():
    """(VALUE_TOL, MEAN_TOL, GRAD_TOL, IDENT_TOL): TOL_FACTOR times the EMU_* figures."""
    return tuple(TOL_FACTOR * v for v in (EMU_VALUE, EMU_MEAN, EMU_GRAD, EMU_IDENT))


def scale_dims(width, height, depth, scales):
    """[(W_s, H_s, D_s)]: every axis is halved, rounding up; an axis that has reached 1 stays 1."""
    dims = [(width, height, depth)]
    for _ in range(1, scales):
        dims.append(tuple((n + 1) // 2 for n in dims[-1]))
    return dims


def _taps(n):
    i = np.arange((n + 1) // 2)
    return np.minimum(2 * i, n - 1), np.minimum(2 * i + 1, n - 1)


def downsample(p):
    """D: scale s -> s + 1 in the order of the definition, coordinates clamped to scale s; in the dtype of p (float64: the model;
    float32: every operation rounded in that order, the kernels' pyramid)."""
    (z0, z1), (y0, y1), (x0, x1) = _taps(p.shape[0]), _taps(p.shape[1]), _taps(p.shape[2])

    def plane(z):
        return (p[np.ix_(z, y0, x0)] + p[np.ix_(z, y0, x1)]) + (p[np.ix_(z, y1, x0)] + p[np.ix_(z, y1, x1)])
    return (plane(z0) + plane(z1)) * p.dtype.type(0.125)


def downsample_t(g, shape):
    """Dt: the adjoint of D for a scale of `shape`, by scatter-add: every coarse voxel gives 0.125 of itself to each of the eight
    (clamped) positions it read."""
    out = np.zeros(shape, np.float64)
    for zs in _taps(shape[0]):
        for ys in _taps(shape[1]):
            for xs in _taps(shape[2]):
                np.add.at(out, (zs[:, None, None], ys[None, :, None], xs[None, None, :]), 0.125 * g)
    return out


def box_adjoint_weight(n):
    """c of the definition along one axis of n voxels: 2 on the last voxel of an odd axis (n = 1 included), else 1."""
    c = np.ones(n)
    if n % 2:
        c[n - 1] = 2.0
    return c


def pyramid(vol, scales, dtype=np.float64):
    out = [np.asarray(vol, dtype)]
    for _ in range(1, scales):
        with np.errstate(all="ignore"):
            out.append(downsample(out[-1]))
    return out


def coefficients(means, weights, g_out, shapes):
    """k_s of the definition for every scale: (((gOut w_s) MS) / m_s) / (double(W_s) double(H_s) double(D_s)); all 0 when MS = 0 or
    gOut = 0, 0 where w_s = 0."""
    scales = len(weights)
    ms = combine(means, weights)
    k = []
    for s in range(scales):
        m = float(means[s][1] if s == scales - 1 else means[s][0])
        if ms != 0.0 and float(g_out) != 0.0 and weights[s] != 0.0:
            k.append(float(g_out) * weights[s] * ms / m / S.voxels(shapes[s]))
        else:
            k.append(0.0)
    return k


class Model(object):
    """The float64 definition for one pair of volumes at data range R."""

    def __init__(self, a, b, data_range):
        self.c1, self.c2 = constants(data_range)
        self.pa, self.pb = [np.asarray(a, np.float64)], [np.asarray(b, np.float64)]
        self._terms, self._local = {}, {}

    def volumes(self, s):
        while len(self.pa) <= s:
            self.pa.append(downsample(self.pa[-1]))
            self.pb.append(downsample(self.pb[-1]))
        return self.pa[s], self.pb[s]

    def terms(self, s):
        if s not in self._terms:
            a, b = self.volumes(s)
            self._terms[s] = S._terms(a, b, self.c1, self.c2, None)
        return self._terms[s]

    def scale_means(self, s):
        _, _, A1, A2, B1, B2 = self.terms(s)
        n = S.voxels(A1.shape)
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
            a, b = self.volumes(s)
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
            t_aa, t_ab = S.blur_t(d_aa), S.blur_t(d_ab)
            self._local[key] = (S.blur_t(d_mu_a) + 2.0 * a * t_aa + b * t_ab, S.blur_t(d_mu_b) + 2.0 * b * t_aa + a * t_ab)
        return self._local[key]

    def grad(self, g_out, scales=5, weights=None):
        """(dLoss/da, dLoss/db) in float64 for dLoss/dMS = g_out."""
        w = check_weights(scales, weights)
        m = self.means(scales)
        shapes = [self.volumes(s)[0].shape for s in range(scales)]
        k = coefficients(m, w, g_out, shapes)
        ga = gb = None
        for s in range(scales - 1, -1, -1):
            if k[s] != 0.0:
                la, lb = self.local(s, s == scales - 1)
                la, lb = k[s] * la, k[s] * lb
            else:
                la, lb = np.zeros(shapes[s]), np.zeros(shapes[s])
            if ga is not None:
                la, lb = la + downsample_t(ga, shapes[s]), lb + downsample_t(gb, shapes[s])
            ga, gb = la, lb
        return ga, gb


def msssim(a, b, data_range, scales=5, weights=None):
    """(MS-SSIM as float64, per-scale means as a (scales, 2) array of {mcs, mssim})."""
    return Model(a, b, data_range).msssim(scales, weights)


def grad(a, b, data_range, g_out, scales=5, weights=None):
    """(dLoss/da, dLoss/db) in float64."""
    return Model(a, b, data_range).grad(g_out, scales, weights)


# ---- fp32 emulation of msssim3f_kernels.hip ---------------------------------------------------------------------------------------------

class _ScaleEmu(object):
    """One scale of one pair as the kernels compute it: the cs and ssim maps (float32) and the unscaled partial derivatives of both
    gradient forms, everything under that scale's centre (ssim3f_model.emulate_fp32, with the cs form added)."""

    def __init__(self, a, b, data_range):
        self.a, self.b = a, b
        D, H, W = a.shape
        c1, c2 = (F(x) for x in constants(data_range))
        g = gaussian_taps().astype(F)[5:]          # centre .. edge
        self.g = g
        cA, cB = S.centre(a, data_range), S.centre(b, data_range)
        two, one = F(2.0), F(1.0)
        with np.errstate(all="ignore"):
            sa = (np.pad(a, 5, mode="edge") - cA).astype(F)
            sb = (np.pad(b, 5, mode="edge") - cB).astype(F)
            qs = _fma32(sb, sb, (sa * sa).astype(F))
            x = (sa * sb).astype(F)
            mA, mB, eS, eX = S._blur32(sa, g), S._blur32(sb, g), S._blur32(qs, g), S._blur32(x, g)
            pc = (mA * mB).astype(F)
            tc = ((mA * mA).astype(F) + (mB * mB).astype(F)).astype(F)
            sS, sAB = (eS - tc).astype(F), (eX - pc).astype(F)
            uA, uB = (mA + cA).astype(F), (mB + cB).astype(F)
            muAB = (uA * uB).astype(F)
            tm = ((uA * uA).astype(F) + (uB * uB).astype(F)).astype(F)
            A1, A2 = _fma32(muAB, two, np.full_like(muAB, c1)), _fma32(sAB, two, np.full_like(sAB, c2))
            B1, B2 = (tm + c1).astype(F), (sS + c2).astype(F)
            n, den = (A1 * A2).astype(F), (B1 * B2).astype(F)
            r1, r2 = (one / B1).astype(F), (one / B2).astype(F)
            self.ssim = (n * (one / den).astype(F)).astype(F)
            self.cs = (A2 * r2).astype(F)
            # the ssim form
            r12 = (r1 * r2).astype(F)
            s = (n * r12).astype(F)
            dab = ((two * A1).astype(F) * r12).astype(F)
            daa = -(s * r2).astype(F)
            f1, f2 = (A2 * r12).astype(F), (s * r1).astype(F)

            def d_mu(u_other, u_self, m_self, m_other):
                t = ((two * u_other).astype(F) * f1).astype(F) - ((two * u_self).astype(F) * f2).astype(F)
                t = t.astype(F) - ((two * m_self).astype(F) * daa).astype(F)
                return (t.astype(F) - (m_other * dab).astype(F)).astype(F)
            self.p_last = (d_mu(uB, uA, mA, mB), d_mu(uA, uB, mB, mA), daa, dab)
            # the cs form
            cab = (two * r2).astype(F)
            caa = -(self.cs * r2).astype(F)
            cmA = (-((two * mA).astype(F) * caa).astype(F) - (mB * cab).astype(F)).astype(F)
            cmB = (-((two * mB).astype(F) * caa).astype(F) - (mA * cab).astype(F)).astype(F)
            self.p_cs = (cmA, cmB, caa, cab)
            self.ca, self.cb = sa[5:5 + D, 5:5 + H, 5:5 + W], sb[5:5 + D, 5:5 + H, 5:5 + W]      # a', b' at the voxel

    def means(self):
        n = S.voxels(self.a.shape)
        return float(np.sum(self.cs.astype(np.float64)) / n), float(np.sum(self.ssim.astype(np.float64)) / n)

    def local(self, k, last):
        """The float32 local gradient (d/da, d/db) for the float coefficient k; +0 everywhere for k = 0, whatever the samples are."""
        D, H, W = self.a.shape
        if k == 0:
            return np.zeros((D, H, W), F), np.zeros((D, H, W), F)
        wx, wy, wz = adjoint_weights(W, self.g), adjoint_weights(H, self.g), adjoint_weights(D, self.g)
        two = F(2.0)
        dmA, dmB, daa, dab = self.p_last if last else self.p_cs
        with np.errstate(all="ignore"):
            def gt(v):
                return S._adjoint32(S._adjoint32(S._adjoint32((k * v).astype(F), wx, 2), wy, 1), wz, 0)
            r_a, r_b, r_aa, r_ab = gt(dmA), gt(dmB), gt(daa), gt(dab)
            ga = ((r_a + ((two * self.ca).astype(F) * r_aa).astype(F)).astype(F) + (self.cb * r_ab).astype(F)).astype(F)
            gb = ((r_b + ((two * self.cb).astype(F) * r_aa).astype(F)).astype(F) + (self.ca * r_ab).astype(F)).astype(F)
        return ga, gb


class Emulation(object):
    """The kernels' arithmetic for one pair of volumes at data range R."""

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

    def grad(self, g_out, scales=5, weights=None):
        """(float32 dLoss/da, float32 dLoss/db): k_s from the emulation's own means, rounded to float once; scale by scale
        fp32(local + fp32(0.125 c g_{s+1}(x >> 1, y >> 1, z >> 1)))."""
        w = check_weights(scales, weights)
        m = self.means(scales)
        shapes = [self.scale(s).a.shape for s in range(scales)]
        with np.errstate(all="ignore"):
            k = [F(x) for x in coefficients(m, w, float(F(g_out)), shapes)]
        ga = gb = None
        for s in range(scales - 1, -1, -1):
            la, lb = self.scale(s).local(k[s], s == scales - 1)
            if ga is not None:
                d, h, wd = la.shape
                cz, cy, cx = box_adjoint_weight(d), box_adjoint_weight(h), box_adjoint_weight(wd)
                c = (F(0.125) * (cz[:, None, None] * cy[None, :, None] * cx[None, None, :])).astype(F)
                ix = np.ix_(np.arange(d) >> 1, np.arange(h) >> 1, np.arange(wd) >> 1)
                with np.errstate(all="ignore"):
                    la = (la + (c * ga[ix]).astype(F)).astype(F)
                    lb = (lb + (c * gb[ix]).astype(F)).astype(F)
            ga, gb = la, lb
        return ga, gb


def emulate_fp32(a, b, data_range, scales=5, weights=None, g_out=None):
    """(value as float64, (scales, 2) means) as the kernels compute them; with g_out also the float32 gradients."""
    e = Emulation(a, b, data_range)
    v, m = e.msssim(scales, weights)
    if g_out is None:
        return v, m
    return (v, m) + e.grad(g_out, scales, weights)


def scale_sets():
    """The (scales, weights) the figures are measured at: Wang's five, and 1 .. 8 scales with uniform weights."""
    return [(5, None)] + [(n, (1.0 / n,) * n) for n in range(1, MAX_SCALES + 1)]


def measure_pair(fa, fb, r, sets=None, g_out=1.0):
    """(value, mean, grad) figures of the emulation against the model on one pair, the worst over `sets`."""
    mod, emu = Model(fa, fb, r), Emulation(fa, fb, r)
    val = mean = gr = 0.0
    for scales, w in (scale_sets() if sets is None else sets):
        gv, gm = mod.msssim(scales, w)
        ev, em = emu.msssim(scales, w)
        val, mean = max(val, abs(ev - gv)), max(mean, float(np.abs(em - gm).max()))
        for e, x in zip(emu.grad(g_out, scales, w), mod.grad(g_out, scales, w)):
            gr = max(gr, float(np.abs(e - x).max() / np.abs(x).max()))
    return val, mean, gr


def measure_ident(fa, r, sets=None, g_out=1.0):
    """max|grad| * W * H * D * R / |gOut| of the emulation on the pair (fa, fa), the worst over `sets`."""
    emu = Emulation(fa, fa, r)
    ident = 0.0
    for scales, w in (scale_sets() if sets is None else sets):
        ea, eb = emu.grad(g_out, scales, w)
        ident = max(ident, float(max(np.abs(ea).max(), np.abs(eb).max())) * S.voxels(fa.shape) * r / abs(g_out))
    return ident


def measure(manifest, fixtures=FIXTURES):
    """(value, mean, grad, ident) of the emulation against the float64 model: the worst over fixtures x FORMS x scale_sets()."""
    val = mean = gr = ident = 0.0
    for name in fixtures:
        for _, fa, fb, r in S.fixture_forms(manifest, name):
            v, m, g = measure_pair(fa, fb, r)
            val, mean, gr = max(val, v), max(mean, m), max(gr, g)
            ident = max(ident, measure_ident(fa, r))
    return val, mean, gr, ident
