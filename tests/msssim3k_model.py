"""float64 model of the library's multi-scale SSIM of VOLUMES under a caller-chosen window (the definition in include/rmgr/ssim-hip.h, the
rmgr_ssim_hip_*_msssim3f_win* entries), and an fp32 emulation of the kernels that compute it, on top of tests/msssim3f_model.py and
tests/ssim3k_model.py, which stay as they are.

The yardstick of tests/test_msssim3k_cpu.py and tests/test_gpu_msssim3k.py.  Volumes are (D, H, W) arrays.

Model(a, b, R, window) is msssim3f_model.Model -- its pyramid, means, weighted product, k_s and accumulation across scales through the
adjoint of the clamped box filter -- with ssim3k_model's _terms / blur_t under the window in place of the 11-tap ones: the definition with
5 replaced by the window's radius on every axis at every scale.  At the default window it returns msssim3f_model's values exactly.

Emulation(a, b, R, window) restates the KERNELS' arithmetic at the window's radius (walk_body and adjoint_body of ssim3_walk.h in their
multi-scale forms: instantiated by msssim3k_kernels.hip for R = 1 .. 4, by msssim3f_kernels.hip with the window's taps for R = 5): it is
msssim3f_model.Emulation with ssim3k_model's _blur32 / adjoint_weights / _adjoint32 at radius R.  At the default window it reproduces
msssim3f_model.Emulation bit for bit; at one scale of weight 1 it is ssim3k_model.emulate_fp32 bit for bit.
"""
import numpy as np

import msssim3f_model as M3
import ssim3f_model as S
import ssim3k_model as K3
from msssim3f_model import MAX_SCALES, WANG_WEIGHTS, pyramid  # noqa: F401  (re-exported for the tests)
from ssim3k_model import DEFAULT, FIXTURES, FORMS, WINDOWS, name_of, radius  # noqa: F401

F = np.float32
TOL_FACTOR = 2.0

# The configurations the emulation and the GPU are measured at: Wang's 5 scales; uniform weights at 1, 3 and 8 scales.
CONFIGS = ((5, None), (1, (1.0,)), (3, (1.0 / 3,) * 3), (8, (0.125,) * 8))

# What the fp32 emulation below measures against the float64 model, per window the worst over FIXTURES x FORMS x CONFIGS
# (tests/test_msssim3k_cpu.py pins the figures from both sides): the value, any per-scale mean, the gradient error over the volume's
# largest float64 gradient magnitude, and max|grad| * W * H * D * R / |gOut| on the pair of identical volumes (every fixture's A against
# itself: exact gradient 0).  The GPU tests assert TOL_FACTOR (2.0) x these: the project's standing margin for what an emulation does not
# restate -- the order of the fp64 sums, the 1-ulp reciprocal and the device's pow.
EMU = {
    # window: (EMU_VALUE, EMU_MEAN, EMU_GRAD, EMU_IDENT)
    # measured: 1.127e-5, 1.181e-5, 9.947e-5, 4.046e-4
    (3, 0.0, 'uniform'): (1.2e-05, 1.2e-05, 1.0e-04, 4.1e-04),
    # measured: 7.355e-6, 1.080e-5, 1.264e-4, 4.046e-4
    (5, 0.8, 'gaussian'): (7.4e-06, 1.1e-05, 1.3e-04, 4.1e-04),
    # measured: 1.425e-5, 1.484e-5, 2.364e-4, 5.395e-4
    (7, 0.0, 'uniform'): (1.5e-05, 1.5e-05, 2.4e-04, 5.4e-04),
    # measured: 9.922e-6, 1.042e-5, 1.388e-4, 5.416e-4
    (7, 1.5, 'gaussian'): (1.0e-05, 1.1e-05, 1.4e-04, 5.5e-04),
    # measured: 9.954e-6, 1.029e-5, 1.301e-4, 4.046e-4
    (9, 1.5, 'gaussian'): (1.0e-05, 1.1e-05, 1.4e-04, 4.1e-04),
    # measured: 9.875e-6, 1.039e-5, 2.083e-4, 4.062e-4
    (11, 2.0, 'gaussian'): (9.9e-06, 1.1e-05, 2.1e-04, 4.1e-04),
    # measured: 1.118e-5, 1.169e-5, 2.025e-4, 5.673e-4
    (11, 0.0, 'uniform'): (1.2e-05, 1.2e-05, 2.1e-04, 5.7e-04),
}
# GPU: what tests/test_gpu_msssim3k.py measured on an MI355X, the same four figures over the cases it runs (the five golden volumes in two
# forms at Wang's scales; one golden volume at 1, 3 and 8 uniform scales and with a zero weight).
GPU = {
    (3, 0.0, 'uniform'): (2.684e-06, 1.181e-05, 7.314e-05, 2.836e-04),
    (5, 0.8, 'gaussian'): (4.717e-06, 1.080e-05, 8.095e-05, 2.836e-04),
    (7, 0.0, 'uniform'): (3.448e-06, 1.484e-05, 1.203e-04, 3.782e-04),
    (7, 1.5, 'gaussian'): (2.197e-06, 1.043e-05, 5.913e-05, 2.836e-04),
    (9, 1.5, 'gaussian'): (2.771e-06, 1.029e-05, 7.935e-05, 2.836e-04),
    (11, 2.0, 'gaussian'): (1.146e-06, 1.039e-05, 6.195e-05, 3.782e-04),
    (11, 0.0, 'uniform'): (1.376e-06, 1.170e-05, 8.537e-05, 7.564e-04),
}

# The same for the odd sizes of msssim3k_inputs.odd_cases() -- volumes smaller than the window at coarse scales, down to 1 x 1 x 1 --,
# measured on those inputs at 8 uniform scales under the two windows they are run with: (value, mean, gradient); every mean that enters a
# product there is above ODD_MIN_MEAN under every window of WINDOWS.
# measured: 1.481e-7, 5.738e-7, 3.515e-5 and 8.730e-8, 3.359e-7, 2.896e-5; lowest mean 0.934
ODD_EMU = {
    (3, 0.0, 'uniform'): (1.5e-07, 5.8e-07, 3.6e-05),
    (9, 1.5, 'gaussian'): (8.8e-08, 3.4e-07, 2.9e-05),
}
ODD_MIN_MEAN = 0.9
# GPU: 1.420e-7, 5.684e-7, 3.515e-5 and 8.175e-8, 3.284e-7, 3.047e-5

# The lowest mean that enters a product (mcs, or mssim of the last scale) under any window on FIXTURES x FORMS x CONFIGS stays above this:
# no case sits near the ReLU or divides by a small m_s (tests/test_msssim3k_cpu.py asserts it; the lowest is the 3-tap box at scale 0).
MIN_MEAN = 0.5


def tolerances(window):
    """(VALUE_TOL, MEAN_TOL, GRAD_TOL, IDENT_TOL) of a window on the GPU: TOL_FACTOR times its EMU figures."""
    return tuple(TOL_FACTOR * v for v in EMU[tuple(window)])


def odd_tolerances(window):
    """(VALUE_TOL, MEAN_TOL, GRAD_TOL) of a window on the odd sizes: TOL_FACTOR times its ODD_EMU figures."""
    return tuple(TOL_FACTOR * v for v in ODD_EMU[tuple(window)])


class Model(M3.Model):
    """The float64 definition for one pair of volumes at data range R under `window`."""

    def __init__(self, a, b, data_range, window=DEFAULT):
        M3.Model.__init__(self, a, b, data_range)
        self.window = tuple(window)

    def terms(self, s):
        if s not in self._terms:
            a, b = self.volumes(s)
            self._terms[s] = K3._terms(a, b, self.c1, self.c2, self.window)
        return self._terms[s]

    def local(self, s, last):
        """msssim3f_model.Model.local with Gt the adjoint of the clamped window."""
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
            w = self.window
            t_aa, t_ab = K3.blur_t(d_aa, w), K3.blur_t(d_ab, w)
            self._local[key] = (K3.blur_t(d_mu_a, w) + 2.0 * a * t_aa + b * t_ab, K3.blur_t(d_mu_b, w) + 2.0 * b * t_aa + a * t_ab)
        return self._local[key]


def model(a, b, data_range, window=DEFAULT):
    return Model(a, b, data_range, window)


# ---- fp32 emulation of the kernels at the window's radius ------------------------------------------------------------------------------

class _ScaleEmu(M3._ScaleEmu):
    """msssim3f_model._ScaleEmu with R in place of 5: one scale of one pair as the kernels compute it under the window's taps g (centre
    first).  means() is that class's."""

    def __init__(self, a, b, data_range, g):
        self.a, self.b = a, b
        D, H, W = a.shape
        R = len(g) - 1
        c1, c2 = (F(x) for x in S.constants(data_range))
        self.g = g
        cA, cB = S.centre(a, data_range), S.centre(b, data_range)
        two, one = F(2.0), F(1.0)
        fma = M3._fma32
        with np.errstate(all="ignore"):
            sa = (np.pad(a, R, mode="edge") - cA).astype(F)
            sb = (np.pad(b, R, mode="edge") - cB).astype(F)
            qs = fma(sb, sb, (sa * sa).astype(F))
            x = (sa * sb).astype(F)
            mA, mB, eS, eX = K3._blur32(sa, g), K3._blur32(sb, g), K3._blur32(qs, g), K3._blur32(x, g)
            pc = (mA * mB).astype(F)
            tc = ((mA * mA).astype(F) + (mB * mB).astype(F)).astype(F)
            sS, sAB = (eS - tc).astype(F), (eX - pc).astype(F)
            uA, uB = (mA + cA).astype(F), (mB + cB).astype(F)
            muAB = (uA * uB).astype(F)
            tm = ((uA * uA).astype(F) + (uB * uB).astype(F)).astype(F)
            A1, A2 = fma(muAB, two, np.full_like(muAB, c1)), fma(sAB, two, np.full_like(sAB, c2))
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
            self.ca, self.cb = sa[R:R + D, R:R + H, R:R + W], sb[R:R + D, R:R + H, R:R + W]      # a', b' at the voxel

    def local(self, k, last):
        """The float32 local gradient (d/da, d/db) for the float coefficient k: ssim3k_model.apply_fp32 on this scale's terms."""
        D, H, W = self.a.shape
        if k == 0:
            return np.zeros((D, H, W), F), np.zeros((D, H, W), F)
        wx, wy, wz = K3.adjoint_weights(W, self.g), K3.adjoint_weights(H, self.g), K3.adjoint_weights(D, self.g)
        two = F(2.0)
        dmA, dmB, daa, dab = self.p_last if last else self.p_cs
        with np.errstate(all="ignore"):
            def gt(v):
                return K3._adjoint32(K3._adjoint32(K3._adjoint32((k * v).astype(F), wx, 2), wy, 1), wz, 0)
            r_a, r_b, r_aa, r_ab = gt(dmA), gt(dmB), gt(daa), gt(dab)
            ga = ((r_a + ((two * self.ca).astype(F) * r_aa).astype(F)).astype(F) + (self.cb * r_ab).astype(F)).astype(F)
            gb = ((r_b + ((two * self.cb).astype(F) * r_aa).astype(F)).astype(F) + (self.ca * r_ab).astype(F)).astype(F)
        return ga, gb


class Emulation(M3.Emulation):
    """The kernels' arithmetic for one pair of volumes at data range R under `window`: msssim3f_model.Emulation -- its pyramid, means,
    k_s and accumulation across scales -- over scales computed at the window's radius."""

    def __init__(self, a, b, data_range, window=DEFAULT):
        M3.Emulation.__init__(self, a, b, data_range)
        self.taps = K3.taps(window)

    def scale(self, s):
        while len(self.pa) <= s:
            with np.errstate(all="ignore"):
                self.pa.append(M3.downsample(self.pa[-1]))
                self.pb.append(M3.downsample(self.pb[-1]))
        if s not in self._scale:
            self._scale[s] = _ScaleEmu(self.pa[s], self.pb[s], self.r, self.taps)
        return self._scale[s]


def lowest_mean(means, weights=None):
    """The smallest mean that enters the product: mcs of every scale but the last, mssim of the last; weights given: scales with a weight."""
    scales = len(means)
    return min(float(means[s][1 if s == scales - 1 else 0]) for s in range(scales) if weights is None or weights[s] != 0.0)


def figures(got_value, got_means, got_grads, mod, scales, weights, g_out):
    """What a value, (scales, 2) means and a pair of gradients leave against the float64 Model `mod`: (value error, largest per-scale mean
    error, largest gradient error over that volume's largest float64 gradient magnitude)."""
    mv, mm = mod.msssim(scales, weights)
    want = mod.grad(g_out, scales, weights)
    gr = max(float(np.abs(np.asarray(g, np.float64) - w).max() / np.abs(w).max()) for g, w in zip(got_grads, want))
    return abs(float(got_value) - mv), float(np.abs(np.asarray(got_means, np.float64) - mm).max()), gr


def ident_figure(got_grads, shape, data_range, g_out):
    """max|grad| * W * H * D * R / |gOut| of the gradients of a pair of identical volumes (exact gradient 0)."""
    return max(float(np.abs(g).max()) for g in got_grads) * S.voxels(shape) * data_range / abs(g_out)


def measure(manifest, window, fixtures=FIXTURES, configs=CONFIGS):
    """(value, mean, grad, ident, lowest per-scale mean) of Emulation against the float64 model for one window: the worst over
    fixtures x FORMS x configs (see EMU); the lowest mean is the smallest that enters a product in any configuration."""
    v = m = gr = ident = 0.0
    lowest = 9.0
    for name in fixtures:
        for _, fa, fb, r in K3.fixture_forms(manifest, name):
            mod, emu = Model(fa, fb, r, window), Emulation(fa, fb, r, window)
            same = Emulation(fa, fa, r, window)
            for scales, w in configs:
                ev, em = emu.msssim(scales, w)
                fv, fm, fg = figures(ev, em, emu.grad(1.0, scales, w), mod, scales, w, 1.0)
                v, m, gr = max(v, fv), max(m, fm), max(gr, fg)
                ident = max(ident, ident_figure(same.grad(1.0, scales, w), fa.shape, r, 1.0))
                lowest = min(lowest, lowest_mean(mod.means(scales)))
    return v, m, gr, ident, lowest


def measure_odd(window, cases, scales=8, g_out=-0.75):
    """(value, mean, grad, lowest mean that enters a product) of Emulation against the float64 model over `cases`
    (msssim3k_inputs.odd_cases()) at `scales` uniform scales."""
    v = m = gr = 0.0
    lowest = 9.0
    w = (1.0 / scales,) * scales
    for _, a, b, r in cases:
        mod, emu = Model(a, b, r, window), Emulation(a, b, r, window)
        ev, em = emu.msssim(scales, w)
        fv, fm, fg = figures(ev, em, emu.grad(g_out, scales, w), mod, scales, w, g_out)
        v, m, gr = max(v, fv), max(m, fm), max(gr, fg)
        lowest = min(lowest, lowest_mean(mod.means(scales)))
    return v, m, gr, lowest
