"""float64 model of the library's multi-scale SSIM under a caller-chosen window (the definition in include/rmgr/ssim-hip.h, the
rmgr_ssim_hip_*_msssimf_win* entries), and an fp32 emulation of the kernels that compute it, on top of tests/msssimf_model.py and
tests/ssimk_model.py, which stay as they are.

The yardstick of tests/test_msssimk_cpu.py and tests/test_gpu_msssimk.py.

model(a, b, R, window) is msssimf_model.Model itself: that class already is the definition for finite samples under any taps of up to 11
(blur and blur_t clamp, and a tap of 0 reads nothing), so the window's float32 taps, widened and zero-padded to 11, make it the definition
with 5 replaced by the window's radius at every scale.  At the default window it returns msssimf_model's values exactly.

Emulation(a, b, R, window) restates the KERNELS' arithmetic at the window's radius (strip_body and grad_body of ssim2_walk.h in their
multi-scale forms: instantiated by msssimk_kernels.hip for R = 1 .. 4, by msssimf_kernels.hip with the window's taps for R = 5): it is
msssimf_model.Emulation with ssimk_model's _blur32 / adjoint_weights / _adjoint32 in place of the 5-tap ones.  At the default window it
reproduces msssimf_model.Emulation bit for bit.
"""
import numpy as np

import msssimf_model as MF
import ssimf_model as SF
import ssimk_model as SK
from msssimf_model import WANG_WEIGHTS  # noqa: F401  (re-exported for the tests)
from ssimk_model import DEFAULT, FIXTURES, FORMS, TOL_FACTOR, WINDOWS, name_of, radius  # noqa: F401

F = np.float32

# The configurations the emulation and the GPU are measured at: Wang's 5 scales; uniform weights at 1, 3 and 8 scales.
CONFIGS = ((5, None), (1, (1.0,)), (3, (1.0 / 3,) * 3), (8, (0.125,) * 8))

# What the fp32 emulation below measures against the float64 model, per window the worst over FIXTURES x FORMS x CONFIGS
# (tests/test_msssimk_cpu.py pins the figures from both sides): the value, any per-scale mean, the gradient error over the plane's largest
# float64 gradient magnitude, and max|grad| * W * H * R / |gOut| on the pair of identical images (every fixture's A against itself: exact
# gradient 0).  The GPU tests assert TOL_FACTOR (2.0) x these: the project's standing margin for what an emulation does not restate -- the
# order of the fp64 sums, the 1-ulp reciprocal, contraction and the device's pow.
# GPU: what tests/test_gpu_msssimk.py measured on an MI355X for the same cases, the same four figures.
EMU = {
    # window: (EMU_VALUE, EMU_MEAN, EMU_GRAD, EMU_IDENT)
    # measured: 2.652e-6, 2.652e-6, 7.330e-5, 3.662e-4
    (3, 0.0, 'uniform'): (2.7e-06, 2.7e-06, 7.4e-05, 3.7e-04),
    # measured: 1.489e-6, 1.489e-6, 9.228e-5, 2.441e-4
    (5, 0.8, 'gaussian'): (1.5e-06, 1.5e-06, 9.3e-05, 2.5e-04),
    # measured: 2.308e-6, 2.308e-6, 5.857e-5, 3.817e-4
    (7, 0.0, 'uniform'): (2.4e-06, 2.4e-06, 5.9e-05, 3.9e-04),
    # measured: 6.676e-7, 6.676e-7, 5.284e-5, 3.357e-4
    (7, 1.5, 'gaussian'): (6.7e-07, 6.7e-07, 5.3e-05, 3.4e-04),
    # measured: 1.377e-6, 1.377e-6, 5.416e-5, 4.315e-4
    (9, 1.5, 'gaussian'): (1.4e-06, 1.4e-06, 5.5e-05, 4.4e-04),
    # measured: 5.488e-7, 6.545e-7, 4.429e-5, 3.662e-4
    (11, 2.0, 'gaussian'): (5.5e-07, 6.6e-07, 4.5e-05, 3.7e-04),
    # measured: 1.195e-6, 1.195e-6, 5.193e-5, 7.279e-4
    (11, 0.0, 'uniform'): (1.2e-06, 1.2e-06, 5.2e-05, 7.3e-04),
}
GPU = {
    (3, 0.0, 'uniform'): (2.647e-06, 2.647e-06, 7.519e-05, 2.441e-04),
    (5, 0.8, 'gaussian'): (1.488e-06, 1.485e-06, 9.185e-05, 2.441e-04),
    (7, 0.0, 'uniform'): (2.325e-06, 2.303e-06, 6.008e-05, 7.054e-04),
    (7, 1.5, 'gaussian'): (6.853e-07, 6.637e-07, 5.222e-05, 3.591e-04),
    (9, 1.5, 'gaussian'): (1.352e-06, 1.373e-06, 4.850e-05, 4.369e-04),
    (11, 2.0, 'gaussian'): (5.319e-07, 6.584e-07, 4.404e-05, 3.242e-04),
    (11, 0.0, 'uniform'): (1.184e-06, 1.190e-06, 4.781e-05, 6.038e-04),
}

# The same for the odd sizes of msssimk_inputs.odd_cases() -- planes smaller than the window at coarse scales, down to 1 x 1 --, measured on
# those inputs under the two windows they are run with: (value, mean, gradient); every mean that enters a product there is above 0.7.
# measured: 3.514e-6, 4.189e-6, 8.833e-5 and 2.869e-6, 3.956e-6, 7.090e-5
ODD_EMU = {
    (3, 0.0, 'uniform'): (3.6e-06, 4.2e-06, 8.9e-05),
    (9, 1.5, 'gaussian'): (2.9e-06, 4.0e-06, 7.1e-05),
}
ODD_MIN_MEAN = 0.7
# GPU: 3.519e-6, 4.184e-6, 8.833e-5 and 2.839e-6, 3.950e-6, 7.090e-5

# The lowest per-scale mean (mcs or mssim) of any window on FIXTURES x FORMS at 5 and 8 scales stays above this: no case sits near the ReLU
# or divides by a small m_s (tests/test_msssimk_cpu.py asserts it).
MIN_MEAN = 0.53


def tolerances(window):
    """(VALUE_TOL, MEAN_TOL, GRAD_TOL, IDENT_TOL) of a window on the GPU: TOL_FACTOR times its EMU figures."""
    return tuple(TOL_FACTOR * v for v in EMU[tuple(window)])


def padded_taps(window):
    """The window's 2R + 1 float32 taps, widened to float64, zero-padded to the 11 taps msssimf_model / ssimf_model take."""
    g = SK.full_taps(window)
    pad = 5 - radius(window)
    return np.concatenate([np.zeros(pad), g, np.zeros(pad)])


def model(a, b, data_range, window=DEFAULT):
    """The float64 definition for one pair under `window`: msssimf_model.Model with the window's taps."""
    return MF.Model(a, b, data_range, g=padded_taps(window))


# ---- fp32 emulation of the kernels at the window's radius ------------------------------------------------------------------------------

class _ScaleEmu(MF._ScaleEmu):
    """msssimf_model._ScaleEmu with R in place of 5: one scale of one pair as the kernels compute it under the window's taps g (centre
    first)."""

    def __init__(self, a, b, data_range, g):
        self.a, self.b = a, b
        H, W = a.shape
        R = len(g) - 1
        c1, c2 = (F(x) for x in SF.constants(data_range))
        self.g = g
        cA, cB = SF.centres(a, data_range), SF.centres(b, data_range)
        pa, pb = np.pad(a, R, mode="edge"), np.pad(b, R, mode="edge")
        self.cs, self.ssim = np.empty((H, W), F), np.empty((H, W), F)
        self.strips = []
        two, one = F(2.0), F(1.0)
        fma = SF._fma32
        with np.errstate(all="ignore"):
            for i, x0 in enumerate(range(0, W, SF.STRIP_W)):
                x1 = min(x0 + SF.STRIP_W, W)
                # the gradient kernel needs the statistics R columns beyond the strip column, under the same centre: the whole width
                # is computed with this strip column's centre and the columns wanted are taken (as ssimk_model.emulate_fp32)
                sa = (pa - cA[i]).astype(F)
                sb = (pb - cB[i]).astype(F)
                qs = fma(sb, sb, (sa * sa).astype(F))
                x = (sa * sb).astype(F)
                mA, mB, eS, eX = SK._blur32(sa, g), SK._blur32(sb, g), SK._blur32(qs, g), SK._blur32(x, g)
                pc = (mA * mB).astype(F)
                tc = ((mA * mA).astype(F) + (mB * mB).astype(F)).astype(F)
                sS, sAB = (eS - tc).astype(F), (eX - pc).astype(F)
                uA, uB = (mA + cA[i]).astype(F), (mB + cB[i]).astype(F)
                muAB = (uA * uB).astype(F)
                tm = ((uA * uA).astype(F) + (uB * uB).astype(F)).astype(F)
                A1, A2 = fma(muAB, two, np.full_like(muAB, c1)), fma(sAB, two, np.full_like(sAB, c2))
                B1, B2 = (tm + c1).astype(F), (sS + c2).astype(F)
                n, den = (A1 * A2).astype(F), (B1 * B2).astype(F)
                r1, r2 = (one / B1).astype(F), (one / B2).astype(F)
                self.ssim[:, x0:x1] = (n * (one / den).astype(F)).astype(F)[:, x0:x1]
                self.cs[:, x0:x1] = (A2 * r2).astype(F)[:, x0:x1]
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
                last = (d_mu(uB, uA, mA, mB), d_mu(uA, uB, mB, mA), daa, dab)
                # the cs form
                csv = (A2 * r2).astype(F)
                cab = (two * r2).astype(F)
                caa = -(csv * r2).astype(F)
                cmA = (-((two * mA).astype(F) * caa).astype(F) - (mB * cab).astype(F)).astype(F)
                cmB = (-((two * mB).astype(F) * caa).astype(F) - (mA * cab).astype(F)).astype(F)
                self.strips.append((x0, x1, sa[R:R + H, R:R + W], sb[R:R + H, R:R + W], last, (cmA, cmB, caa, cab)))

    def local(self, k, last):
        """The float32 local gradient (d/da, d/db) for the float coefficient k."""
        H, W = self.a.shape
        ga, gb = np.zeros((H, W), F), np.zeros((H, W), F)
        if k == 0:
            return ga, gb
        wx, wy = SK.adjoint_weights(W, self.g), SK.adjoint_weights(H, self.g)
        two = F(2.0)
        with np.errstate(all="ignore"):
            for x0, x1, ca, cb, p_last, p_cs in self.strips:
                dmA, dmB, daa, dab = p_last if last else p_cs

                def gt(v):
                    return SK._adjoint32(SK._adjoint32((k * v).astype(F), wx, 1), wy, 0)
                r_a, r_b, r_aa, r_ab = gt(dmA), gt(dmB), gt(daa), gt(dab)
                va = ((r_a + ((two * ca).astype(F) * r_aa).astype(F)).astype(F) + (cb * r_ab).astype(F)).astype(F)
                vb = ((r_b + ((two * cb).astype(F) * r_aa).astype(F)).astype(F) + (ca * r_ab).astype(F)).astype(F)
                ga[:, x0:x1], gb[:, x0:x1] = va[:, x0:x1], vb[:, x0:x1]
        return ga, gb


class Emulation(MF.Emulation):
    """The kernels' arithmetic for one pair at data range R under `window`: msssimf_model.Emulation -- its pyramid, means, k_s and
    accumulation across scales -- over scales computed at the window's radius."""

    def __init__(self, a, b, data_range, window=DEFAULT):
        MF.Emulation.__init__(self, a, b, data_range)
        self.taps = SK.taps(window)

    def scale(self, s):
        while len(self.pa) <= s:
            with np.errstate(all="ignore"):
                self.pa.append(MF.downsample(self.pa[-1]))
                self.pb.append(MF.downsample(self.pb[-1]))
        if s not in self._scale:
            self._scale[s] = _ScaleEmu(self.pa[s], self.pb[s], self.r, self.taps)
        return self._scale[s]


def figures(got_value, got_means, got_grads, mod, scales, weights, g_out):
    """What a value, (scales, 2) means and a pair of gradients leave against the float64 Model `mod`: (value error, largest per-scale mean
    error, largest gradient error over that plane's largest float64 gradient magnitude)."""
    mv, mm = mod.msssim(scales, weights)
    want = mod.grad(g_out, scales, weights)
    gr = max(float(np.abs(np.asarray(g, np.float64) - w).max() / np.abs(w).max()) for g, w in zip(got_grads, want))
    return abs(float(got_value) - mv), float(np.abs(np.asarray(got_means, np.float64) - mm).max()), gr


def ident_figure(got_grads, shape, data_range, g_out):
    """max|grad| * W * H * R / |gOut| of the gradients of a pair of identical images (exact gradient 0)."""
    return max(float(np.abs(g).max()) for g in got_grads) * shape[0] * shape[1] * data_range / abs(g_out)


def measure(manifest, window, fixtures=FIXTURES, configs=CONFIGS):
    """(value, mean, grad, ident, lowest per-scale mean) of Emulation against the float64 model for one window: the worst over
    fixtures x FORMS x configs (see EMU); the lowest mean is taken over the configurations of 5 and 8 scales."""
    v = m = gr = ident = 0.0
    lowest = 9.0
    for name in fixtures:
        for _, fa, fb, r in SK.fixture_forms(manifest, name):
            mod, emu = model(fa, fb, r, window), Emulation(fa, fb, r, window)
            same = Emulation(fa, fa, r, window)
            for scales, w in configs:
                ev, em = emu.msssim(scales, w)
                fv, fm, fg = figures(ev, em, emu.grad(1.0, scales, w), mod, scales, w, 1.0)
                v, m, gr = max(v, fv), max(m, fm), max(gr, fg)
                ident = max(ident, ident_figure(same.grad(1.0, scales, w), fa.shape, r, 1.0))
                if scales in (5, 8):
                    mm = mod.means(scales)
                    lowest = min(lowest, min(float(mm[s][1 if s == scales - 1 else 0]) for s in range(scales)))
    return v, m, gr, ident, lowest


def measure_odd(window, cases):
    """(value, mean, grad, lowest mean that enters a product) of Emulation against the float64 model over `cases`
    (msssimk_inputs.odd_cases()) at gOut = -0.75 and uniform weights."""
    v = m = gr = 0.0
    lowest = 9.0
    for _, _, configs, a, b, r in cases:
        mod, emu = model(a, b, r, window), Emulation(a, b, r, window)
        for scales in configs:
            w = (1.0 / scales,) * scales
            ev, em = emu.msssim(scales, w)
            fv, fm, fg = figures(ev, em, emu.grad(-0.75, scales, w), mod, scales, w, -0.75)
            v, m, gr = max(v, fv), max(m, fm), max(gr, fg)
            mm = mod.means(scales)
            lowest = min(lowest, min(float(mm[s][1 if s == scales - 1 else 0]) for s in range(scales)))
    return v, m, gr, lowest
