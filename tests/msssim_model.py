"""float64 model of the library's multi-scale SSIM (the definition in include/rmgr/ssim-hip.h, rmgr_ssim_hip_compute_msssim_*).

The yardstick of tests/test_msssim_cpu.py and tests/test_gpu_msssim.py: clamped 2 x 2 pyramid, clamped separable 11-tap Gaussian
(sigma 1.5), cs and ssim per pixel, fp64 means per scale, ReLU'd weighted product.  Plain numpy, no reference to the GPU code.

c1 / c2: the GPU kernels use the float-rounded constants (C1_F32, C2_F32, the engine's); the reference's double oracle
(oracle.ssim_naive_f64) uses the double ones (C1_F64, C2_F64), which tests pass in when they tie the model to that oracle.
"""
import numpy as np

C1_F64 = (0.01 * 255.0) * (0.01 * 255.0)
C2_F64 = (0.03 * 255.0) * (0.03 * 255.0)
C1_F32 = float(np.float32(C1_F64))
C2_F32 = float(np.float32(C2_F64))
WANG_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_SCALES = 8


def gaussian_taps():
    """The true 1-D Gaussian, sigma 1.5, normalised over its 11 taps (float64)."""
    i = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def scale_dims(width, height, scales):
    dims = [(width, height)]
    for _ in range(1, scales):
        w, h = dims[-1]
        dims.append(((w + 1) // 2, (h + 1) // 2))
    return dims


def downsample(p):
    """Scale s -> s + 1: ((P(2x,2y) + P(2x+1,2y)) + (P(2x,2y+1) + P(2x+1,2y+1))) * 0.25, coordinates clamped to scale s."""
    h, w = p.shape
    ys = np.arange((h + 1) // 2)
    xs = np.arange((w + 1) // 2)
    y0, y1 = np.minimum(2 * ys, h - 1), np.minimum(2 * ys + 1, h - 1)
    x0, x1 = np.minimum(2 * xs, w - 1), np.minimum(2 * xs + 1, w - 1)
    return ((p[np.ix_(y0, x0)] + p[np.ix_(y0, x1)]) + (p[np.ix_(y1, x0)] + p[np.ix_(y1, x1)])) * 0.25


def pyramid(img, scales):
    out = [np.asarray(img, np.float64)]
    for _ in range(1, scales):
        out.append(downsample(out[-1]))
    return out


def blur(p, g=None):
    """Separable 11 + 11 blur with clamped edges: same-size output."""
    g = gaussian_taps() if g is None else g
    h, w = p.shape
    q = np.pad(p, 5, mode="edge")
    rows = sum(g[k] * q[:, k:k + w] for k in range(11))
    return sum(g[k] * rows[k:k + h, :] for k in range(11))


def scale_means(a, b, c1=C1_F32, c2=C2_F32):
    """(mean cs, mean ssim) of one scale, float64 throughout (centred at 128 like the kernels; it changes nothing in float64)."""
    a = np.asarray(a, np.float64) - 128.0
    b = np.asarray(b, np.float64) - 128.0
    ma, mb = blur(a), blur(b)
    s_ab = blur(a * b) - ma * mb
    s_s = blur(a * a + b * b) - (ma * ma + mb * mb)
    ua, ub = ma + 128.0, mb + 128.0
    cs = (2.0 * s_ab + c2) / (s_s + c2)
    l = (2.0 * ua * ub + c1) / (ua * ua + ub * ub + c1)
    n = float(a.size)
    return float(np.sum(cs) / n), float(np.sum(l * cs) / n)


def msssim(a, b, scales=5, weights=None, c1=C1_F32, c2=C2_F32):
    """(MS-SSIM as float64, per-scale means as a (scales, 2) array of {mcs, mssim})."""
    if weights is None:
        assert scales == 5, "Wang's weights are five"
        weights = WANG_WEIGHTS
    assert 1 <= scales <= MAX_SCALES and len(weights) == scales
    pa, pb = pyramid(a, scales), pyramid(b, scales)
    means = np.array([scale_means(pa[s], pb[s], c1, c2) for s in range(scales)], np.float64)
    return combine(means, weights), means


def combine(means, weights):
    scales = len(weights)
    r = 1.0
    for s in range(scales):
        v = means[s][1] if s == scales - 1 else means[s][0]
        r *= max(v, 0.0) ** weights[s]
    return r
