"""float64 model of the library's SSIM of 9- to 16-bit samples (the definition in include/rmgr/ssim-hip.h, rmgr_ssim_hip_*_ssim16).

The yardstick of tests/test_ssim16_cpu.py and tests/test_gpu_ssim16.py: L = 2^depth - 1, C1 / C2 from L, the clamped separable 11-tap
Gaussian (sigma 1.5), the SSIM formula per pixel, the fp64 mean over double(W) * double(H).  Plain numpy, no reference to the GPU code.

c1 / c2: the kernels use the float-rounded constants (constants(depth, f32=True)); the reference's double oracle (oracle.ssim_naive_f64)
uses the double ones, which tests pass in when they tie the model to that oracle at depth 8.

emulate_fp32() restates the KERNEL's arithmetic (centre per 128-column strip column, fp32 planes, row pass then column pass in the
kernel's order, fma where the kernel fuses): what the GPU should produce up to the order of the fp64 sum and the 1-ulp reciprocal.
"""
import numpy as np

STRIP_W = 128


def constants(depth, f32=True):
    """(C1, C2) of a bit depth: (0.01 L)^2, (0.03 L)^2 with the products in double, rounded to float when f32."""
    L = float((1 << depth) - 1)
    c1, c2 = (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)
    if f32:
        return float(np.float32(c1)), float(np.float32(c2))
    return c1, c2


def gaussian_taps():
    """The true 1-D Gaussian, sigma 1.5, normalised over its 11 taps, rounded to float (the engine's taps), as float64."""
    i = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return (g / g.sum()).astype(np.float32).astype(np.float64)


def blur(p, g=None):
    """Separable 11 + 11 blur with clamped edges: same-size output, float64."""
    g = gaussian_taps() if g is None else g
    h, w = p.shape
    q = np.pad(p, 5, mode="edge")
    rows = sum(g[k] * q[:, k:k + w] for k in range(11))
    return sum(g[k] * rows[k:k + h, :] for k in range(11))


def ssim_map(a, b, depth, c1=None, c2=None, g=None):
    """Per-pixel SSIM in float64 (variances and covariance as E[xy] - mu_x mu_y on the raw samples: exact enough in float64)."""
    if c1 is None:
        c1, c2 = constants(depth)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ma, mb = blur(a, g), blur(b, g)
    s_ab = blur(a * b, g) - ma * mb
    s_s = blur(a * a + b * b, g) - (ma * ma + mb * mb)
    return (2.0 * ma * mb + c1) * (2.0 * s_ab + c2) / ((ma * ma + mb * mb + c1) * (s_s + c2))


def ssim(a, b, depth, c1=None, c2=None, g=None):
    """(global SSIM as float64 -- the fp64 sum over double(W) * double(H) --, float64 map)."""
    m = ssim_map(a, b, depth, c1, c2, g)
    return float(np.sum(m) / (float(m.shape[1]) * float(m.shape[0]))), m


# ---- fp32 emulation of ssim16_kernels.hip -------------------------------------------------------------------------------

def _fma32(x, y, z):
    """float32 fma: the product is exact in float64 (24 + 24 bits); one rounding of the sum (to float64, then float32)."""
    return (x.astype(np.float64) * np.float64(y) + z.astype(np.float64)).astype(np.float32)


def centres(img):
    """The integer centre of every 128-column strip column: the sample at (min(x0 + 64, W - 1), (H - 1) // 2)."""
    h, w = img.shape
    xs = np.minimum(np.arange(0, w, STRIP_W) + 64, w - 1)
    return np.asarray(img, np.int64)[(h - 1) // 2, xs]


def _blur32(p, g):
    """The kernel's blur of one centred fp32 plane (already padded by 5 on every side, edge-clamped): per column m the folded
    sums s_i = p[m+i] + p[m-i], h = s_0 g_0 then fma(s_i, g_i, h); per output row y the column pass adds h of rows y-5 .. y+5 in
    that order, the first one multiplied into zero."""
    H, W = p.shape[0] - 10, p.shape[1] - 10
    c = p[:, 5:5 + W]
    h = (c * np.float32(g[0])).astype(np.float32)
    for i in range(1, 6):
        s = (p[:, 5 + i:5 + i + W] + p[:, 5 - i:5 - i + W]).astype(np.float32)
        h = _fma32(s, g[i], h)
    v = (h[0:H] * np.float32(g[5])).astype(np.float32)
    for j in range(-4, 6):
        v = _fma32(h[5 + j:5 + j + H], g[abs(j)], v)
    return v


def emulate_fp32(a, b, depth):
    """(global value as float64, float32 map) as the kernel computes them, strip column by strip column."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    H, W = a.shape
    c1, c2 = (np.float32(x) for x in constants(depth))
    g = gaussian_taps().astype(np.float32)[5:]          # centre .. edge
    cA, cB = centres(a), centres(b)
    pa, pb = np.pad(a, 5, mode="edge"), np.pad(b, 5, mode="edge")
    out = np.empty((H, W), np.float32)
    for k, x0 in enumerate(range(0, W, STRIP_W)):
        x1 = min(x0 + STRIP_W, W)
        sa = (pa[:, x0:x1 + 10] - cA[k]).astype(np.float32)            # exact
        sb = (pb[:, x0:x1 + 10] - cB[k]).astype(np.float32)
        aa = (sa * sa).astype(np.float32)
        qs = (sb.astype(np.float64) * sb.astype(np.float64) + aa.astype(np.float64)).astype(np.float32)   # fma(b', b', a'^2)
        x = (sa * sb).astype(np.float32)
        mA, mB, eS, eX = _blur32(sa, g), _blur32(sb, g), _blur32(qs, g), _blur32(x, g)
        f = np.float32
        pc = (mA * mB).astype(f)
        tc = ((mA * mA).astype(f) + (mB * mB).astype(f)).astype(f)
        sS = (eS - tc).astype(f)
        sAB = (eX - pc).astype(f)
        uA, uB = (mA + f(cA[k])).astype(f), (mB + f(cB[k])).astype(f)
        muAB = (uA * uB).astype(f)
        tm = ((uA * uA).astype(f) + (uB * uB).astype(f)).astype(f)
        n = (_fma32(muAB, 2.0, np.full_like(muAB, c1)) * _fma32(sAB, 2.0, np.full_like(sAB, c2))).astype(f)
        den = ((tm + c1).astype(f) * (sS + c2).astype(f)).astype(f)
        out[:, x0:x1] = (n * (f(1.0) / den).astype(f)).astype(f)
    return float(np.sum(out.astype(np.float64)) / (float(W) * float(H))), out
