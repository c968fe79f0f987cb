"""Inputs shared by tests/test_ssimhk_cpu.py and tests/test_gpu_ssimhk.py (SSIM of float16 / bfloat16 planes under a caller-chosen
window): seeded pairs as uint16 bit patterns, and the planes and upstream gradients of the rounding test, whose input condition the CPU
module checks with the float64 model so that the GPU test cannot pass vacuously.  Sizes are W x H; arrays are (H, W)."""
import numpy as np

import halfmodel as HM

ONE_PER_RADIUS = [(3, 0.0, "uniform"), (5, 0.8, "gaussian"), (7, 0.0, "uniform"), (9, 1.5, "gaussian"), (11, 2.0, "gaussian")]


def random_pair_f(w, h, seed):
    """The float32 pair of tests/test_gpu_ssimw.py's random_pair: A uniform in [0, 1), B = A + 0.1 N(0, 1), clipped."""
    rng = np.random.default_rng(seed)
    a = rng.random((h, w), dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal((h, w)).astype(np.float32), 0, 1).astype(np.float32)
    return a, b


def random_pair(w, h, seed, enc):
    """That pair rounded into the encoding: two (H, W) uint16 arrays of bit patterns."""
    a, b = random_pair_f(w, h, seed)
    return HM.round_to(a, enc), HM.round_to(b, enc)


def widened(pairs, enc):
    return [(HM.widen(a, enc), HM.widen(b, enc)) for a, b in pairs]


# The rounding test: one 33 x 33 pair and two upstream gradients dLoss/dS.  The gradient of a mean SSIM is of order gOut / (W H) = gOut /
# 1089 per pixel.  G_SMALL leaves it around 1e-5, among the float16 subnormals (below 6.1e-5); G_LARGE takes about a third of the
# pixels past 65504, to Inf, and leaves the others normal numbers.
ROUNDING_SIZE = (33, 33)
ROUNDING_SEED = 1789
G_SMALL, G_LARGE = 2.0 ** -6, 2.0 ** 26


def rounding_pair(enc):
    return random_pair(ROUNDING_SIZE[0], ROUNDING_SIZE[1], ROUNDING_SEED, enc)


def census(u16, enc):
    """(subnormal, Inf, normal) element counts of an array of bit patterns."""
    u16 = np.asarray(u16, np.uint16)
    mag, expo = u16 & 0x7FFF, (0x7C00 if enc == HM.F16 else 0x7F80)
    sub = HM.is_subnormal(u16, enc)
    inf = mag == expo
    normal = ((mag & expo) != 0) & ((mag & expo) != expo)
    return int(sub.sum()), int(inf.sum()), int(normal.sum())
