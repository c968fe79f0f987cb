"""The inputs of tests/test_gpu_tall_strips.py and their float64 references, in plain numpy: no GPU, no library call.

Three launch shapes whose pair counts make the planners choose strips of many reduction cells (tests/sample_plan.py says which), and per
shape and sample type seven distinct seeded pairs that a launch's descriptors pick among: the float pairs with test_gpu_ssimw.random_pair
(pair 0 at the seed 100 W + H that tests/test_gpu_ssimk.py uses), the others with the generators of tests/sample_forms_inputs.py.
tests/test_sample_plan_cpu.py holds the fp32 emulation of every model to the GPU bounds on these very pairs.
"""
import numpy as np

import halfmodel as HM
import msssimf_model as MS
import sample_forms_inputs as IN
import ssim16_model as M16
import ssimf_model as MF
import ssimk_model as K
from test_gpu_ssimw import random_pair

# (name, W, H, pairs of the launch)
CASES = (("A", 9, 603, 1000), ("B", 9, 2115, 1000), ("C", 260, 601, 350))
SHAPES = tuple((h, w) for _, w, h, _ in CASES)            # (H, W)
GRAD_SHAPE, GRAD_COUNT = (603, 9), 300                    # the gradient launches of the windowed kernels
PAIRS = 7
RANGE = IN.RANGE
G_OUTS = (-0.75, 0.5, 1.0, -2.0, 0.25, 1.5, -1.25)        # dLoss/dS of pair k in the scalar gradient launches


def shape_id(shape):
    return "%dx%d" % (shape[1], shape[0])


_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def pairs_f(shape):
    """Seven float32 pairs in [0, 1]: ssimf, msssimf and every window."""
    h, w = shape
    return _once(("f", shape), lambda: [random_pair(w, h, 100 * w + h + k) for k in range(PAIRS)])


def pairs_16(shape, depth):
    return _once(("16", shape, depth), lambda: IN.pairs16(np.random.default_rng(IN.SEED + 1000 * shape[1] + shape[0] + 100000 * depth), PAIRS, shape, depth))


def pairs_h(shape, enc):
    """Seven times ((bit patterns a, b), (the float32 planes they stand for))."""
    def make():
        rng = np.random.default_rng(IN.SEED + 1000 * shape[1] + shape[0] + 100000 * (3 + HM.ENCODINGS.index(enc)))
        return [IN.random_pair_h(shape[0], shape[1], rng, enc) for _ in range(PAIRS)]
    return _once(("h", shape, enc), make)


def picks(count, salt):
    """Which of the seven pairs each descriptor of a launch of `count` pairs names."""
    p = np.random.default_rng(IN.SEED + salt).integers(0, PAIRS, count)
    assert len(set(p.tolist())) == PAIRS          # every pair takes part
    return p


def upstream(shape):
    """Seven per-pixel upstream gradients, one per pair: the standard-normal planes of ssimk_model.upstream_planes."""
    return _once(("up", shape), lambda: [next(K.upstream_planes(shape[0], shape[1], seed=k))[1] for k in range(PAIRS)])


# ---- float64 references, computed once ----------------------------------------------------------------------------------------------

def model_f(shape, k):
    a, b = pairs_f(shape)[k]
    return _once(("mf", shape, k), lambda: MF.ssim(a, b, RANGE))


def model_16(shape, depth, k):
    a, b = pairs_16(shape, depth)[k]
    return _once(("m16", shape, depth, k), lambda: M16.ssim(a.astype(np.int64), b.astype(np.int64), depth))


def model_ms(shape, k, scales, weights):
    a, b = pairs_f(shape)[k]
    return _once(("mms", shape, k), lambda: MS.Model(a, b, RANGE)).msssim(scales, weights)


def model_k(shape, k, window):
    a, b = pairs_f(shape)[k]
    return _once(("mk", shape, k, window), lambda: K.ssim(a, b, RANGE, window))


def model_k_grad(shape, k, window):
    """((dA, dB) for the scalar G_OUTS[k], (dA, dB) for the plane upstream(shape)[k])."""
    a, b = pairs_f(shape)[k]
    return _once(("mkg", shape, k, window), lambda: (K.grad(a, b, RANGE, G_OUTS[k], window), K.grad_map(a, b, RANGE, upstream(shape)[k], window)))
