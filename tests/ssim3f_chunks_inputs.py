"""The inputs of tests/test_gpu_ssim3f_chunks.py and their float64 references, in plain numpy: no GPU, no library call.  Sizes are
W x H x D; arrays are (D, H, W).

Two shapes whose volume counts make plan3f choose every chunk depth (tests/ssim3f_plan.py says which count gives which), and per shape
seven distinct seeded pairs that a launch's descriptors pick among (test_gpu_ssim3f.random_pair).  Every volume of a launch also draws its
dLoss/dS among the five values G_OUTS, independently of its pair, so that neighbours differ: a launch is then made of 35 (pair, gOut)
combinations, each of which has a one-volume launch to be compared with.  tests/test_ssim3f_plan_cpu.py holds the fp32 emulation of the
model to the GPU bounds on these very pairs.
"""
import numpy as np

import ssim3f_model as S
import ssim3f_plan as P
from test_gpu_ssim3f import random_pair

# 17 x 17 x 131: four tiles, three of them one voxel wide or high; 16 full cells and a 3-slice cell; at depth 64 the last chunk is 3 slices.
# 5 x 3 x 1000: both lateral axes shorter than the window, under deep chunks.
SHAPES = ((17, 17, 131), (5, 3, 1000))
PAIRS = 7
RANGE = 1.0
G_OUTS = (-0.75, 0.5, 1.0, -2.0, 0.25)
COUNT_CAP = 512                                           # no launch of the chunk tests holds more volumes
SEED = 20261019
LIMIT_SHAPE, LIMIT_COUNT, LIMIT_SALT = (2, 1, 3), 65537, 2  # two more volumes than one launch takes; the salt of its draw
RING_SHAPE, SF_SLOTS = (33, 17, 9), 8                     # kSfSlots of ssim_context.h
RING_COUNT = 2 * SF_SLOTS + 1


def shape_id(shape):
    return "%dx%dx%d" % tuple(shape)


_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def pairs(shape, n=PAIRS):
    """n distinct float32 pairs in [0, 1] of one shape."""
    w, h, d = shape
    return _once(("pairs", shape, n), lambda: [random_pair(shape, 10000 * w + 100 * h + d + k) for k in range(n)])


def picks(count, salt):
    """(which of the seven pairs, which of the five gOut values) each volume of a launch of `count` volumes names: the 35 combinations
    in turn, starting at one that depends on the salt, in a seeded shuffle -- 35 volumes or more name every combination, 7 or more
    every pair."""
    combo = np.random.default_rng([SEED, count, salt]).permutation((np.arange(count) + 11 * salt) % (PAIRS * len(G_OUTS)))
    return combo % PAIRS, combo % len(G_OUTS)                 # 7 and 5 are coprime: 35 consecutive numbers give every combination


def model(shape, k):
    """(value, map) of pair k in float64."""
    a, b = pairs(shape)[k]
    return _once(("model", shape, k), lambda: S.ssim(a, b, RANGE))


def model_grad(shape, k, g):
    """(dA, dB) of pair k in float64 for dLoss/dS = G_OUTS[g]."""
    a, b = pairs(shape)[k]
    return _once(("grad", shape, k, g), lambda: S.grad(a, b, RANGE, G_OUTS[g]))


def held_g(k):
    """The gOut value at which pair k's one-volume gradient is held to the model (every value takes part)."""
    return k % len(G_OUTS)


# ---- which launches: one count per chunk depth ----------------------------------------------------------------------------------------

def depth_counts(shape, cus):
    """[(count, geometry)]: for every chunk depth plan3f can give this shape, the smallest count up to COUNT_CAP that gives it, in
    ascending order of count."""
    w, h, d = shape
    seen, out = set(), []
    for n in range(1, COUNT_CAP + 1):
        geo = P.plan3f(w, h, d, n, cus)
        if geo.chunk_slices not in seen:
            seen.add(geo.chunk_slices)
            out.append((n, geo))
    return out
