"""The inputs of tests/test_gpu_sample_forms.py and their float64 references, in plain numpy: no GPU, no library call.

One pair per sample family and shape, drawn with the generators of the families' own GPU tests (test_gpu_ssimf.random_pair,
test_gpu_ssim16._pairs, test_gpu_ssimh.random_pair; test_gpu_msssimf.random_pair and test_gpu_ssimw.random_pair draw the same
planes as test_gpu_ssimf's) at a fixed seed, the upstream-gradient plane of the map gradient (ssimw_model.weight_planes, "normal"),
and the models' values on exactly these pixels.  tests/test_sample_forms_cpu.py holds the fp32 emulation of every model to the
GPU bounds on these inputs, so that a miss on the GPU means the kernel.
"""
import numpy as np

import halfmodel as HM
import msssimf_model as MS
import ssim16_model as M16
import ssimf_model as MF
import ssimw_model as MW
from test_gpu_ssim16 import _pairs as pairs16
from test_gpu_ssimf import random_pair as random_pair_f
from test_gpu_ssimh import random_pair as random_pair_h

SEED = 20261018
BIG, TALL = (19, 130), (300, 3)          # (H, W): 130 x 19 and 3 x 300 as W x H
SHAPES = (BIG, TALL)
RANGE = 1.0                              # data range of the float and half pairs
DEPTHS = (10, 16)
MS_CONFIGS = (("wang5", 5, None), ("uniform3", 3, (1.0 / 3, 1.0 / 3, 1.0 / 3)))
G_OUT = -0.75                            # dLoss/dS of the float gradients
EDGE = 1 << 21                           # fits16_narrow() / fitsf_narrow(), and fitsh_narrow() for the map: steps below it fit 32 bits
EDGE_H = 1 << 22                         # fitsh_narrow() for the 2-byte samples


def g_out_h(h, w):
    """dLoss/dS of the half gradients: W H, so that the rounded pixels are normal numbers (test_gpu_ssimh's choice)."""
    return float(w * h)


def _rng(h, w, salt):
    return np.random.default_rng(SEED + 100000 * salt + 1000 * w + h)


def pair_f(shape):
    """float32 pair in [0, 1]: the pair of ssimf, msssimf and the map gradient."""
    return random_pair_f(shape[0], shape[1], _rng(shape[0], shape[1], 1))


def pair_16(shape, depth):
    return pairs16(_rng(shape[0], shape[1], depth), 1, shape, depth)[0]


def pair_h(shape, enc):
    """((bit patterns a, b), (the float32 planes they stand for))."""
    return random_pair_h(shape[0], shape[1], _rng(shape[0], shape[1], 3 + HM.ENCODINGS.index(enc)), enc)


def gmap(shape):
    """The per-pixel upstream gradient of the map-gradient cases."""
    return dict(MW.weight_planes(shape[0], shape[1], seed=7))["normal"]


def crop(pair, w):
    """The first w columns of a pair, contiguous: the widths of the device-resident map layouts (130, even, and 129, odd)."""
    return tuple(np.ascontiguousarray(p[:, :w]) for p in pair)


_cache = {}


def model(key):
    """float64 references, computed once: ("ssimf", shape) -> (value, map); ("ssimf_grad", shape) -> (dA, dB);
    ("ssim16", shape, depth) -> (value, map); ("ssimw", shape) -> (dA, dB); ("msssimf", shape, name) -> (value, means);
    ("msssimf_grad", shape, name) -> (dA, dB)."""
    if key in _cache:
        return _cache[key]
    kind, shape = key[0], key[1]
    if kind == "ssim16":
        a, b = pair_16(shape, key[2])
        out = M16.ssim(a.astype(np.int64), b.astype(np.int64), key[2])
    else:
        a, b = pair_f(shape)
        if kind == "ssimf":
            out = MF.ssim(a, b, RANGE)
        elif kind == "ssimf_grad":
            out = MF.grad(a, b, RANGE, G_OUT)
        elif kind == "ssimw":
            out = MW.grad_map(a, b, RANGE, gmap(shape))
        else:
            scales, weights = dict((n, (s, w)) for n, s, w in MS_CONFIGS)[key[2]]
            if ("ms-model", shape) not in _cache:
                _cache[("ms-model", shape)] = MS.Model(a, b, RANGE)
            mod = _cache[("ms-model", shape)]
            out = mod.msssim(scales, weights) if kind == "msssimf" else mod.grad(G_OUT, scales, weights)
    _cache[key] = out
    return out


class Layout(object):
    """The index arithmetic of one column volume: column x starts at element x * step, rows lie one element apart (a slice taken
    across the slices of a volume).  Every plane sits at a row offset of its own inside the columns.  An input plane is stored four
    times -- as it is, mirrored, bottom-up and both -- so that a view read with step -step and / or stride -1 sees the SAME image, and
    one dense reference serves every reading direction.  The rows after the inputs are handed out one output plane at a time."""

    def __init__(self, dtype, step, width):
        self.dtype, self.step, self.width = np.dtype(dtype), int(step), int(width)
        self.rows, self.shapes, self.stored, self.in_rows = {}, {}, [], 0

    def add(self, name, img):
        assert img.shape[1] <= self.width and name not in self.shapes
        self.shapes[name] = img.shape
        for fy in (False, True):
            for fx in (False, True):
                self.rows[(name, fx, fy)] = self.in_rows
                self.stored.append((self.in_rows, img[::-1 if fy else 1, ::-1 if fx else 1]))
                self.in_rows += img.shape[0]
        return name

    def close(self, out_rows, gap=8):
        self.next = self.out0 = self.in_rows + gap
        self.end = self.out0 + out_rows
        assert self.end < self.step
        self.n = (self.width - 1) * self.step + self.end

    def index(self, row0, h, w):
        """Element index of every (row, column) of the h x w plane stored from row `row0`, in the buffer's own orientation."""
        return row0 + np.arange(h, dtype=np.int64)[:, None] + np.arange(w, dtype=np.int64)[None, :] * self.step

    def view(self, row0, h, w, flip_x=False, flip_y=False):
        """(element offset of the view's pixel (0, 0), step, stride) of that plane read mirrored and / or bottom-up."""
        off = row0 + ((w - 1) * self.step if flip_x else 0) + (h - 1 if flip_y else 0)
        return off, (-self.step if flip_x else self.step), (-1 if flip_y else 1)

    def claim(self, h):
        r = self.next
        self.next += h
        assert self.next <= self.end, "out of output rows"
        return r

    def build(self, fill, out_fill):
        host = np.full(self.n, fill, self.dtype)
        host[self.index(self.out0, self.end - self.out0, self.width)] = out_fill
        for row0, img in self.stored:
            host[self.index(row0, img.shape[0], img.shape[1])] = img
        return host
