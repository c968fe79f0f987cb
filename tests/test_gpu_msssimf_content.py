"""GPU: 2-D multi-scale SSIM of float32 samples and its gradient (msssimf_kernels.hip: the kFormMulti / kMsUp / kMsLast forms of
ssim2_walk.h) against the float64 model (tests/msssimf_model.py) BY SAMPLE CONTENT: the catalogue of tests/content_classes.py as planes --
the classes of tests/test_gpu_ssimf_content.py -- and one bad sample at the centre of a strip column of EVERY scale.  Sizes are W x H;
arrays are (H, W).

Shape.  300 x 40 at 4 scales with uniform weights and gOut = -0.75.  Per scale, its plane, its 128-column strip columns and their centre
samples (x, y), each on that scale's own plane:
    scale 0   300 x 40   3 strip columns   (64, 19) (192, 19) (299, 19)
    scale 1   150 x 20   2                 (64, 9) (149, 9)
    scale 2    75 x 10   1                 (64, 4)
    scale 3    38 x 5    1                 (37, 2)
The catalogue's centre classes alter (299, 19), the last strip column's centre of scale 0, and its x step lies on x = 256.  The four
positions of msssimf_model.CONTENT_POSITIONS are scale-0 samples whose 2^s block is the centre of a strip column of scale s and of no
other scale: (192, 19), (128, 18) -> (64, 9), (256, 16) -> (64, 4), (296, 20) -> (37, 2).

Bounds.  msssimf_model.class_bounds: VALUE_TOL, MEAN_TOL, GRAD_TOL and IDENT_TOL, the family's own, for every class but the three of
msssimf_model.CLASS_EMU, whose emulation alone leaves more than 85 % of an EMU figure on this shape; those are held to their own emulated
figures times the family's ratio TOL / EMU.  tests/test_msssimf_cpu.py holds the conditions on the CPU: the figures, m_s >= 0.2, the
positions, and that a NaN reaches in the emulation exactly as far as in the model.  Where the exact gradient is 0 the figure is
max|grad| W H R / |gOut| (content_classes.grad_figures).  A 1e15 sample overflows float32 products near it: its gradients are compared
outside the exclusion, the model's NaN set with a NaN at the same position; value and means are compared whole.  The MI355X measured
(value, mean, gradient) 2.45e-6, 1.15e-5, 2.09e-4 on `offset above the range`, 4.96e-6, 1.99e-5, 4.28e-6 on `step on x = 256` and
8.34e-7, 3.12e-6, 7.35e-5 on `unit data at range 1e-6` -- the emulation's figures --, at most 5.8e-8, 2.0e-7 and 8.4e-6 on every other
finite class (6.6e-7 on the means of `anticorrelated`), and 3.6e-7, 1.3e-6 and 8.4e-6 with a bad sample at a centre; the module runs in about a second.

Do the tests bite?  Checked on the emulation (msssimf_model._ScaleEmu's centres altered on scales >= 1, never committed):
 - the `<= range` select removed on scales >= 1: every 1e15, NaN and Inf case at the centres of scales 1, 2 and 3 fails, on A and on
   B -- the 1e15 means are off by 1e14 x EMU_MEAN, the NaN set grows from 6720 to 10240 pixels of 12000 at scale 1 and to the whole plane
   at scales 2 and 3; the cases at scale 0's centre and every finite class pass (`offset above the range` and `unit data at range 1e-6`
   drop to 0.2 of EMU: nothing upper-bounded can see that);
 - scale s centred by the sample of SCALE 0's plane at scale s's centre coordinates: NO test fails, and none can.  The sample read is
   an ordinary one, or is replaced by 0: any centre within the range gives the same mathematics, so a centre from the wrong plane only
   changes rounding (`step on x = 256` drops from 12.1 to 0.09 of EMU_MEAN -- the step then misses the centre sample).  The CPU pin of
   CLASS_EMU from below sees it in the emulation; on the GPU only the kernels' bit identities could (tests/test_gpu_sample_forms.py);
 - cA and cB exchanged on scales >= 1: NO test fails either, for the same reason: both stay within the range (largest figure 1.7 of
   EMU_MEAN, the 1e15 on A at scale 3's centre, under MEAN_TOL).
So these tests pin the select of every scale and the reach of a bad sample; the position of a coarse scale's centre is pinned only by
bits, as tests/test_gpu_ssimf_content.py found for the single scale.
"""
import time

import numpy as np
import pytest

import content_classes as C
import msssimf_model as M
import ssimf_model as SF
from test_gpu_msssimf import DevicePairs, bits

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]     # the float64 model meets Inf - Inf on purpose

SHAPE, SCALES, WEIGHTS, G_OUT = M.CONTENT_SHAPE, M.CONTENT_SCALES, M.CONTENT_WEIGHTS, M.CONTENT_G_OUT
CLASSES = [c for c in C.plane_classes(SHAPE) if c[0] not in C.HUGE_CLASSES and c[0] not in C.NONFINITE_CLASSES]
FINITE = [c[0] for c in CLASSES if c[0] != "anticorrelated"]
BAD = (("1e15", np.float32(C.HUGE)), ("NaN", np.float32(np.nan)), ("Inf", np.float32(np.inf)))
WORST = {}

_models = {}


@pytest.fixture(scope="module", autouse=True)
def module_report():
    t0 = time.time()
    yield
    print("\nmsssimf content: %.1f s; largest figure against its bound, per class of CLASS_EMU:" % (time.time() - t0))
    for name in M.CLASS_EMU:
        if name in WORST:
            print("  %-26s value %.3g (%.3g), mean %.3g (%.3g), gradient %.3g (%.3g)" % ((name,) + tuple(x for p in zip(WORST[name], M.class_bounds(name)) for x in p)))


def model(key, a, b, r):
    """The float64 model of a pair, made once and left unchanged."""
    if key not in _models:
        _models[key] = M.Model(a, b, r)
    return _models[key]


def same(x, y):
    """The same bit patterns, NaN compared as NaN."""
    x, y = np.asarray(x), np.asarray(y)
    nx, ny = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(bits(x[~nx]), bits(y[~ny]))


def launch(ctx, pairs, r, g_out, clean=None):
    """(values, means, [(dA, dB)]) of `pairs` in ONE forward and ONE backward launch.  clean: the (scales, 2) means handed to the backward
    for every pair whose own are NaN."""
    dp = DevicePairs(ctx, pairs)
    v, m = dp.forward(r, SCALES, WEIGHTS)
    handed = None
    if clean is not None:
        handed = m.copy()
        for i in range(len(pairs)):
            if np.isnan(m[i]).any():
                handed[i] = clean
    g = dp.grads(r, g_out, SCALES, WEIGHTS, means=handed)
    dp.free()
    return v, m, g


def clean_means(ctx):
    """The device's means of the base pair."""
    _, m, _ = launch(ctx, [M.base_pair()], 1.0, [G_OUT])
    assert np.all(np.isfinite(m[0]))
    return m[0]


def test_the_base_pair_and_the_positions_are_the_catalogues():
    a, b = M.base_pair()
    _, ca, cb, _, _ = C.named(C.plane_classes(SHAPE), "centre above the range (A)")
    where = C.plane_centres(SHAPE)[-1]
    assert where == (19, 299) and ca[where] == np.float32(C.ABOVE) and np.array_equal(cb, b)
    ca[where] = a[where]
    assert np.array_equal(ca, a)
    for s, pos in enumerate(M.CONTENT_POSITIONS):
        assert M.centre_scales(SHAPE, pos, SCALES) == [s]


@pytest.mark.parametrize("name", FINITE)
def test_every_finite_class_against_the_model(gpu_ctx, name):
    _, a, b, r, _ = C.named(CLASSES, name)
    v, m, g = launch(gpu_ctx, [(a, b)], r, [G_OUT])
    figs = M.content_figures(name, v[0], m[0], g[0], model(name, a, b, r), r, G_OUT, SCALES, WEIGHTS)
    tol = M.class_bounds(name)
    print("300x40 %s: value %.3g (%.3g), per-scale means %.3g (%.3g), gradients %.3g (%.3g), where the exact gradient is 0 %.3g (%.3g)"
          % ((name,) + tuple(x for p in zip(figs, tol) for x in p)))
    WORST[name] = figs[:3]
    assert figs[0] <= tol[0] and figs[1] <= tol[1], (name, figs, tol)
    assert figs[2] <= tol[2] and figs[3] <= tol[3], (name, figs, tol)


def test_anticorrelated_is_the_relu_case(gpu_ctx):
    _, a, b, r, _ = C.named(CLASSES, "anticorrelated")
    v, m, g = launch(gpu_ctx, [(a, b)], r, [G_OUT])
    mm = model("anticorrelated", a, b, r).means(SCALES)
    dm = float(np.abs(m[0] - mm).max())
    print("300x40 anticorrelated: value %r, per-scale means %.3g (%.3g), mcs %s" % (float(v[0]), dm, M.MEAN_TOL, m[0][:, 0]))
    assert bits(v)[0] == 0                                                  # +0, not -0
    assert dm <= M.MEAN_TOL and np.all(m[0][:, 0] < 0) and np.all(mm[:, 0] < 0)
    assert not bits(g[0][0]).any() and not bits(g[0][1]).any()              # +0 everywhere, bit for bit


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("scale", range(SCALES))
def test_a_huge_nan_or_inf_sample_at_the_centre_of_one_scale(gpu_ctx, scale, side):
    """The sample is the centre of a strip column of `scale` alone, so that centre is 0 and the sample behaves like any other.  1e15:
    value and means at the family's bounds, the gradients finite and at GRAD_TOL outside the exclusion.  NaN and Inf: the value and every
    mean are NaN; with the clean pair's device means the gradients are NaN exactly where the model's are, and at GRAD_TOL elsewhere."""
    pos = M.CONTENT_POSITIONS[scale]
    clean = clean_means(gpu_ctx)
    planes = [M.planted_pair(pos, side, val) for _, val in BAD]
    mods = [model((scale, side, what), a, b, 1.0) for (what, _), (a, b) in zip(BAD, planes)]
    reach = np.isnan(mods[1].grad(G_OUT, SCALES, WEIGHTS, means=clean)[0])
    assert reach.any() and not reach.all()
    for (what, _), pair, mod in zip(BAD, planes, mods):
        v, m, g = launch(gpu_ctx, [pair], 1.0, [G_OUT], clean)
        if what == "1e15":
            mv, mm = mod.msssim(SCALES, WEIGHTS)
            want = mod.grad(G_OUT, SCALES, WEIGHTS)
            dv, dm = abs(v[0] - mv), float(np.abs(m[0] - mm).max())
            assert dv <= M.VALUE_TOL and dm <= M.MEAN_TOL, (scale, side, what, dv, dm)
            keep = ~reach
        else:
            assert np.isnan(v[0]) and np.isnan(m[0]).all(), (scale, side, what, v, m)
            want = mod.grad(G_OUT, SCALES, WEIGHTS, means=clean)
            dv = dm = float("nan")
            keep = ~np.isnan(want[0])
            assert np.array_equal(~keep, reach)
        errs = []
        for got, wnt in zip(g[0], want):
            assert np.all(np.isfinite(got[keep])) and np.all(np.isfinite(wnt[keep])), (scale, side, what)
            if what != "1e15":
                assert np.array_equal(np.isnan(wnt), ~keep) and np.array_equal(np.isnan(got), ~keep), (scale, side, what, int(np.isnan(got).sum()), int((~keep).sum()))
            errs.append(float(np.abs(got - wnt)[keep].max() / np.abs(wnt[keep]).max()))
        print("300x40 %s at %r, the centre of scale %d, on %s: value %.3g (%.3g), means %.3g (%.3g), gradients outside %d pixels %.3g %.3g (%.3g)"
              % (what, pos, scale, side, dv, M.VALUE_TOL, dm, M.MEAN_TOL, int((~keep).sum()), errs[0], errs[1], M.GRAD_TOL))
        assert max(errs) <= M.GRAD_TOL, (scale, side, what, errs)


def selected_centres(a, b):
    """Every scale's strip-column centres of A and of B as the kernels select them, NaN-free, as one tuple."""
    emu = M.Emulation(a, b, 1.0)
    emu.scale(SCALES - 1)
    return tuple(float(c) for s in range(SCALES) for p in (emu.pa[s], emu.pb[s]) for c in SF.centres(p, 1.0))


def test_one_launch_of_every_class_and_centre_has_the_bits_of_the_lone_launches(gpu_ctx):
    """ONE launch holds one plane of each class of data range 1 (18 pairs) and the eight planes with a bad sample at the centre of one
    scale on A or on B (1e15, NaN, Inf in turn), interleaved so that neighbours differ in some scale's selected centre.  Every value,
    mean and gradient has the bits of the pair launched alone (NaN compared as NaN), again after launches at the other ranges."""
    ctx = gpu_ctx
    classes = C.plane_classes(SHAPE)
    unit = [(c[0], c[1], c[2]) for c in classes if c[3] == 1.0]
    others = [c for c in classes if c[3] != 1.0]
    planted = []
    for s, pos in enumerate(M.CONTENT_POSITIONS):
        for k, side in enumerate("AB"):
            what, val = BAD[(2 * s + k) % 3]
            planted.append(("%s at the centre of scale %d (%s)" % (what, s, side),) + M.planted_pair(pos, side, val))
    special = [e for e in unit if e[0] in C.CENTRE_CLASSES]
    plain = [e for e in unit if e[0] not in C.CENTRE_CLASSES]
    entries = [e for three in zip(plain, special, planted) for e in three] + plain[len(planted):]
    assert len(unit) == 18 and len(special) == 8 and len(planted) == 8 and len(others) == 3 and len(entries) == 26
    cen = [selected_centres(a, b) for _, a, b in entries]
    assert all(cen[i] != cen[i + 1] for i in range(len(entries) - 1))
    pairs = [(a, b) for _, a, b in entries]
    g_out = [-0.75 + 0.25 * i for i in range(len(entries))]                  # differs per pair; one is 0
    clean = clean_means(ctx)
    alone = [launch(ctx, [pairs[i]], 1.0, [g_out[i]], clean) for i in range(len(entries))]
    assert sum(bool(np.isnan(x[0][0])) for x in alone) == 8 and not same(alone[0][2][0][0], alone[2][2][0][0])
    for call in range(2):
        v, m, g = launch(ctx, pairs, 1.0, g_out, clean)
        for i, (name, _, _) in enumerate(entries):
            assert same(v[i], alone[i][0][0]) and same(m[i], alone[i][1][0]), (name, call)
            assert same(g[i][0], alone[i][2][0][0]) and same(g[i][1], alone[i][2][0][1]), (name, call)
        for _, a, b, r, _ in others:                          # other data through the same context before the second call
            launch(ctx, [(a, b)], r, [1.0])
