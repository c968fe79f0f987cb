"""GPU: the 2-D float32 kernels (ssimf_kernels.hip, ssimw_kernels.hip, ssimk_kernels.hip) against the float64 models BY SAMPLE
CONTENT: the catalogue of tests/content_classes.py as planes -- the classes of tests/test_gpu_ssim3_content.py, with "centre" meaning
the centre sample of a 128-column strip column.  Sizes are W x H; arrays are (H, W).

Shape.  150 x 24: two strip columns with centres at x = 64 and x = 149 on row 11, three 8-row cells, 5 x 1 gradient tiles.  The centre
classes alter the SECOND strip column's centre sample (149, 11) only, so the first keeps its ordinary centre and the two columns of one
plane differ in centre; the steps lie on the strip columns' common edge (x = 128) and on the first cell's (y = 8).

Bounds.  None is new.  Value, map and both gradients of ssimf, the map gradient of ssimw under the three weight planes of
ssimw_model.weight_planes, and the windowed entries under the seven windows of ssimk_model.WINDOWS (scalar gradient and the planes of
ssimk_model.upstream_planes) are held to the float64 model at the family's bounds: ssimf_model.*_TOL, ssimw_model.WGRAD_TOL /
WIDENT_TOL, ssimk_model.tolerances(window).  tests/test_content_classes_cpu.py holds the condition: on these very planes the fp32
emulations stay within the EMU figures.  Exclusions, the huge / Inf / NaN classes and the figure where the exact gradient is 0: as in
tests/test_gpu_ssim3_content.py.

Do the tests bite?  Checked on the emulations (ssimf_model.centres altered, never committed):
 - the `<= range` select removed: `huge centre sample (A)`, `(B)`, `Inf at the centre (A)`, `(B)` and `NaN at the centre (B)` fail: the
   whole second strip column is centred by the bad sample;
 - the centre row taken from the workgroup's own rows: NO class fails, and none can.  A 2-D workgroup blurs its own halo under its own
   centre -- the gradient kernel recomputes the statistics of its tile + 2R and keeps nothing in scratch -- so any in-range centre gives
   the same mathematics, and a wrong one only changes rounding by less than `outlier at the centre` already leaves.  What pins the
   centre's position in 2-D is the bit identity across strip heights and batches (tests/test_gpu_tall_strips.py,
   tests/test_gpu_sample_forms.py), not accuracy.  In 3-D the coefficient scratch makes it an accuracy matter (see that module).
"""
import numpy as np
import pytest

import content_classes as C
import ssimf_model as M
import ssimk_model as K
import ssimw_model as MW
from test_gpu_ssimk import backward, forward, mk, same64
from test_gpu_ssimw import random_pair, same

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]     # the float64 model meets Inf - Inf on purpose

W, H = 150, 24
SHAPE = (H, W)
G_OUT = -0.75
WINDOWS = [None] + list(K.WINDOWS)
WINDOW_IDS = ["engine window"] + [K.name_of(w) for w in K.WINDOWS]
BY_WINDOW = pytest.mark.parametrize("window", WINDOWS, ids=WINDOW_IDS)

_refs = {}


def model_window(window):
    return K.DEFAULT if window is None else window


def tolerances(window):
    """(per pixel, global, gradient, ident, map gradient, map ident): the family's own."""
    if window is None:
        return M.PX_TOL, M.G_TOL, M.GRAD_TOL, M.IDENT_TOL, MW.WGRAD_TOL, MW.WIDENT_TOL
    px, g, grad, ident = K.tolerances(window)
    return px, g, grad, ident, grad, ident


def weights(window):
    return list(MW.weight_planes(H, W) if window is None else K.upstream_planes(H, W))


def references(window):
    """The classes under one window with their float64 model, computed once and left unchanged:
    [(name, a, b, r, exclude, gradient exclude, float64 map, scalar gradients, [(weight name, k, gradients)])]."""
    if window not in _refs:
        mw, R = model_window(window), K.radius(model_window(window))
        out = []
        for name, a, b, r, ex in C.plane_classes(SHAPE, radius=R):
            maps = [(wn, k, K.grad_map(a, b, r, k, mw)) for wn, k in weights(window)]
            out.append((name, a, b, r, ex, None if ex is None else C.dilate(ex, R), K.ssim_map(a, b, r, mw), K.grad(a, b, r, G_OUT, mw), maps))
        _refs[window] = out
    return _refs[window]


def calls(ctx, window, pairs, r, g_out, planes):
    """(sums, maps, scalar gradients, map gradients) of `pairs` in one launch each: the entries without _win for window None."""
    plain, win = window is None, mk(window)
    s, ms = forward(ctx, pairs, r, win, plain=plain)
    gr = backward(ctx, pairs, r, win, scalar=g_out, plain=plain)
    gm = backward(ctx, pairs, r, win, planes=planes, plain=plain)
    return s, ms, gr, gm


def hold(ctx, window, ref, what):
    """One class on the GPU against its float64 model; prints what it measured."""
    name, a, b, r, ex, exg, gm, want, maps = ref
    px_tol, g_tol, grad_tol, ident_tol, mapgrad_tol, mapident_tol = tolerances(window)
    n = float(W) * float(H)
    s, ms, gr, got_maps = calls(ctx, window, [(a, b)] * len(maps), r, [G_OUT] * len(maps), [k for _, k, _ in maps])
    px, gl = C.map_figures(name, s[0] / n, ms[0], gm, n, ex)
    scalar = C.grad_figures(name, gr[0], want, exg, abs(G_OUT) / n, r)
    weighted = [f for (_, k, wk), g in zip(maps, got_maps) for f in C.grad_figures(name, g, wk, exg, np.abs(k).max(), r)]
    figs = (px, gl, C.worst(scalar, False), C.worst(weighted, False), C.worst(scalar, True), C.worst(weighted, True))
    print("%s %s: per-pixel %.3g (%.3g), global %.3g (%.3g), gradients %.3g (%.3g), map gradients %.3g (%.3g), where the exact gradient "
          "is 0 %.3g (%.3g) and %.3g (%.3g)" % (what, name, px, px_tol, gl, g_tol, figs[2], grad_tol, figs[3], mapgrad_tol, figs[4], ident_tol,
                                                 figs[5], mapident_tol))
    assert px <= px_tol and gl <= g_tol, (what, name, px, gl)
    assert figs[2] <= grad_tol and figs[3] <= mapgrad_tol and figs[4] <= ident_tol and figs[5] <= mapident_tol, (what, name, figs)


def test_the_model_and_the_base_are_the_modules_own():
    """The engine window of ssimk_model is ssimf_model's taps, so one model serves the entries with and without a window; the
    catalogue's base pair is test_gpu_ssimw.random_pair; the centres are where the module says."""
    assert np.array_equal(K.full_taps(K.DEFAULT), M.gaussian_taps())
    for x, y in zip(C.random_pair(SHAPE, 4200), random_pair(W, H, 4200)):
        assert same(x, y)
    assert C.plane_centres(SHAPE) == [(11, 64), (11, 149)]


@BY_WINDOW
def test_every_class_against_the_model(gpu_ctx, window):
    what = WINDOW_IDS[WINDOWS.index(window)]
    for ref in references(window):
        hold(gpu_ctx, window, ref, "%s 150x24" % what)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["NaN", "Inf"])
@pytest.mark.parametrize("side", ["A", "B"])
@BY_WINDOW
def test_the_reach_of_a_nan_or_inf_at_a_strip_column_centre(gpu_ctx, window, side, bad):
    """The second strip column's centre sample of A or of B is NaN or Inf: that centre is 0, so exactly the (2R + 1)^2 map pixels and
    the (4R + 1)^2 gradient pixels around it are NaN -- both gradients, scalar and map form -- and every other pixel is finite, in the
    first strip column too."""
    R = K.radius(model_window(window))
    a, b = (x.copy() for x in C.random_pair(SHAPE, 4200))
    where = C.plane_centres(SHAPE)[1]
    (a if side == "A" else b)[where] = bad
    k = np.random.default_rng(6).standard_normal(SHAPE).astype(np.float32)
    s, ms, gr, gm = calls(gpu_ctx, window, [(a, b)], 1.0, [1.0], [k])
    near, far = C.box(SHAPE, where, R), C.box(SHAPE, where, 2 * R)
    assert np.isnan(s[0]) and np.array_equal(np.isnan(ms[0]), near) and np.all(np.isfinite(ms[0][~near]))
    for g in tuple(gr[0]) + tuple(gm[0]):
        assert np.array_equal(np.isnan(g), far) and np.all(np.isfinite(g[~far]))


@BY_WINDOW
def test_one_launch_of_every_class_has_the_bits_of_the_lone_launches(gpu_ctx, window):
    """ONE launch holds one plane of each class of data range 1 (18 pairs), neighbours differing in the second strip column's centre
    (0.5, ordinary, 0 on one side); every sum, map, gradient and map gradient has the bits of the class launched alone.  The launch is
    repeated after launches of the other ranges' classes."""
    ctx = gpu_ctx
    classes = dict((c[0], c) for c in C.plane_classes(SHAPE, radius=K.radius(model_window(window))))
    special = [n for n in classes if n in C.CENTRE_CLASSES]
    plain = [n for n in classes if n not in C.CENTRE_CLASSES and classes[n][3] == 1.0]
    names = [n for pair in zip(special, plain) for n in pair] + plain[len(special):]
    others = [c for c in classes.values() if c[3] != 1.0]
    assert len(names) == 18 and names[0] == "outlier at the centre" and names[2].startswith("centre above") and len(others) == 3
    pairs = [(classes[n][1], classes[n][2]) for n in names]
    k = np.random.default_rng(7).standard_normal(SHAPE).astype(np.float32)
    g = [-0.75 + 0.25 * i for i in range(len(names))]
    alone = [calls(ctx, window, [pairs[i]], 1.0, [g[i]], [k]) for i in range(len(names))]
    assert not same(alone[0][1][0], alone[1][1][0])
    for call in range(2):
        s, ms, gr, gm = calls(ctx, window, pairs, 1.0, g, [k] * len(names))
        for i, n in enumerate(names):
            assert same64(s[i], alone[i][0][0]) and same(ms[i], alone[i][1][0]), (n, call)
            for got, want in ((gr[i], alone[i][2][0]), (gm[i], alone[i][3][0])):
                assert same(got[0], want[0]) and same(got[1], want[1]), (n, call)
        for _, a, b, r, _ in others:                           # other data through the same context before the second call
            calls(ctx, window, [(a, b)], r, [1.0], [k])
