"""GPU: the float32 volume kernels (ssim3f_kernels.hip, ssim3w_kernels.hip, ssim3k_kernels.hip) and the 16-bit ones (ssim3h_kernels.hip)
against the float64 models BY SAMPLE CONTENT: the catalogue of tests/content_classes.py -- constants, a bump, an outlier at the volume's
centre voxel, a centre above the range, huge, Inf and NaN on A and on B, a narrow band near the range, an offset above the range,
negative and anticorrelated samples, steps on tile and cell boundaries, one impulse, ranges far from 1.  Sizes are W x H x D; arrays are
(D, H, W).

Why.  The kernels blur centred samples, one centre per volume, "the centre voxel when its magnitude is at most dataRange, else 0"; the
re-add uA = mA + cA, the derivative in the centred variables and the backward's coefficient scratch all ride on it, and centring is
invisible on benign data.  The other modules feed these kernels uniform noise and natural images.

Shape.  40 x 19 x 12: three tiles in x, two in y, an 8-slice cell and a 4-slice one; the centre (19, 9, 5) lies in the SECOND tile column,
so every other workgroup reads a centre from outside its own tile.  5 x 3 x 4, every axis shorter than the window, for the centre classes.

Bounds.  None is new.  Value, map, both gradients and the map gradient under the three weight volumes of ssim3w_model.weight_volumes are
held to the float64 model at the family's tolerances() -- ssim3f_model / ssim3w_model for the entries without a window, ssim3k_model per
window for the seven windows of ssimk_model.WINDOWS -- outside the class's exclusion.  tests/test_content_classes_cpu.py holds the
condition: on these very arrays the fp32 emulations of the kernels stay within the EMU figures, half of these bounds.  Where the exact
gradient is 0 (`constant equal`; a one-hot weight on a step's flat side) the IDENT bound takes max|grad| R / max|k|, the same figure as
max|grad| W H D R / |gOut| for the uniform k (see that module).  On the huge, Inf and NaN classes the comparison leaves out the
(2R + 1)^3 box (value, map) and the (4R + 1)^3 box (gradients) around the centre voxel; inside, Inf and NaN must give NaN on exactly
that box, and a huge sample (1e15: its square, 1e30, is finite in float32) must leave the map, every gradient and the value finite
wherever the float64 model is finite -- everywhere: a kernel that spread Inf or NaN through the windows of a finite sample fails.

Do the tests bite?  Checked on the emulations (ssim3f_model / ssim3k_model with centre() altered, never committed), under all eight
windows:
 - the `<= range` select removed: `huge centre sample (A)`, `(B)`, `Inf at the centre (A)`, `(B)` and `NaN at the centre (B)` fail --
   the whole volume is centred by the bad sample and no voxel outside the box stays finite or within the bound; `centre above the
   range` then still passes (3.0 is a poor centre, not a wrong one);
 - the centre taken from the workgroup's own tile: the forward stays right (each tile is consistent with itself); the GRADIENTS fail
   on 16 of the 22 classes, every one whose tiles then differ in centre -- `outlier at the centre`, `centre above the range (A)` and
   `(B)`, the huge, Inf and NaN classes, `flat with a bump`, `narrow high`, `negative`, `anticorrelated`, `range 1e-3`, `range 65535`,
   the steps on x and y -- because a coefficient in the scratch and the voxel that collects it across a tile edge no longer share
   their centre.
"""
import numpy as np
import pytest

import content_classes as C
import halfmodel as HM
import ssim3f_model as S
import ssim3k_model as K3
import ssim3w_model as W3
from test_gpu_ssim3f import Vol, random_pair, same
from test_gpu_ssim3h import Device
from test_gpu_ssim3h import run as run_half
from test_gpu_ssim3k import run, same_grads

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]     # the float64 model meets Inf - Inf on purpose

SIZE, SMALL = (40, 19, 12), (5, 3, 4)
SHAPE, SMALL_SHAPE = SIZE[::-1], SMALL[::-1]
G_OUT = -0.75
WINDOWS = [None] + list(K3.WINDOWS)
WINDOW_IDS = ["engine window"] + [K3.name_of(w) for w in K3.WINDOWS]
BY_WINDOW = pytest.mark.parametrize("window", WINDOWS, ids=WINDOW_IDS)
HALF_CLASSES = ("centre above the range (B)", "Inf at the centre (A)", "outlier at the centre")

_refs = {}


def model_window(window):
    return K3.DEFAULT if window is None else window


def tolerances(window):
    """(per voxel, global, gradient, ident, map gradient): the family's own."""
    if window is None:
        return S.tolerances() + (W3.tolerances(),)
    return K3.tolerances(window)


def references(shape, window, only=None):
    """The classes of one shape under one window with their float64 model, computed once and left unchanged:
    [(name, a, b, r, exclude, gradient exclude, float64 map, scalar gradients, [(weight name, k, gradients)])]."""
    key = (shape, window, only)
    if key not in _refs:
        mw, R = model_window(window), K3.radius(model_window(window))
        out = []
        for name, a, b, r, ex in C.volume_classes(shape, radius=R):
            if only is not None and name not in only:
                continue
            der = K3.derivatives(a, b, r, mw)
            maps = [(wn, k, K3.apply(der, k, mw)) for wn, k in W3.weight_volumes(shape, 0)]
            out.append((name, a, b, r, ex, None if ex is None else C.dilate(ex, R), K3.ssim_map(a, b, r, mw),
                        K3.apply(der, G_OUT / S.voxels(shape), mw), maps))
        _refs[key] = out
    return _refs[key]


def hold(ctx, window, ref, what):
    """One class on the GPU against its float64 model; prints what it measured."""
    name, a, b, r, ex, exg, gm, want, maps = ref
    px_tol, g_tol, grad_tol, ident_tol, mapgrad_tol = tolerances(window)
    vox = S.voxels(a.shape)
    va, vb = Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b)
    try:
        s, ms, gr = run(ctx, None, r, window, g_out=[G_OUT], inputs=[(va, vb)])
        got_maps = run(ctx, None, r, window, ks=[k for _, k, _ in maps], forward=False, inputs=[(va, vb)] * len(maps))[2]
    finally:
        va.free()
        vb.free()
    px, gl = C.map_figures(name, s[0] / vox, ms[0], gm, vox, ex)
    scalar = C.grad_figures(name, gr[0], want, exg, abs(G_OUT) / vox, r)
    weighted = [f for (_, k, wk), g in zip(maps, got_maps) for f in C.grad_figures(name, g, wk, exg, np.abs(k).max(), r)]
    figs = (px, gl, C.worst(scalar, False), C.worst(weighted, False), max(C.worst(scalar, True), C.worst(weighted, True)))
    print("%s %s: per-voxel %.3g (%.3g), global %.3g (%.3g), gradients %.3g (%.3g), map gradients %.3g (%.3g), where the exact gradient "
          "is 0 %.3g (%.3g)" % (what, name, px, px_tol, gl, g_tol, figs[2], grad_tol, figs[3], mapgrad_tol, figs[4], ident_tol))
    assert px <= px_tol and gl <= g_tol, (what, name, px, gl)
    assert figs[2] <= grad_tol and figs[3] <= mapgrad_tol and figs[4] <= ident_tol, (what, name, figs)


def test_the_model_and_the_base_are_the_modules_own():
    """The engine window of ssim3k_model is ssim3f_model's taps, so one model serves the entries with and without a window; the
    catalogue's base pair is test_gpu_ssim3f.random_pair."""
    assert np.array_equal(K3.full_taps(K3.DEFAULT), S.gaussian_taps())
    for x, y in zip(C.random_pair(SHAPE, 4100), random_pair(SIZE, 4100)):
        assert same(x, y)
    assert C.volume_centre(SHAPE) == (5, 9, 19)


@BY_WINDOW
def test_every_class_against_the_model(gpu_ctx, window):
    what = WINDOW_IDS[WINDOWS.index(window)]
    for ref in references(SHAPE, window):
        hold(gpu_ctx, window, ref, "%s 40x19x12" % what)


@BY_WINDOW
def test_centre_classes_where_every_axis_is_shorter_than_the_window(gpu_ctx, window):
    what = WINDOW_IDS[WINDOWS.index(window)]
    for ref in references(SMALL_SHAPE, window, C.CENTRE_CLASSES):
        hold(gpu_ctx, window, ref, "%s 5x3x4" % what)


# ---- reach -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["NaN", "Inf", "-Inf"])
@pytest.mark.parametrize("side", ["A", "B"])
@BY_WINDOW
def test_the_reach_of_a_nan_or_inf_at_the_centre(gpu_ctx, window, side, bad):
    """The centre voxel of A or of B is NaN or Inf: the centre of that side is 0, so exactly the (2R + 1)^3 map voxels and the
    (4R + 1)^3 gradient voxels around it are NaN -- for both gradients, the scalar and the map form -- and every other voxel is finite.
    A centre that let the sample through would spread it over the whole volume."""
    R = K3.radius(model_window(window))
    a, b = (x.copy() for x in C.random_pair(SHAPE, 4100))
    where = C.volume_centre(SHAPE)
    (a if side == "A" else b)[where] = bad
    k = np.random.default_rng(6).standard_normal(SHAPE).astype(np.float32)
    s, ms, gr = run(gpu_ctx, [(a, b)], 1.0, window, g_out=[1.0])
    got = run(gpu_ctx, [(a, b)], 1.0, window, ks=[k], forward=False)[2][0]
    near, far = C.box(SHAPE, where, R), C.box(SHAPE, where, 2 * R)
    assert np.isnan(s[0]) and np.array_equal(np.isnan(ms[0]), near) and np.all(np.isfinite(ms[0][~near]))
    for g in tuple(gr[0]) + tuple(got):
        assert np.array_equal(np.isnan(g), far) and np.all(np.isfinite(g[~far]))


# ---- determinism across content --------------------------------------------------------------------------------------------------------

def mixed_order(names):
    """The classes of one launch, ordered so that neighbours differ in centre: a centre class (outlier, above the range, huge, Inf, NaN:
    a centre of 0 on one side, or 0.5) between two classes with an ordinary centre."""
    special = [n for n in names if n in C.CENTRE_CLASSES]
    plain = [n for n in names if n not in C.CENTRE_CLASSES]
    out = []
    while special or plain:
        if special:
            out.append(special.pop(0))
        if plain:
            out.append(plain.pop(0))
    return out


@BY_WINDOW
def test_one_launch_of_every_class_has_the_bits_of_the_lone_launches(gpu_ctx, window):
    """ONE launch holds one volume of each class of data range 1 (19 volumes), neighbours differing in centre; every sum, map, gradient
    and map gradient has the bits of the class launched alone -- a centre taken from the neighbouring descriptor shows here.  The launch
    is repeated after a backward of the other ranges' classes has left their coefficients in the scratch."""
    ctx = gpu_ctx
    classes = dict((c[0], c) for c in C.volume_classes(SHAPE, radius=K3.radius(model_window(window))))
    names = mixed_order([n for n, c in classes.items() if c[3] == 1.0])
    others = [c for c in classes.values() if c[3] != 1.0]
    assert len(names) == 19 and names[0] == "outlier at the centre" and names[2].startswith("centre above") and len(others) == 3
    k = np.random.default_rng(7).standard_normal(SHAPE).astype(np.float32)
    inputs = [(Vol(ctx, SHAPE, "dense", classes[n][1]), Vol(ctx, SHAPE, "dense", classes[n][2])) for n in names]
    g = [-0.75 + 0.25 * i for i in range(len(names))]
    try:
        alone = [run(ctx, None, 1.0, window, g_out=[g[i]], inputs=[inputs[i]]) for i in range(len(names))]
        alone_map = [run(ctx, None, 1.0, window, ks=[k], forward=False, inputs=[inputs[i]])[2][0] for i in range(len(names))]
        assert not same(alone[0][1][0], alone[1][1][0])
        for call in range(2):
            s, ms, gr = run(ctx, None, 1.0, window, g_out=g, inputs=inputs)
            gm = run(ctx, None, 1.0, window, ks=[k] * len(names), forward=False, inputs=inputs)[2]
            for i, n in enumerate(names):
                assert same(s[i:i + 1], alone[i][0]) and same(ms[i], alone[i][1][0]), (n, call)
                assert same_grads(gr[i], alone[i][2][0]) and same_grads(gm[i], alone_map[i]), (n, call)
            for _, a, b, r, _ in others:                       # other data in the scratch before the second call
                run(ctx, [(a, b)], r, window, g_out=[1.0], forward=False)
    finally:
        for va, vb in inputs:
            va.free()
            vb.free()


# ---- 16-bit volumes ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device(gpu_ctx):
    d = Device(gpu_ctx)
    yield d
    gpu_ctx.trim()


@pytest.mark.parametrize("enc", HM.ENCODINGS)
@pytest.mark.parametrize("shape", [SHAPE, SMALL_SHAPE], ids=["40x19x12", "5x3x4"])
def test_half_volumes_against_the_float64_model(device, enc, shape):
    """float16 and bfloat16 volumes of three centre classes on the grid k / 128, which both encodings hold exactly (asserted): value and
    map against the float64 model -- not against ssim3f -- at ssim3f's bounds.  No bound for a 16-bit gradient exists, so none is held."""
    px_tol, g_tol = S.tolerances()[:2]
    vox = S.voxels(shape)
    classes = [c for c in C.volume_classes(shape, exact=True) if c[0] in HALF_CLASSES]
    assert len(classes) == 3
    for name, a, b, r, ex in classes:
        ua, ub = HM.round_to(a, enc), HM.round_to(b, enc)
        assert same(HM.widen(ua, enc), a) and same(HM.widen(ub, enc), b), (name, enc)
        s, ms, _ = run_half(device, enc, [(ua, ub)], r)
        px, gl = C.map_figures(name, s[0] / vox, ms[0], S.ssim_map(a, b, r), vox, ex)
        print("%s %dx%dx%d %s: per-voxel %.3g (%.3g), global %.3g (%.3g)" % ((enc,) + shape[::-1] + (name, px, px_tol, gl, g_tol)))
        assert px <= px_tol and gl <= g_tol, (name, enc, px, gl)

