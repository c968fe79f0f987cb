"""CPU: the catalogue of tests/content_classes.py is what it claims, and on it every float family's fp32 emulation of its kernels stays
within the family's EMU figures of its float64 model -- half of what tests/test_gpu_ssim3_content.py and tests/test_gpu_ssimf_content.py
assert of the GPU on the same arrays.  This is the reference alone: no GPU, no library call.  It is the condition that keeps those modules
honest: a class on which the kernels' own arithmetic (restated operation by operation) left more than the EMU figure would make the GPU
bound a statement about the class, not about the kernel.

Families and figures.  ssim3f_model.emulate_fp32 (per voxel, global, gradient, and max|grad| W H D R where the exact gradient is 0);
ssim3w_model.emulate_fp32_map_grad under the three weight volumes of ssim3w_model.weight_volumes; ssim3k_model.emulate_fp32 under every
window of ssimk_model.WINDOWS (scalar and map gradients); ssimf_model.emulate_fp32; ssimw_model.emulate_fp32_map_grad under
ssimw_model.weight_planes; ssimk_model.emulate_fp32 under every window (scalar gradient and ssimk_model.upstream_planes).

Where the exact gradient is 0.  `constant equal` under any weight, and a one-hot weight whose windows see a = b only (a step's flat side):
the error relative to max|grad| has no meaning there.  The gradient is linear in the upstream weight k, and the families' IDENT figure is
max|grad| W H D R / |gOut| = max|grad| R / |k| for the uniform k = gOut / (W H D); with a weight volume the same figure is taken as
max|grad| R / max|k| (ssimw_model.EMU_WIDENT is defined so), against the family's IDENT figure.  No bound is new.

EXCLUDED lists the (family, class, window) triples whose emulation exceeds an EMU figure and whose amplitude could not be lowered: at most
two, never a centre class.  It is empty: the amplitudes of tests/content_classes.py are chosen so that every class stays within 85 % of
every family's and window's figures.  On the huge classes the emulations, like the GPU, must be finite inside the boxes wherever the
float64 model is (content_classes.map_figures, grad_figure).

offsets_above_the_range() measures what the documents state about samples far above the data range (README.md): nothing
is asserted of the GPU there.
"""
import numpy as np
import pytest

import content_classes as C
import halfmodel as HM
import ssim3f_model as S
import ssim3k_model as K3
import ssim3w_model as W3
import ssimf_model as M
import ssimk_model as K
import ssimw_model as MW

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")     # the float64 models meet Inf - Inf on the Inf and NaN classes

VOLUME, SMALL_VOLUME, PLANE = (12, 19, 40), (4, 3, 5), (24, 150)       # (D, H, W), (D, H, W), (H, W): the GPU modules' shapes
G_OUT = -0.75
HALF_CLASSES = ("centre above the range (B)", "Inf at the centre (A)", "outlier at the centre")
# (family, class, window name): the emulation's measured figure, where no lower amplitude brings it inside.  At most two, no centre class.
EXCLUDED = {}


def volume_rows(shape, window=None, only=None, exact=False):
    """[(class, {figure name: (measured, EMU bound)})] of the 3-D families on the catalogue: window None, ssim3f_model and ssim3w_model;
    else ssim3k_model under that window."""
    R = 5 if window is None else K3.radius(window)
    samples = S.voxels(shape)
    rows = []
    for name, a, b, r, ex in C.volume_classes(shape, radius=R, exact=exact):
        if only is not None and name not in only:
            continue
        exg = None if ex is None else C.dilate(ex, R)
        k = G_OUT / samples
        weights = list(W3.weight_volumes(shape, 0))
        if window is None:
            emu_px, emu_g, emu_grad, emu_ident, emu_map = S.EMU_PX, S.EMU_G, S.EMU_GRAD, S.EMU_IDENT, W3.EMU_GRAD
            _, gm = S.ssim(a, b, r)
            ev, em, ea, eb = S.emulate_fp32(a, b, r, g_out=G_OUT)
            scalar = C.grad_figures(name, (ea, eb), S.grad(a, b, r, G_OUT), exg, abs(k), r)
            der = W3.derivatives_fp32(a, b, r)
            maps = [f for _, kv in weights for f in C.grad_figures(name, W3.apply_fp32(der, kv), W3.grad_map(a, b, r, kv), exg, np.abs(kv).max(), r)]
        else:
            emu_px, emu_g, emu_grad, emu_ident, emu_map = K3.EMU[window]
            _, gm = K3.ssim(a, b, r, window)
            ev, em, der = K3.forward_fp32(a, b, r, window)
            der64 = K3.derivatives(a, b, r, window)
            scalar = C.grad_figures(name, K3.apply_fp32(der, np.float32(float(np.float32(G_OUT)) / samples), window), K3.apply(der64, k, window), exg, abs(k), r)
            maps = [f for _, kv in weights for f in C.grad_figures(name, K3.apply_fp32(der, kv, window), K3.apply(der64, kv, window), exg, np.abs(kv).max(), r)]
        px, gl = C.map_figures(name, ev, em, gm, samples, ex)
        rows.append((name, {"px": (px, emu_px), "global": (gl, emu_g), "grad": (C.worst(scalar, False), emu_grad),
                            "mapgrad": (C.worst(maps, False), emu_map), "null": (max(C.worst(scalar, True), C.worst(maps, True)), emu_ident)}))
    return rows


def plane_rows(shape, window=None):
    """The same of the 2-D families: window None, ssimf_model and ssimw_model; else ssimk_model under that window."""
    R = 5 if window is None else K.radius(window)
    h, w = shape
    samples = float(w) * float(h)
    rows = []
    for name, a, b, r, ex in C.plane_classes(shape, radius=R):
        exg = None if ex is None else C.dilate(ex, R)
        k = G_OUT / samples
        if window is None:
            emu_px, emu_g, emu_grad, emu_ident, emu_map, emu_mapnull = M.EMU_PX, M.EMU_G, M.EMU_GRAD, M.EMU_IDENT, MW.EMU_WGRAD, MW.EMU_WIDENT
            _, gm = M.ssim(a, b, r)
            ev, em, ea, eb = M.emulate_fp32(a, b, r, g_out=G_OUT)
            scalar = C.grad_figures(name, (ea, eb), M.grad(a, b, r, G_OUT), exg, abs(k), r)
            maps = [f for _, kv in MW.weight_planes(h, w) for f in C.grad_figures(name, MW.emulate_fp32_map_grad(a, b, r, kv), MW.grad_map(a, b, r, kv), exg, np.abs(kv).max(), r)]
        else:
            emu_px, emu_g, emu_grad, emu_ident = K.EMU[window]
            emu_map, emu_mapnull = emu_grad, emu_ident
            _, gm = K.ssim(a, b, r, window)
            ev, em, ea, eb = K.emulate_fp32(a, b, r, window, g_out=G_OUT)
            scalar = C.grad_figures(name, (ea, eb), K.grad(a, b, r, G_OUT, window), exg, abs(k), r)
            maps = [f for _, kv in K.upstream_planes(h, w) for f in C.grad_figures(name, K.emulate_fp32(a, b, r, window, gmap=kv)[2:], K.grad_map(a, b, r, kv, window), exg, np.abs(kv).max(), r)]
        px, gl = C.map_figures(name, ev, em, gm, samples, ex)
        rows.append((name, {"px": (px, emu_px), "global": (gl, emu_g), "grad": (C.worst(scalar, False), emu_grad), "mapgrad": (C.worst(maps, False), emu_map),
                            "null": (C.worst(scalar, True), emu_ident), "mapnull": (C.worst(maps, True), emu_mapnull)}))
    return rows


def hold(family, wname, rows):
    """Print the table of one family and window; every figure within its EMU bound, or the triple in EXCLUDED."""
    keys = list(rows[0][1])
    print("\n%s, %s: the emulation against the float64 model, worst figure (EMU bound)" % (family, wname))
    print("%-28s " % "class" + " ".join("%-19s" % k for k in keys))
    over = []
    for name, figs in rows:
        print("%-28s " % name + " ".join("%8.2e (%7.1e)" % figs[k] for k in keys))
        if any(not figs[k][0] <= figs[k][1] for k in keys) and (family, name, wname) not in EXCLUDED:
            over.append((name, {k: figs[k] for k in keys if not figs[k][0] <= figs[k][1]}))
    assert not over, over


WINDOW_PARAMS = [None] + list(K.WINDOWS)
WINDOW_IDS = ["engine window"] + [K.name_of(w) for w in K.WINDOWS]


@pytest.mark.parametrize("window", WINDOW_PARAMS, ids=WINDOW_IDS)
def test_volume_emulations_stay_within_the_emu_figures(window):
    wname = "engine window" if window is None else K.name_of(window)
    family = "ssim3f + ssim3w" if window is None else "ssim3k"
    hold(family, wname + " %dx%dx%d" % VOLUME[::-1], volume_rows(VOLUME, window))
    hold(family, wname + " %dx%dx%d" % SMALL_VOLUME[::-1], volume_rows(SMALL_VOLUME, window, only=C.CENTRE_CLASSES))


@pytest.mark.parametrize("window", WINDOW_PARAMS, ids=WINDOW_IDS)
def test_plane_emulations_stay_within_the_emu_figures(window):
    wname = "engine window" if window is None else K.name_of(window)
    hold("ssimf + ssimw" if window is None else "ssimk", wname + " %dx%d" % PLANE[::-1], plane_rows(PLANE, window))


def test_the_excluded_table_is_small_and_holds_no_centre_class():
    assert len(EXCLUDED) <= 2 and not any(name in C.CENTRE_CLASSES for _, name, _ in EXCLUDED)


def test_the_classes_exact_in_float16_and_bfloat16():
    """The three classes of the 16-bit volumes, on the grid: every sample survives both encodings unchanged, and the emulation holds."""
    for shape in (VOLUME, SMALL_VOLUME):
        classes = [c for c in C.volume_classes(shape, exact=True) if c[0] in HALF_CLASSES]
        assert len(classes) == 3
        for name, a, b, r, ex in classes:
            for enc in HM.ENCODINGS:
                for v in (a, b):
                    back = HM.widen(HM.round_to(v, enc), enc)
                    assert np.array_equal(back.view(np.uint32), v.view(np.uint32)), (name, enc)
        hold("ssim3f on the grid k / 128", "%dx%dx%d" % shape[::-1], volume_rows(shape, None, only=HALF_CLASSES, exact=True))


# ---- the classes are what they claim ----------------------------------------------------------------------------------------------

def differing(x, y):
    return [tuple(p) for p in np.argwhere(x.view(np.uint32) != y.view(np.uint32))]


@pytest.mark.parametrize("shape", [VOLUME, SMALL_VOLUME], ids=["40x19x12", "5x3x4"])
def test_volume_classes_alter_the_voxel_the_model_takes_the_centre_from(shape):
    classes = C.volume_classes(shape)
    base_a, base_b = C.random_pair(shape, 4100)
    centre = C.volume_centre(shape)
    assert centre == tuple((n - 1) // 2 for n in shape) and (shape != VOLUME or centre == (5, 9, 19))
    names = [c[0] for c in classes]
    assert all(n in names for n in C.CENTRE_CLASSES) and len(set(names)) == len(names)
    for name, a, b, r, ex in classes:
        if name not in C.CENTRE_CLASSES or name == "outlier at the centre":
            continue
        side = name[-2]
        hit, other, base_hit, base_other = (a, b, base_a, base_b) if side == "A" else (b, a, base_b, base_a)
        assert differing(hit, base_hit) == [centre] and differing(other, base_other) == [], name
        # the centre: 0 on the altered side only -- above the range, or not a number --, the base's own sample on the other
        assert S.centre(hit, r) == 0 and S.centre(other, r) == base_other[centre] != 0, name
        assert (ex is None) == name.startswith("centre above"), name
        if ex is not None:
            assert np.array_equal(ex, C.box(shape, centre, 5)), name
    _, a, b, r, _ = C.named(classes, "outlier at the centre")
    assert differing(a, np.full(shape, np.float32(C.FLAT))) == [centre] and S.centre(a, r) == np.float32(C.BUMP) and abs(S.centre(b, r) - C.FLAT) < 0.3
    _, a, b, r, _ = C.named(classes, "offset above the range")
    assert S.centre(a, r) == 0 and S.centre(b, r) == 0 and a[centre] > 2 and b[centre] >= 2
    _, a, b, r, _ = C.named(classes, "unit data at range 1e-6")
    assert S.centre(a, r) == 0 and S.centre(b, r) == 0 and r == 1e-6
    for name in ("impulse", "flat with a bump"):
        _, a, _, _, _ = C.named(classes, name)
        at = tuple(np.argwhere(a == a.max())[0])
        assert np.count_nonzero(a == a.max()) == 1 and at == C.off_centre(shape) and all(p != c for p, c in zip(at, centre)), name


def test_plane_classes_alter_the_centre_of_the_second_strip_column():
    classes = C.plane_classes(PLANE)
    base_a, base_b = C.random_pair(PLANE, 4200)
    centres = C.plane_centres(PLANE)
    assert centres == [(11, 64), (11, 149)]
    first, second = centres
    for name, a, b, r, ex in classes:
        if name not in C.CENTRE_CLASSES or name == "outlier at the centre":
            continue
        side = name[-2]
        hit, other, base_hit, base_other = (a, b, base_a, base_b) if side == "A" else (b, a, base_b, base_a)
        assert differing(hit, base_hit) == [second] and differing(other, base_other) == [], name
        ch, co = M.centres(hit, r), M.centres(other, r)
        assert ch[1] == 0 and ch[0] == base_hit[first] != 0 and co[0] == base_other[first] != 0 and co[1] == base_other[second] != 0, name
        if ex is not None:
            assert np.array_equal(ex, C.box(PLANE, second, 5)), name
    _, a, b, r, _ = C.named(classes, "outlier at the centre")
    assert differing(a, np.full(PLANE, np.float32(C.FLAT))) == [second] and list(M.centres(a, r)) == [np.float32(C.FLAT), np.float32(C.BUMP)]
    _, a, b, r, _ = C.named(classes, "offset above the range")
    assert not M.centres(a, r).any() and not M.centres(b, r).any()
    for name in ("impulse", "flat with a bump"):
        _, a, _, _, _ = C.named(classes, name)
        at = tuple(np.argwhere(a == a.max())[0])
        assert np.count_nonzero(a == a.max()) == 1 and at not in centres and at[0] != 11 and at[1] not in (64, 149), name


def test_the_base_is_the_gpu_modules_random_pair():
    """content_classes.random_pair restates the generator of tests/test_gpu_ssim3f.py and tests/test_gpu_ssimw.py (not imported here: they
    load the library)."""
    rng = np.random.default_rng(4100)
    a = rng.random(VOLUME, dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal(VOLUME).astype(np.float32), 0, 1).astype(np.float32)
    got = C.random_pair(VOLUME, 4100)
    assert np.array_equal(got[0], a) and np.array_equal(got[1], b)
    _, ca, cb, r, _ = C.named(C.volume_classes(VOLUME), "range 65535")
    assert np.array_equal(ca, a * np.float32(65535)) and np.array_equal(cb, b * np.float32(65535)) and r == 65535.0


# ---- large offsets above the range: what the documents state ------------------------------------------------------------------------

def offsets_above_the_range(offsets=(8.0, 100.0, 1000.0), shape=(12, 19, 21), plane=PLANE):
    """[(offset, per-voxel error of ssim3f_model.emulate_fp32, per-pixel error of ssimf_model.emulate_fp32)], each against its float64
    model, for the base pair + offset at range 1 on a 21 x 19 x 12 volume and on a 150 x 24 plane: samples above the range are used as
    stored, not centred, and the cancellation in E[a^2] - mu^2 grows with the square of the offset."""
    a, b = C.random_pair(shape, 4100)
    pa, pb = C.random_pair(plane, 4200)
    out = []
    for off in offsets:
        o = np.float32(off)
        e3 = float(np.abs(S.emulate_fp32(a + o, b + o, 1.0)[1] - S.ssim(a + o, b + o, 1.0)[1]).max())
        e2 = float(np.abs(M.emulate_fp32(pa + o, pb + o, 1.0)[1] - M.ssim(pa + o, pb + o, 1.0)[1]).max())
        out.append((off, e3, e2))
    return out


def test_large_offsets_above_the_range_are_measured_not_bounded():
    """Prints the figures README.md and INTEGRATION.md quote.  The documents promise nothing here, so nothing is asserted but the trend
    they describe: in both families the error grows with the offset and is past the per-sample bound by an offset of 100."""
    figs = offsets_above_the_range()
    for off, e3, e2 in figs:
        print("offset %g above range 1: per-sample error of the emulation %.3g (volume), %.3g (plane)" % (off, e3, e2))
    assert figs[0][1] < figs[1][1] < figs[2][1] and figs[1][1] > 2 * S.EMU_PX
    assert figs[0][2] < figs[1][2] < figs[2][2] and figs[1][2] > M.PX_TOL
