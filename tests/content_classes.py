"""A catalogue of sample CONTENT for the float32 SSIM families, in plain numpy: seeded, no GPU, no library call.

The float kernels blur centred samples a' = a - cA, b' = b - cB: one centre per volume (ssim3f_model.centre) or per 128-column strip column
(ssimf_model.centres), the sample at a fixed position "when its magnitude is at most the data range, else 0".  Centring is invisible in the
mathematics, so a centre read from the wrong place, a missing select or a cA / cB swap only shows when the centre sample is an outlier,
above the range, Inf or NaN -- and the SSIM terms themselves want content that drives them: sigma = 0, negative SSIM, means near the range,
negative samples, samples above the range, a step edge on a tile boundary, one impulse, ranges far from 1.  This module holds that content
once, for tests/test_content_classes_cpu.py (the emulations against the float64 models: the reference alone) and for the GPU modules
tests/test_gpu_ssim3_content.py and tests/test_gpu_ssimf_content.py.

volume_classes(shape, data_range) and plane_classes(shape, data_range) return [(name, a, b, data range, exclude)].  shape is the array's:
(D, H, W) or (H, W).  data_range scales the classes that have no range of their own.  exclude is None, or a boolean mask of the samples
left out of the accuracy comparison of the VALUE and the MAP under the window radius given (the (2R + 1)-box around the altered sample,
clipped); dilate(exclude, R) is the (4R + 1)-box of the GRADIENTS.  exact=True puts every sample of the generic classes on the grid k / 128
(flat 0.125, outlier 0.375), which float16 and bfloat16 hold exactly.

Amplitudes.  Every amplitude is chosen under one condition: on the shapes the GPU modules use, each family's fp32 emulation of its
kernels stays within 85 % of every EMU figure of every window (tests/test_content_classes_cpu.py prints what each class leaves), so that
the GPU bound -- twice EMU -- says something about the kernel and not about the class.  Two kinds of content bring the kernels' own
arithmetic near those figures, and their amplitudes are the largest round ones the condition allows: a rounding that every sample
shares, which the global figure cannot average away (`constant differ` at 0.1 / 0.2; `outlier at the centre` at 0.5 over 0.1, the
volume centred to -0.4), and a gradient that is a small difference of large terms (`narrow high`, the steps at height 0.25, `offset
above the range` at +1.5).  The outlier separates cA from cB by 0.4, the offset puts every sample above the range, the steps cross a tile
boundary.  `narrow high` is 0.85 + 0.15 base: means near the range, but its variance (1.9e-3) is NOT small against C2 (8.1e-4) -- a
narrower band (0.98 + 0.02 base) leaves up to 3 times the gradient figure of seven (family, window) pairs in the emulation, more than
the two an exclusion may cover.  sigma near 0 is driven by the constants, the flat classes and the steps' flat sides at low means only;
means near the range WITH tiny variance are not covered by this catalogue.

The 2-D multi-scale family (tests/test_gpu_msssimf_content.py, planes of 300 x 40 at 4 scales) is the one place where the condition does
not hold for every class, and there the amplitudes stay as they are: msssimf_model.CLASS_EMU holds the three classes' own emulated (value,
mean, gradient) figures and the GPU bound is derived from those.  They are measured limits of centring: the step on a strip column's edge
(x = 256) is a step ON the centre sample two scales down, where the flat side is blurred at a' = -0.25 and E[a'^2] - mu'^2 cancels against
C2 (5.0e-6, 2.0e-5, 4.3e-6); with every sample above the range every centre is 0 and nothing is centred (`offset above the range`: 2.5e-6,
1.2e-5, 2.1e-4; `unit data at range 1e-6`: 8.4e-7, 3.2e-6, 7.6e-5).
"""
import numpy as np

F = np.float32
STRIP_W = 128

CENTRE_CLASSES = ("outlier at the centre", "centre above the range (A)", "centre above the range (B)", "huge centre sample (A)",
                  "huge centre sample (B)", "Inf at the centre (A)", "Inf at the centre (B)", "NaN at the centre (B)")
NONFINITE_CLASSES = ("Inf at the centre (A)", "Inf at the centre (B)", "NaN at the centre (B)")
HUGE_CLASSES = ("huge centre sample (A)", "huge centre sample (B)")
FLAT, BUMP, ABOVE, HUGE = 0.1, 0.5, 3.0, 1e15         # flat level; bump and outlier; the centre above range 1; huge
CONST_A, CONST_B = 0.1, 0.2                           # `constant differ`
NARROW = 0.15                                         # `narrow high`: (1 - NARROW) + NARROW base
STEP = 0.25                                           # the steps' height
OFFSET = 1.5                                          # `offset above the range`
EXACT_BUMP = 0.375                                    # the outlier on the grid of the 16-bit encodings, over a flat 0.125


def random_pair(shape, seed):
    """The base pair: uniform [0, 1) and a noisy, clipped copy -- test_gpu_ssim3f.random_pair / test_gpu_ssimw.random_pair, restated
    (the GPU modules assert the bits agree)."""
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=F)
    b = np.clip(a + F(0.1) * rng.standard_normal(shape).astype(F), 0, 1).astype(F)
    return a, b


def volume_centre(shape):
    """(z, y, x) of the volume's centre sample."""
    return tuple((n - 1) // 2 for n in shape)


def plane_centres(shape):
    """[(y, x)] of the centre sample of every strip column."""
    h, w = shape
    return [((h - 1) // 2, min(x0 + 64, w - 1)) for x0 in range(0, w, STRIP_W)]


def off_centre(shape):
    """The position of the bump and of the impulse: a third of the way along every axis, moved on by one where that is a centre
    coordinate of the axis -- never a centre of a volume or of a strip column, and inside the first tile of the shapes in use."""
    pos = []
    for n in shape:
        p = n // 3
        if n > 1 and p == (n - 1) // 2:
            p = (p + 1) % n
        pos.append(p)
    return tuple(pos)


def box(shape, where, radius):
    m = np.zeros(shape, bool)
    m[tuple(slice(max(p - radius, 0), p + radius + 1) for p in where)] = True
    return m


def dilate(mask, radius):
    """Every sample within `radius` (on every axis) of a sample of the mask."""
    out = np.zeros_like(mask)
    for p in np.argwhere(mask):
        out |= box(mask.shape, tuple(p), radius)
    return out


def _classes(shape, data_range, radius, centres_ab, steps, seed, exact):
    """centres_ab: the position altered on A / B by the centre classes.  steps: [(label, axis, split)]."""
    r = F(data_range)
    base_a, base_b = random_pair(shape, seed)
    if exact:
        base_a, base_b = (np.round(base_a * F(128)) / F(128)).astype(F), (np.round(base_b * F(128)) / F(128)).astype(F)
    flat_v, bump_v = (F(0.125), F(EXACT_BUMP)) if exact else (F(FLAT), F(BUMP))
    rng = np.random.default_rng(seed + 1)
    noise = rng.standard_normal(shape).astype(F)
    if exact:
        noise = (np.round(noise * F(8)) / F(8)).astype(F)
    flat = np.full(shape, flat_v, F)
    off = off_centre(shape)
    out = []

    def add(name, a, b, rng_=None, exclude=None):
        out.append((name, np.ascontiguousarray(a, F), np.ascontiguousarray(b, F), float(r if rng_ is None else rng_), exclude))

    def altered(side, value, scale=True):
        a, b = base_a * r, base_b * r
        t = a if side == "A" else b
        t[centres_ab] = F(value) * r if scale else F(value)
        return a, b
    add("constant equal", np.full(shape, F(0.5)) * r, np.full(shape, F(0.5)) * r)
    add("constant differ", np.full(shape, F(CONST_A)) * r, np.full(shape, F(CONST_B)) * r)
    bump = flat.copy()
    bump[off] = bump_v
    add("flat with a bump", bump * r, (bump + F(0.05 if not exact else 0.0625) * noise).astype(F) * r)
    outlier = flat.copy()
    outlier[centres_ab] = bump_v
    add("outlier at the centre", outlier * r, (flat + F(0.05 if not exact else 0.0625) * noise).astype(F) * r)
    for side in "AB":
        add("centre above the range (%s)" % side, *altered(side, ABOVE))
    for side in "AB":
        add("huge centre sample (%s)" % side, *altered(side, HUGE, scale=False), exclude=box(shape, centres_ab, radius))
    for what, side in (("Inf", "A"), ("Inf", "B"), ("NaN", "B")):
        add("%s at the centre (%s)" % (what, side), *altered(side, np.inf if what == "Inf" else np.nan, scale=False),
            exclude=box(shape, centres_ab, radius))
    add("narrow high", (F(1.0 - NARROW) + F(NARROW) * base_a).astype(F) * r, (F(1.0 - NARROW) + F(NARROW) * base_b).astype(F) * r)
    add("offset above the range", (base_a + F(OFFSET)) * r, (base_b + F(OFFSET)) * r)
    add("negative", -base_a * r, -base_b * r)
    add("anticorrelated", base_a * r, (F(1.0) - base_a).astype(F) * r)
    for label, axis, split in steps:
        idx = np.arange(shape[axis]).reshape([-1 if k == axis else 1 for k in range(len(shape))])
        add("step on %s = %d" % (label, split), np.broadcast_to((idx >= split).astype(F) * F(STEP), shape) * r,
            np.broadcast_to((idx >= split + 1).astype(F) * F(STEP), shape) * r)
    impulse = np.zeros(shape, F)
    impulse[off] = 1
    add("impulse", impulse * r, np.zeros(shape, F))
    add("range 1e-3", base_a * F(1e-3), base_b * F(1e-3), 1e-3)
    add("range 65535", base_a * F(65535), base_b * F(65535), 65535.0)
    add("unit data at range 1e-6", base_a, base_b, 1e-6)
    return out


def volume_classes(shape, data_range=1.0, radius=5, seed=4100, exact=False):
    """The catalogue as volumes of `shape` = (D, H, W).  The centre classes alter the volume's one centre sample; the steps split x at 16
    (the first tile boundary), y at 16 and z at 8 (the first 8-slice cell), each clipped to the last sample of a shorter axis."""
    d, h, w = shape
    steps = [("x", 2, min(16, w - 1)), ("y", 1, min(16, h - 1)), ("z", 0, min(8, d - 1))]
    return _classes(tuple(shape), data_range, radius, volume_centre(shape), steps, seed, exact)


def plane_classes(shape, data_range=1.0, radius=5, seed=4200, exact=False):
    """The catalogue as planes of `shape` = (H, W).  The centre classes alter the centre sample of the LAST strip column (the second of a
    plane of 129 .. 256 columns), so that the first keeps its ordinary centre; the steps split x at the last strip column's first column
    (128: a strip column's edge, which every 32-pixel gradient tile shares) and y at 8 (the first 8-row cell)."""
    h, w = shape
    steps = [("x", 1, min(STRIP_W * ((w - 1) // STRIP_W), w - 1)), ("y", 0, min(8, h - 1))]
    return _classes(tuple(shape), data_range, radius, plane_centres(shape)[-1], steps, seed, exact)


def named(classes, name):
    for c in classes:
        if c[0] == name:
            return c
    raise KeyError(name)


# ---- the comparison every module makes -----------------------------------------------------------------------------------------------

def map_figures(name, got_value, got_map, want_map, samples, exclude):
    """(per-sample error, global error) of a value and a map against the float64 map outside `exclude`, after the finiteness checks: every
    sample outside `exclude` is finite; the non-finite classes are NaN on all of `exclude` and give a NaN value; the huge classes are
    finite inside `exclude` exactly where the float64 model is, and their value is finite when the model's is.  With an exclusion the
    global figure is taken on the sum of the map's samples outside it."""
    got_map = np.asarray(got_map, np.float64)
    if exclude is None:
        assert np.all(np.isfinite(got_map)) and np.isfinite(got_value), name
        return float(np.abs(got_map - want_map).max()), abs(float(got_value) - float(np.sum(want_map)) / samples)
    assert np.all(np.isfinite(got_map[~exclude])), name
    assert np.array_equal(np.isnan(want_map), exclude) == (name in NONFINITE_CLASSES), name      # the model's own reach
    if name in NONFINITE_CLASSES:
        assert np.array_equal(np.isnan(got_map), exclude) and np.isnan(got_value), name
    if name in HUGE_CLASSES:
        assert np.array_equal(np.isfinite(got_map[exclude]), np.isfinite(want_map[exclude])), name
        assert np.isfinite(got_value) == np.isfinite(np.sum(want_map)), name
    if exclude.all():
        return 0.0, 0.0
    return float(np.abs(got_map - want_map)[~exclude].max()), abs(float(np.sum(got_map[~exclude])) - float(np.sum(want_map[~exclude]))) / samples


def grad_figure(name, got, want, exclude, null_scale=None):
    """The error of one gradient against the float64 gradient over the latter's largest magnitude, both outside `exclude` (the gradients'
    box); null_scale given -- the exact gradient is 0 --: max|grad| * null_scale instead.  Finiteness as in map_figures."""
    got = np.asarray(got, np.float64)
    if exclude is None:
        assert np.all(np.isfinite(got)), name
        keep = np.ones(got.shape, bool)
    else:
        keep = ~exclude
        assert np.all(np.isfinite(got[keep])), name
        if name in NONFINITE_CLASSES:
            assert np.array_equal(np.isnan(want), exclude) and np.array_equal(np.isnan(got), exclude), name
        if name in HUGE_CLASSES:
            assert np.array_equal(np.isfinite(got[exclude]), np.isfinite(want[exclude])), name
    if not keep.any():
        return 0.0
    if null_scale is not None:
        return float(np.abs(got[keep]).max()) * null_scale
    return float(np.abs(got - want)[keep].max() / np.abs(want[keep]).max())


def is_null(want, keep, kmax, r):
    """The exact gradient is 0 up to float64 rounding (ssimw_model.is_null, outside an exclusion): the images agree wherever a window reaches a non-zero weight."""
    return not keep.any() or float(np.abs(want[keep]).max()) * float(r) <= 1e-9 * float(kmax)


def grad_figures(name, got, want, exg, kmax, r):
    """[(figure, is the null figure)] of a pair of gradients for an upstream weight of largest magnitude kmax."""
    out = []
    for g, w in zip(got, want):
        keep = np.ones(w.shape, bool) if exg is None else ~exg
        null = is_null(w, keep, kmax, r)
        out.append((grad_figure(name, g, w, exg, float(r) / float(kmax) if null else None), null))
    return out


def worst(figs, null):
    return max([f for f, n in figs if n == null] or [0.0])
