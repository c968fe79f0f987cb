"""CPU: what tests/test_gpu_tall_strips.py rests on, checked without a device.

  * tests/sample_plan.py restates the strip planners of the five sample families.  A small host program (tests/src/plan_probe.cpp, its
    own main, no HIP call) is linked against the project's built kernel objects and prints what plan16 / planf / planh / plank /
    strip_rows_of choose; the restatement must agree on the shapes of the GPU module, on a few hundred seeded random launches with
    heights on both sides of 2048, and for 64, 128, 256 and 304 CUs.
  * On a 256-CU device the three launch shapes of the GPU module have the strips its docstring describes.
  * The fp32 emulation of every model stays inside the bounds the GPU module asserts on the exact pairs it uses
    (tests/tall_strips_inputs.py), so that a miss on the GPU means the kernel and not the inputs.
"""
import os
import subprocess

import numpy as np
import pytest

import halfmodel as HM
import msssimf_model as MS
import sample_forms_inputs as IN
import sample_plan as SP
import ssim16_model as M16
import ssimf_model as MF
import ssimk_model as K
import tall_strips_inputs as T
from conftest import ROOT
from test_gpu_ssim16 import G_TOL as G16_TOL, PX_TOL as PX16_TOL

HIPCC = "/opt/rocm/bin/hipcc"
KERNEL_OBJECTS = ["build/obj/%s_kernels.o" % n for n in ("ssim16", "ssimf", "ssimh", "ssimk", "msssimf")]
CUS = (64, 128, 256, 304)
BY_SHAPE = pytest.mark.parametrize("shape", T.SHAPES, ids=T.shape_id)
BY_WINDOW = pytest.mark.parametrize("window", K.WINDOWS, ids=K.name_of)


# ---- 1. the restatement against the C++ ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """The probe, linked against the kernel objects of the library under test (the Makefile's own rules bring them up to date: nothing
    to do after a build)."""
    r = subprocess.run(["make", "-C", ROOT, "-j5"] + KERNEL_OBJECTS, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path_factory.mktemp("plan_probe")
    obj, exe = str(out / "plan_probe.o"), str(out / "plan_probe")
    src = os.path.join(ROOT, "tests", "src", "plan_probe.cpp")
    for cmd in ([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                 "-I" + os.path.join(ROOT, "ssim_amd", "csrc"), "-c", src, "-o", obj],
                [HIPCC, "--offload-arch=gfx950", obj] + [os.path.join(ROOT, o) for o in KERNEL_OBJECTS] + ["-o", exe]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]

    def run(rows):
        """rows: (family, radius, W, H, count, CUs) -> [(cell_rows, strip_rows, strips_x, strips_y, cells_y)]."""
        text = "".join("%s %d %d %d %d %d\n" % row for row in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        assert len(got) == len(rows)
        return got
    return run


def launches():
    """(W, H, count): the launches of the GPU module, alone and at every scale of msssimf's pyramid, and 300 seeded random ones."""
    out = []
    for _, w, h, n in T.CASES:
        for s in range(5):
            out += [(SP.msf_dim(w, s), SP.msf_dim(h, s), n), (SP.msf_dim(w, s), SP.msf_dim(h, s), 1)]
    out.append((T.GRAD_SHAPE[1], T.GRAD_SHAPE[0], T.GRAD_COUNT))
    rng = np.random.default_rng(20261019)
    for i in range(300):
        kind = i % 3
        if kind == 0:                              # anything, heights on both sides of 2048
            w, h = int(rng.integers(1, 1200)), int(rng.integers(1, 6000))
        elif kind == 1:                            # at the change of the cell height
            w, h = int(rng.integers(1, 400)), int(rng.integers(2048 - 40, 2048 + 40))
        else:                                      # small images in large batches: the tall strips of the GPU module
            w, h = int(rng.integers(1, 300)), int(rng.integers(1, 2600))
        n = int(rng.choice([1, 2, 3, 7, 16, 70, 140, 300, 350, 1000, 2000, 5000])) if kind else int(rng.integers(1, 3000))
        out.append((w, h, n))
    return out


def test_the_restatement_agrees_with_the_planners(probe):
    rows = []
    for w, h, n in launches():
        for cus in CUS:
            rows += [(fam, 0, w, h, n, cus) for fam in SP.FAMILIES if fam != "ssimk"]
            rows += [("ssimk", radius, w, h, n, cus) for radius in (1, 2, 3, 4)]
    rows += [(fam, 1, 9, 603, 1000, 0) for fam in SP.FAMILIES]               # no CU count known: 256
    got = probe(rows)
    tall = both = 0
    for row, (cell_rows, strip_rows, strips_x, strips_y, cells_y) in zip(rows, got):
        fam, radius, w, h, n, cus = row
        geo = SP.plan(fam, w, h, n, cus, radius)
        assert (strip_rows, strips_x, strips_y) == geo[1:], (row, got, geo)
        assert cell_rows in (0, geo.cell_rows) and (cell_rows != 0 or fam == "msssimf"), (row, cell_rows, geo)
        assert cells_y == (h + geo.cell_rows - 1) // geo.cell_rows, (row, cells_y)
        assert strip_rows % geo.cell_rows == 0 and geo.cell_rows <= strip_rows <= max(geo.cell_rows, SP.MAX_STRIP_ROWS)
        tall += SP.cells_per_strip(geo, h) > SP.CELL_BATCH
        both += geo.cell_rows == 32 and SP.cells_per_strip(geo, h) > 1
    assert tall > 1000 and both > 1000, (tall, both)       # the grid is not one of single-cell strips
    print("\n%d launches agree; %d with more than %d cells per strip, %d with several 32-row cells" % (len(rows), tall, SP.CELL_BATCH, both))


def test_radius_5_is_planned_as_the_11_tap_kernels():
    for _, w, h, n in T.CASES:
        assert SP.plank(5, w, h, n, 256) == SP.planf(w, h, n, 256)


# ---- 2. the launch shapes of the GPU module on 256 CUs ------------------------------------------------------------------------------

def geometries(w, h, n, cus=256):
    return [(fam, radius, SP.plan(fam, w, h, n, cus, radius)) for fam in SP.FAMILIES for radius in ((1, 2, 3, 4, 5) if fam == "ssimk" else (0,))]


def test_the_three_launch_shapes_on_256_cus():
    (_, wa, ha, na), (_, wb, hb, nb), (_, wc, hc, nc) = T.CASES
    for fam, radius, g in geometries(wa, ha, na):
        assert g == SP.Geometry(8, 208, 1, 3), (fam, radius, g)
        assert SP.cells_per_strip(g, ha) == 26 and SP.full_flushes(26) == (3, 2)
        assert (SP.last_strip_rows(g, ha), SP.last_strip_cells(g, ha), SP.last_cell_rows(g, ha)) == (187, 24, 3)
    for fam, radius, g in geometries(wb, hb, nb):
        assert g == SP.Geometry(32, 736, 1, 3), (fam, radius, g)
        assert SP.cells_per_strip(g, hb) == 23
        assert (SP.last_strip_rows(g, hb), SP.last_strip_cells(g, hb), SP.last_cell_rows(g, hb)) == (643, 21, 3)
    for fam, radius, g in geometries(wc, hc, nc):
        assert g == SP.Geometry(8, 56, 3, 11), (fam, radius, g)
        assert SP.cells_per_strip(g, hc) == 7
        assert (SP.last_strip_rows(g, hc), SP.last_strip_cells(g, hc), SP.last_cell_rows(g, hc)) == (41, 6, 1)
    # what the references of the GPU module are: one pair alone is single-cell strips
    for _, w, h, _ in T.CASES:
        for fam, radius, g in geometries(w, h, 1):
            assert SP.cells_per_strip(g, h) == 1, (fam, radius, w, h, g)
    # the shape tests/test_gpu_sample_forms.py once took for a multi-cell one
    assert SP.cells_per_strip(SP.planf(3, 300, 1, 256), 300) == 1


def test_the_helpers_on_an_image_of_one_strip():
    g = SP.planf(100, 20, 100000, 256)            # more strips than any height saves rounds for: one strip per image
    assert g.strips_y == 1 and SP.cells_per_strip(g, 20) == 3 and SP.last_strip_rows(g, 20) == 20 and SP.last_cell_rows(g, 20) == 4
    assert SP.last_cell_rows(SP.planf(100, 16, 1, 256), 16) == 8 and SP.full_flushes(16) == (2, 0)


# ---- 3. the emulations on the pairs of the GPU module -------------------------------------------------------------------------------

def _rel(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def _px(m, gm):
    return float(np.abs(m.astype(np.float64) - gm).max())


@BY_SHAPE
def test_ssimf_emulation_is_inside_the_gpu_bounds(shape):
    worst = [0.0, 0.0]
    for k, (a, b) in enumerate(T.pairs_f(shape)):
        v, m = MF.emulate_fp32(a, b, T.RANGE)
        gv, gm = T.model_f(shape, k)
        worst = [max(worst[0], _px(m, gm)), max(worst[1], abs(v - gv))]
    print("ssimf %s: per pixel %.3g (%.3g), global %.3g (%.3g)" % (T.shape_id(shape), worst[0], MF.PX_TOL, worst[1], MF.G_TOL))
    assert worst[0] <= MF.PX_TOL and worst[1] <= MF.G_TOL


@BY_SHAPE
@pytest.mark.parametrize("enc", HM.ENCODINGS)
def test_ssimf_emulation_on_the_widened_half_planes_is_inside_the_gpu_bounds(shape, enc):
    """ssimh is held to ssimf on the widened planes bit for bit; this ties those planes to the float64 definition."""
    for _, (fa, fb) in T.pairs_h(shape, enc):
        v, m = MF.emulate_fp32(fa, fb, T.RANGE)
        gv, gm = MF.ssim(fa, fb, T.RANGE)
        assert _px(m, gm) <= MF.PX_TOL and abs(v - gv) <= MF.G_TOL


@BY_SHAPE
@pytest.mark.parametrize("depth", IN.DEPTHS)
def test_ssim16_emulation_is_inside_the_gpu_bounds(shape, depth):
    worst = [0.0, 0.0]
    for k, (a, b) in enumerate(T.pairs_16(shape, depth)):
        v, m = M16.emulate_fp32(a, b, depth)
        gv, gm = T.model_16(shape, depth, k)
        worst = [max(worst[0], _px(m, gm)), max(worst[1], abs(v - gv))]
    print("ssim16/%d %s: per pixel %.3g (%.3g), global %.3g (%.3g)" % (depth, T.shape_id(shape), worst[0], PX16_TOL, worst[1], G16_TOL))
    assert worst[0] <= PX16_TOL and worst[1] <= G16_TOL


@BY_SHAPE
@pytest.mark.parametrize("name,scales,weights", IN.MS_CONFIGS, ids=[c[0] for c in IN.MS_CONFIGS])
def test_msssimf_emulation_is_inside_the_gpu_bounds(shape, name, scales, weights):
    worst = [0.0, 0.0]
    for k, (a, b) in enumerate(T.pairs_f(shape)):
        v, m = MS.Emulation(a, b, T.RANGE).msssim(scales, weights)
        gv, gm = T.model_ms(shape, k, scales, weights)
        worst = [max(worst[0], float(np.abs(m - gm).max())), max(worst[1], abs(v - gv))]
    print("msssimf/%s %s: means %.3g (%.3g), value %.3g (%.3g)" % (name, T.shape_id(shape), worst[0], MS.MEAN_TOL, worst[1], MS.VALUE_TOL))
    assert worst[0] <= MS.MEAN_TOL and worst[1] <= MS.VALUE_TOL


@BY_SHAPE
@BY_WINDOW
def test_window_emulation_is_inside_the_gpu_bounds(shape, window):
    """Value and map on every shape; the gradients, for the scalar and the per-pixel upstream form, on the shape of the gradient launches."""
    px_tol, g_tol, grad_tol, _ = K.tolerances(window)
    worst = [0.0, 0.0, 0.0]
    for k, (a, b) in enumerate(T.pairs_f(shape)):
        gv, gm = T.model_k(shape, k, window)
        if shape != T.GRAD_SHAPE:
            v, m = K.emulate_fp32(a, b, T.RANGE, window)
        else:
            v, m, ea, eb = K.emulate_fp32(a, b, T.RANGE, window, g_out=T.G_OUTS[k])
            _, _, pa, pb = K.emulate_fp32(a, b, T.RANGE, window, gmap=T.upstream(shape)[k])
            (wa, wb), (qa, qb) = T.model_k_grad(shape, k, window)
            worst[2] = max(worst[2], _rel(ea, wa), _rel(eb, wb), _rel(pa, qa), _rel(pb, qb))
        worst[:2] = [max(worst[0], _px(m, gm)), max(worst[1], abs(v - gv))]
    print("%s %s: per pixel %.3g (%.3g), global %.3g (%.3g), gradient %.3g (%.3g)" % (
        K.name_of(window), T.shape_id(shape), worst[0], px_tol, worst[1], g_tol, worst[2], grad_tol))
    assert worst[0] <= px_tol and worst[1] <= g_tol and worst[2] <= grad_tol
