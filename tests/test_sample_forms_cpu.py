"""CPU: the fp32 emulation of every model stays inside the GPU bounds on the exact inputs of tests/test_gpu_sample_forms.py
(tests/sample_forms_inputs.py), and every address those tests hand to a kernel lies inside its column volume.

The GPU module asserts the bounds the families' own GPU tests assert on dense images.  Those bounds were measured on the golden pairs;
here the emulations (the kernels' arithmetic restated in numpy) are run on the seeded random pairs the layout cases use, so that a miss
on the GPU means the kernel and not the inputs.
"""
import numpy as np
import pytest

import halfmodel as HM
import msssimf_model as MS
import sample_forms_inputs as IN
import ssim16_model as M16
import ssimf_model as MF
import ssimw_model as MW
from test_gpu_ssim16 import G_TOL as G16_TOL, PX_TOL as PX16_TOL

SHAPES = pytest.mark.parametrize("shape", IN.SHAPES, ids=["130x19", "3x300"])


def _rel(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


@SHAPES
def test_ssimf_emulation_is_inside_the_gpu_bounds(shape):
    a, b = IN.pair_f(shape)
    v, m, ga, gb = MF.emulate_fp32(a, b, IN.RANGE, IN.G_OUT)
    gv, gm = IN.model(("ssimf", shape))
    da, db = IN.model(("ssimf_grad", shape))
    px, g, ea, eb = float(np.abs(m.astype(np.float64) - gm).max()), abs(v - gv), _rel(ga, da), _rel(gb, db)
    print("ssimf %s: per pixel %.3g (%.3g), global %.3g (%.3g), gradient %.3g / %.3g (%.3g)" % (shape, px, MF.PX_TOL, g, MF.G_TOL, ea, eb, MF.GRAD_TOL))
    assert px <= MF.PX_TOL and g <= MF.G_TOL and max(ea, eb) <= MF.GRAD_TOL


@SHAPES
@pytest.mark.parametrize("enc", HM.ENCODINGS)
def test_ssimf_emulation_on_the_widened_half_planes_is_inside_the_gpu_bounds(shape, enc):
    """ssimh is held to ssimf on the widened planes bit for bit; this ties those planes to the float64 definition."""
    _, (fa, fb) = IN.pair_h(shape, enc)
    v, m = MF.emulate_fp32(fa, fb, IN.RANGE)
    gv, gm = MF.ssim(fa, fb, IN.RANGE)
    assert float(np.abs(m.astype(np.float64) - gm).max()) <= MF.PX_TOL and abs(v - gv) <= MF.G_TOL


@SHAPES
@pytest.mark.parametrize("depth", IN.DEPTHS)
def test_ssim16_emulation_is_inside_the_gpu_bounds(shape, depth):
    a, b = IN.pair_16(shape, depth)
    v, m = M16.emulate_fp32(a, b, depth)
    gv, gm = IN.model(("ssim16", shape, depth))
    px, g = float(np.abs(m.astype(np.float64) - gm).max()), abs(v - gv)
    print("ssim16/%d %s: per pixel %.3g (%.3g), global %.3g (%.3g)" % (depth, shape, px, PX16_TOL, g, G16_TOL))
    assert px <= PX16_TOL and g <= G16_TOL


@SHAPES
def test_map_gradient_emulation_is_inside_the_gpu_bound(shape):
    a, b = IN.pair_f(shape)
    ga, gb = MW.emulate_fp32_map_grad(a, b, IN.RANGE, IN.gmap(shape))
    da, db = IN.model(("ssimw", shape))
    assert not MW.is_null(da, IN.gmap(shape), IN.RANGE)
    ea, eb = _rel(ga, da), _rel(gb, db)
    print("ssimw %s: gradient %.3g / %.3g (%.3g)" % (shape, ea, eb, MW.WGRAD_TOL))
    assert max(ea, eb) <= MW.WGRAD_TOL


@SHAPES
@pytest.mark.parametrize("name,scales,weights", IN.MS_CONFIGS, ids=[c[0] for c in IN.MS_CONFIGS])
def test_msssimf_emulation_is_inside_the_gpu_bounds(shape, name, scales, weights):
    a, b = IN.pair_f(shape)
    emu = MS.Emulation(a, b, IN.RANGE)
    v, m = emu.msssim(scales, weights)
    ga, gb = emu.grad(IN.G_OUT, scales, weights)
    gv, gm = IN.model(("msssimf", shape, name))
    da, db = IN.model(("msssimf_grad", shape, name))
    dv, dm, ea, eb = abs(v - gv), float(np.abs(m - gm).max()), _rel(ga, da), _rel(gb, db)
    print("msssimf/%s %s: value %.3g (%.3g), means %.3g (%.3g), gradient %.3g / %.3g (%.3g)" % (name, shape, dv, MS.VALUE_TOL, dm, MS.MEAN_TOL, ea, eb, MS.GRAD_TOL))
    assert gv > 0.05                                       # away from the relu: the gradient is not switched off
    assert dv <= MS.VALUE_TOL and dm <= MS.MEAN_TOL and max(ea, eb) <= MS.GRAD_TOL


def test_emulations_on_the_129_column_crop_are_inside_the_gpu_bounds():
    """test_device_resident_map_layouts also runs the first 129 columns of the 130 x 19 pairs (an odd width); 130 is the pair itself."""
    a, b = IN.crop(IN.pair_f(IN.BIG), 129)
    v, m = MF.emulate_fp32(a, b, IN.RANGE)
    gv, gm = MF.ssim(a, b, IN.RANGE)
    assert float(np.abs(m.astype(np.float64) - gm).max()) <= MF.PX_TOL and abs(v - gv) <= MF.G_TOL
    for enc in HM.ENCODINGS:
        fa, fb = IN.crop(IN.pair_h(IN.BIG, enc)[1], 129)
        v, m = MF.emulate_fp32(fa, fb, IN.RANGE)
        gv, gm = MF.ssim(fa, fb, IN.RANGE)
        assert float(np.abs(m.astype(np.float64) - gm).max()) <= MF.PX_TOL and abs(v - gv) <= MF.G_TOL, enc
    for depth in IN.DEPTHS:
        a, b = IN.crop(IN.pair_16(IN.BIG, depth), 129)
        v, m = M16.emulate_fp32(a, b, depth)
        gv, gm = M16.ssim(a.astype(np.int64), b.astype(np.int64), depth)
        assert float(np.abs(m.astype(np.float64) - gm).max()) <= PX16_TOL and abs(v - gv) <= G16_TOL, depth


def test_every_view_of_a_column_volume_stays_inside_it():
    """The layout arithmetic of the GPU module, without a device: whatever (offset, step, stride) a view hands out, the elements it
    addresses are the plane's own, inside the buffer, in the image's orientation, for every reading direction and step."""
    rng = np.random.default_rng(1)
    for step in (IN.EDGE, IN.EDGE - 1, IN.EDGE_H, 3000):
        lay = IN.Layout(np.float32, step, 130)
        imgs = [rng.random(s, dtype=np.float32) for s in IN.SHAPES]
        names = [lay.add("p%d" % i, img) for i, img in enumerate(imgs)]
        lay.close(64)
        seen = np.zeros(lay.end * 130, bool)                       # (column, row) pairs any plane owns
        for img, name in zip(imgs, names):
            h, w = img.shape
            for fx in (False, True):
                for fy in (False, True):
                    row0 = lay.rows[(name, fx, fy)]
                    off, dstep, dstride = lay.view(row0, h, w, fx, fy)
                    idx = off + np.arange(h)[:, None] * dstride + np.arange(w)[None, :] * dstep
                    assert idx.min() >= 0 and idx.max() < lay.n
                    assert np.array_equal(idx[::-1 if fy else 1, ::-1 if fx else 1], lay.index(row0, h, w))
                    key = (idx // step) * lay.end + idx % step
                    assert not seen[key].any()                      # no two planes share an element
                    seen[key] = True
        r = lay.claim(19)
        assert lay.in_rows <= r and r + 19 <= lay.end and lay.end < step
    host = lay.build(np.float32(np.nan), np.float32(-3.0))
    for img, name in zip(imgs, names):
        off, dstep, dstride = lay.view(lay.rows[(name, True, False)], img.shape[0], img.shape[1], True, False)
        got = host[off + np.arange(img.shape[0])[:, None] * dstride + np.arange(img.shape[1])[None, :] * dstep]
        assert np.array_equal(got, img)                            # a mirrored view sees the image itself
    assert np.all(host[lay.index(r, 19, 130)] == np.float32(-3.0))
