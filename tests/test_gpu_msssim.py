"""GPU: multi-scale SSIM (rmgr_ssim_hip_compute_msssim_device / _host) against its float64 definition (tests/msssim_model.py).

Bounds: every per-scale mean and the final value within TOL of the model on the golden fixtures, one pair per reference image set
and tiny / thin random pairs; on images of at least 1920 x 1080 the scale-0 means and the final value within TOL_LARGE.  TOL started
at 1e-5 (from MODE_SEPARABLE's measured global error, 9.4e-7, README); the first MI355X run measured 5.93e-7 on the fixtures over
scales 1..8 -- what an fp32 model of the kernels predicts, which also puts the tiny random pairs at 1.19e-6 -- so it is 3e-6 now.
Determinism: a pair gives the same bits alone, inside a batch of 33, through either entry point, in any sub-batch split and on
every call; a view with negative step / stride the same bits as its pixels uploaded contiguously.
"""
import os
import subprocess

import numpy as np
import pytest

import msssim_model as M
import ssim_amd
from conftest import GOLDEN, ROOT, image_entries, load_pair, refset_pair

pytestmark = pytest.mark.gpu

TOL = 3e-6
TOL_LARGE = 2e-6
CLI = os.environ.get("RMGR_SSIM_CLI") or os.path.join(ROOT, "ssim_amd", "bin", "rmgr-ssim")


def weights_for(scales):
    return None if scales == 5 else [1.0 / scales] * scales


def check_against_model(a, b, scales, weights, tol, name):
    v, means = ssim_amd.compute_msssim(a, b, scales=scales, weights=weights, per_scale=True)
    mv, mmeans = M.msssim(a, b, scales=scales, weights=weights)
    assert means.shape == (scales, 2)
    err = max(abs(float(v) - mv), float(np.abs(means - mmeans).max()))
    assert err <= tol, (name, scales, err, float(v), mv)
    return err


class DevicePairs(object):
    """Pairs uploaded to the device once; params() builds descriptors (any order, repeats allowed) over them."""

    def __init__(self, ctx, pairs):
        self.shape = pairs[0][0].shape
        self.bufs = [(ctx.upload(a), ctx.upload(b)) for a, b in pairs]

    def params(self, order):
        h, w = self.shape
        ps = (ssim_amd.Params * len(order))()
        for i, k in enumerate(order):
            da, db = self.bufs[k]
            ps[i] = ssim_amd.make_params(w, h, da.ptr, 1, w, db.ptr, 1, w)
        return ps

    def free(self):
        for da, db in self.bufs:
            da.free()
            db.free()


def test_golden_fixtures_every_scale_count(manifest):
    worst = 0.0
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        for scales in range(1, 9):
            worst = max(worst, check_against_model(a, b, scales, weights_for(scales), TOL, n))
    print("golden fixtures, scales 1..8: worst |gpu - model| = %.3g" % worst)


def test_custom_weights(manifest):
    a, b = load_pair(manifest["bbb257x65_q50_ch1"])
    for w in ([0.5, 0.0, 0.25, 0.25], [0.0, 0.0, 0.0, 1.0], [2.0, 0.1, 0.3]):
        check_against_model(a, b, len(w), w, TOL, "weights %s" % w)
    assert float(ssim_amd.compute_msssim(a, b, scales=3, weights=[0.0, 0.0, 0.0])) == 1.0


@pytest.mark.parametrize("set_name", ["bbb255", "bbb257", "bbb360", "bbb1080"])
def test_one_pair_per_reference_set(refsets, set_name):
    a, b = refset_pair(refsets[set_name]["pairs"]["q50_ch1"])
    for scales in (5, 8):
        check_against_model(a, b, scales, weights_for(scales), TOL, set_name)
    if a.shape[0] >= 1080 and a.shape[1] >= 1920:
        v, means = ssim_amd.compute_msssim(a, b, per_scale=True)
        mv, mmeans = M.msssim(a, b)
        assert abs(float(v) - mv) <= TOL_LARGE and np.abs(means[0] - mmeans[0]).max() <= TOL_LARGE, (float(v) - mv, means[0] - mmeans[0])


def test_einstein_set(manifest):
    a, b = load_pair(manifest["einstein_jpg"])
    for scales in (5, 8):
        check_against_model(a, b, scales, weights_for(scales), TOL, "einstein_jpg")


@pytest.mark.parametrize("shape", [(1, 1), (1, 200), (200, 1), (63, 255), (2, 3), (17, 65)])
def test_tiny_and_thin_sizes(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    a = rng.integers(0, 256, shape).astype(np.uint8)
    b = np.clip(a.astype(np.int32) + rng.integers(-40, 41, shape), 0, 255).astype(np.uint8)
    for scales in (1, 5, 8):
        check_against_model(a, b, scales, weights_for(scales), TOL, str(shape))


def test_negative_step_and_stride_views_give_the_same_bits(gpu_ctx, manifest):
    a, b = load_pair(manifest["bbb255x63_q00_ch2"])
    h, w = a.shape
    fa, fb = np.ascontiguousarray(a[::-1, ::-1]), np.ascontiguousarray(b[::-1, ::-1])
    v_view, m_view = ssim_amd.compute_msssim(a[::-1, ::-1], b[::-1, ::-1], per_scale=True)      # host: negative step and stride
    v_copy, m_copy = ssim_amd.compute_msssim(fa, fb, per_scale=True)
    assert np.float32(v_view).tobytes() == np.float32(v_copy).tobytes() and m_view.tobytes() == m_copy.tobytes()
    # the device entry: the original pixels, addressed backwards
    da, db = gpu_ctx.upload(a), gpu_ctx.upload(b)
    try:
        p = (ssim_amd.Params * 1)()
        p[0] = ssim_amd.make_params(w, h, da.ptr + (h - 1) * w + (w - 1), -1, -w, db.ptr + (h - 1) * w + (w - 1), -1, -w)
        v_dev, m_dev = gpu_ctx.msssim_device(p, 1, per_scale=True)
    finally:
        da.free()
        db.free()
    assert v_dev[0].tobytes() == np.float32(v_copy).tobytes() and m_dev[0].tobytes() == m_copy.tobytes()
    # a column view (step = row pitch) against its transposed copy
    v_t = ssim_amd.compute_msssim(a.T, b.T)
    v_tc = ssim_amd.compute_msssim(np.ascontiguousarray(a.T), np.ascontiguousarray(b.T))
    assert np.float32(v_t).tobytes() == np.float32(v_tc).tobytes()


def test_alone_in_a_batch_host_device_and_repeated_calls_are_bit_identical(gpu_ctx, manifest):
    a, b = load_pair(manifest["bbb257x65_q50_ch0"])
    rng = np.random.default_rng(33)
    pairs = [(a, b)] + [(rng.integers(0, 256, a.shape).astype(np.uint8), rng.integers(0, 256, a.shape).astype(np.uint8)) for _ in range(4)]
    alone_v, alone_m = ssim_amd.compute_msssim(a, b, per_scale=True)                 # host entry, default context
    order = [(i * 7) % 5 for i in range(33)]
    order[17] = 0
    dev = DevicePairs(gpu_ctx, pairs)
    try:
        bv, bm = gpu_ctx.msssim_device(dev.params(order), 33, per_scale=True)
        bv2, bm2 = gpu_ctx.msssim_device(dev.params(order), 33, per_scale=True)
        one_v, one_m = gpu_ctx.msssim_device(dev.params([0]), 1, per_scale=True)
    finally:
        dev.free()
    hits = 0
    for i, k in enumerate(order):
        if k == 0:
            assert bv[i].tobytes() == np.float32(alone_v).tobytes() and bm[i].tobytes() == alone_m.tobytes(), i
            hits += 1
    assert hits >= 2
    assert bv.tobytes() == bv2.tobytes() and bm.tobytes() == bm2.tobytes()
    assert one_v[0].tobytes() == np.float32(alone_v).tobytes() and one_m[0].tobytes() == alone_m.tobytes()
    hv, hm = ssim_amd.compute_msssim_batch([pairs[k] for k in order], per_scale=True, ctx=gpu_ctx)      # host batch entry
    assert hv.tobytes() == bv.tobytes() and hm.tobytes() == bm.tobytes()


def test_large_pairs_and_sub_batch_split(gpu_ctx):
    """16 pairs of 4096^2 through the host entry run in two sub-batches (the ~1 GB scratch cap), through the device entry in one;
    the first pair against the model on the host."""
    from ssim_amd import synth
    pairs = [synth.pair_numpy(4096, 4096, seed=s) for s in (1, 2, 3)]
    order = [i % 3 for i in range(16)]
    dev = DevicePairs(gpu_ctx, pairs)
    try:
        dv, dm = gpu_ctx.msssim_device(dev.params(order), 16, per_scale=True)
    finally:
        dev.free()
    hv, hm = ssim_amd.compute_msssim_batch([pairs[k] for k in order], per_scale=True, ctx=gpu_ctx)
    assert hv.tobytes() == dv.tobytes() and hm.tobytes() == dm.tobytes()
    a, b = pairs[0]
    mv, mmeans = M.msssim(a, b)
    assert abs(float(dv[0]) - mv) <= TOL_LARGE and np.abs(dm[0][0] - mmeans[0]).max() <= TOL_LARGE, (float(dv[0]) - mv, dm[0][0] - mmeans[0])
    assert np.abs(dm[0] - mmeans).max() <= TOL


def test_identical_images_give_one(manifest):
    a, _ = load_pair(manifest["einstein_blur"])
    for scales in (1, 5, 8):
        v = ssim_amd.compute_msssim(a, a, scales=scales, weights=weights_for(scales))
        assert abs(float(v) - 1.0) <= 1e-6, (scales, float(v))


def test_single_scale_is_the_engines_double_ssim(gpu_ctx, manifest):
    gpu_ctx.set_mode(ssim_amd.MODE_DOUBLE)
    try:
        for n in ("bbb255x63_q00_ch0", "bbb257x65_q50_ch2", "einstein_jpg", "einstein_impulse"):
            a, b = load_pair(manifest[n])
            ref, _ = gpu_ctx.ssim_planes(a, b)
            v = ssim_amd.compute_msssim(a, b, scales=1, weights=[1.0])
            assert abs(float(v) - float(ref)) <= 2e-6, (n, float(v), float(ref))
    finally:
        gpu_ctx.set_mode(ssim_amd.MODE_EXACT)


def test_the_context_mode_does_not_change_msssim(gpu_ctx, manifest):
    a, b = load_pair(manifest["bbb255x63_q50_ch0"])
    dev = DevicePairs(gpu_ctx, [(a, b)])
    try:
        base = gpu_ctx.msssim_device(dev.params([0]), 1)
        for mode in (ssim_amd.MODE_DOUBLE, ssim_amd.MODE_SEPARABLE, ssim_amd.MODE_FAST):
            gpu_ctx.set_mode(mode)
            assert gpu_ctx.msssim_device(dev.params([0]), 1).tobytes() == base.tobytes()
    finally:
        gpu_ctx.set_mode(ssim_amd.MODE_EXACT)
        dev.free()


def test_cli_msssim_matches_the_binding(tmp_path, manifest):
    il = manifest["_interleaved"]
    w, h = il["width"], il["height"]
    a = np.fromfile(os.path.join(GOLDEN, il["a"]), np.uint8).reshape(h, w, 3)
    b = np.fromfile(os.path.join(GOLDEN, il["b"]), np.uint8).reshape(h, w, 3)
    pa, pb = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm")
    open(pa, "wb").write(b"P6\n%d %d\n255\n" % (w, h) + a.tobytes())
    open(pb, "wb").write(b"P6\n%d %d\n255\n" % (w, h) + b.tobytes())
    r = subprocess.run([CLI, "-m", pa, pb], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    vals = [np.float32(ssim_amd.compute_msssim(a[:, :, c], b[:, :, c])) for c in range(3)]
    total = np.float32(0)
    for v in vals:
        total = np.float32(total + v)
    want = "".join("Channel %u: % 7.4f\n" % (c, vals[c]) for c in range(3)) + "Average  : % 7.4f\n" % np.float32(total / np.float32(3))
    assert r.stdout == want, (r.stdout, want)
    ga, gb = str(tmp_path / "a.pgm"), str(tmp_path / "b.pgm")                 # one channel: the bare line
    open(ga, "wb").write(b"P5\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(a[:, :, 1]).tobytes())
    open(gb, "wb").write(b"P5\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(b[:, :, 1]).tobytes())
    r = subprocess.run([CLI, "-m", ga, gb], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "% 7.4f\n" % vals[1], (r.stdout, r.stderr)
