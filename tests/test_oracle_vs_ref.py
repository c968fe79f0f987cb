"""CPU: the oracle against the REAL reference kernels.

The reference's outputs on these inputs are recorded in tests/golden/ref_outputs.json (tests/tools/make_ref_outputs.py, run with
oracle/_ref, which is compiled from the reference tree by oracle/Makefile): the oracle must reproduce them bit for bit.  Where
oracle/_ref is built, the live reference kernels are held to the same recording as well.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle as o
from conftest import GOLDEN, f32_hex


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "ref_outputs.json")) as f:
        return json.load(f)


def digest(v, s, m):
    """float bits of the global value, the fp64 sum exactly, sha256 of the map's bytes"""
    return {"ssim_hex": f32_hex(v), "sum": float(s).hex(), "map_sha256": hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest() if m is not None else None}


def random_pairs():
    rng = np.random.default_rng(1234)
    for (h, w) in ((1, 1), (5, 7), (63, 255), (64, 256), (65, 257), (130, 600), (300, 301)):
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        kind = rng.integers(0, 3)
        if kind == 0:
            b = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif kind == 1:
            b = np.clip(a.astype(np.int32) + rng.integers(-9, 10, (h, w)), 0, 255).astype(np.uint8)
        else:
            b = (a // 2 + 40).astype(np.uint8)
        yield a, b


def flat_pairs():
    for va, vb in ((0, 0), (255, 255), (0, 255), (17, 18)):
        yield np.full((70, 300), va, np.uint8), np.full((70, 300), vb, np.uint8)


def naive_pair():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (97, 131), dtype=np.uint8)
    b = np.clip(a.astype(np.int32) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    return a, b


@pytest.mark.parametrize("impl,fused", [(5, True), (4, False)])
def test_random_images_bit_exact(recorded, impl, fused):
    want = recorded["random_images"][str(impl)]
    pairs = list(random_pairs())
    assert len(want) == len(pairs)
    for (a, b), ref in zip(pairs, want):
        assert digest(*o.ssim_f32(a, b, want_map=True, fused=fused)) == ref, a.shape
        if o.have_ref():
            assert digest(*o.ref_ssim(a, b, want_map=True, impl=impl)) == ref, a.shape


def test_flat_and_extreme_images_bit_exact(recorded):
    want = recorded["flat_images"]
    pairs = list(flat_pairs())
    assert len(want) == len(pairs)
    for (a, b), ref in zip(pairs, want):
        assert digest(*o.ssim_f32(a, b, want_map=True)) == ref, (a[0, 0], b[0, 0])
        if o.have_ref():
            assert digest(*o.ref_ssim(a, b, want_map=True)) == ref, (a[0, 0], b[0, 0])


def test_naive_f64_identical(recorded):
    a, b = naive_pair()
    v, _, m = o.ssim_naive_f64(a, b, want_map=True)
    assert digest(v, v, m) == recorded["naive_f64"]         # "sum": the double value itself, exactly
    if o.have_ref():
        rv, rm = o.ref_naive_f64(a, b, want_map=True)
        assert digest(rv, rv, rm) == recorded["naive_f64"]


def test_reference_openmp_path_same_float(recorded):
    a, b = o.synth_pair(1920, 1080, 0x5EED)
    want = recorded["openmp_1080p_5eed"]
    assert want["1"] == want["8"] == "0x3f64bb1f"
    for t in (1, 8):
        assert f32_hex(o.ssim_f32(a, b, threads=t)[0]) == want[str(t)]
        if o.have_ref():
            assert f32_hex(o.ref_ssim(a, b, threads=t)[0]) == want[str(t)]
