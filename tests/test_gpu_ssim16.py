"""GPU: SSIM of 9- to 16-bit samples (rmgr_ssim_hip_enqueue_ssim16, rmgr_ssim_hip_compute_ssim16_device / _host) against its float64
definition (tests/ssim16_model.py), and its determinism.

Bounds.  The per-pixel and global tolerances below are measured, not estimated: an fp32 emulation of the kernel's arithmetic
(ssim16_model.emulate_fp32: the centre per 128-column strip column, the row pass, the column pass and the formula in the kernel's
order) lands within 2.3e-4 per pixel and 6.3e-7 globally of the float64 model on the golden fixtures (x257 at depth 16 and as they
are at depth 8), and within 1.6e-4 / 1.9e-7 on the seeded 10-, 12- and 16-bit pairs below.  The asserted bounds are about twice
that: PX_TOL = 5e-4, G_TOL = 1.3e-6.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ssim16_model as M
import ssim_amd
from conftest import ROOT, image_entries, load_pair

pytestmark = pytest.mark.gpu

PX_TOL = 5e-4
G_TOL = 1.3e-6
ONE_TOL = 4e-7          # n * rcp(d) with n == d: the reciprocal's 1 ulp and the product's rounding
CLI = os.environ.get("RMGR_SSIM_CLI") or os.path.join(ROOT, "ssim_amd", "bin", "rmgr-ssim")


def check(a, b, depth, what, got=None):
    v, m = ssim_amd.compute_ssim16(a, b, depth, want_map=True) if got is None else got
    gv, gm = M.ssim(np.asarray(a, np.int64), np.asarray(b, np.int64), depth)
    dp = float(np.abs(m.astype(np.float64) - gm).max())
    assert dp <= PX_TOL, (what, dp)
    assert abs(float(v) - gv) <= G_TOL, (what, float(v), gv)
    return v, m


def seeded_pairs(depth, rng):
    L = (1 << depth) - 1
    yield "noise", rng.integers(0, L + 1, (96, 300)), rng.integers(0, L + 1, (96, 300))
    yy, xx = np.mgrid[0:96, 0:300]
    sm = L * (0.5 + 0.4 * np.sin(xx / 17.0) * np.cos(yy / 11.0))
    noisy = lambda: np.clip(np.round(sm + rng.normal(0, L * 0.01, sm.shape)), 0, L)
    yield "smooth", noisy(), noisy()
    yield "flat", np.full((40, 130), L // 3), np.full((40, 130), L // 3 + 1)
    yield "zero-vs-L", np.zeros((40, 130)), np.full((40, 130), L)
    base = rng.integers(0, L, (64, 200))
    one = base.copy()
    one[10:20, 30:50] += 1
    yield "one-code", base, one


@pytest.mark.parametrize("depth", [10, 12, 16])
def test_seeded_pairs_match_the_model(depth):
    rng = np.random.default_rng(depth)
    for name, a, b in seeded_pairs(depth, rng):
        check(a.astype(np.uint16), b.astype(np.uint16), depth, "%s/%d" % (name, depth))


def test_golden_fixtures_at_depth_16_and_8(manifest):
    with ssim_amd.Context(0, mode=ssim_amd.MODE_DOUBLE) as ctx:
        for n in image_entries(manifest):
            a, b = load_pair(manifest[n])
            check(a.astype(np.uint16) * 257, b.astype(np.uint16) * 257, 16, n + "/16")
            v8, m8 = check(a.astype(np.uint16), b.astype(np.uint16), 8, n + "/8")
            dv, dm = ctx.ssim_planes(a, b, want_map=True)          # the 8-bit engine, fp64 arithmetic
            assert abs(float(v8) - float(dv)) <= G_TOL, n
            assert float(np.abs(m8.astype(np.float64) - dm).max()) <= PX_TOL, n


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (1, 1000), (999, 3), (9, 200003), (130, 257)])
def test_sizes(shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.integers(0, 4096, shape).astype(np.uint16)
    b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, shape), 0, 4095).astype(np.uint16)
    check(a, b, 12, str(shape))


def test_identical_images_give_one():
    rng = np.random.default_rng(3)
    for depth in (8, 10, 16):
        a = rng.integers(0, 1 << depth, (70, 333)).astype(np.uint16)
        v, m = ssim_amd.compute_ssim16(a, a, depth, want_map=True)
        assert np.abs(m.astype(np.float64) - 1.0).max() <= ONE_TOL and abs(float(v) - 1.0) <= ONE_TOL, depth


def _pairs(rng, n, shape=(150, 260), depth=12):
    L = (1 << depth) - 1
    out = []
    for _ in range(n):
        a = rng.integers(0, L + 1, shape).astype(np.uint16)
        out.append((a, np.clip(a.astype(np.int64) + rng.integers(-200, 201, shape), 0, L).astype(np.uint16)))
    return out


def test_batch_position_size_and_repeat_give_the_same_bits():
    rng = np.random.default_rng(11)
    pairs = _pairs(rng, 9)
    alone = np.array([ssim_amd.compute_ssim16(a, b, 12)[0] for a, b in pairs], np.float32)
    for n in (1, 2, 5, 9):
        got = ssim_amd.compute_ssim16_batch(pairs[:n], 12)
        assert got.tobytes() == alone[:n].tobytes(), n
    rev = ssim_amd.compute_ssim16_batch(pairs[::-1], 12)
    assert rev.tobytes() == alone[::-1].tobytes()
    assert ssim_amd.compute_ssim16_batch(pairs, 12).tobytes() == alone.tobytes()       # every call


def test_sub_batch_split_gives_the_same_bits():
    # eight 6144^2 pairs stage 1.2 GB: more than one sub-batch of the host entry point
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1024, (6144, 6144)).astype(np.uint16)
    b = np.clip(a.astype(np.int64) + rng.integers(-9, 10, a.shape), 0, 1023).astype(np.uint16)
    pairs = [(a, b), (b, a), (a, a), (b, b), (a, b), (b, a), (a, b), (b, a)]
    alone = {k: ssim_amd.compute_ssim16(x, y, 10)[0] for k, (x, y) in {"ab": (a, b), "ba": (b, a), "aa": (a, a), "bb": (b, b)}.items()}
    want = np.array([alone["ab"], alone["ba"], alone["aa"], alone["bb"], alone["ab"], alone["ba"], alone["ab"], alone["ba"]], np.float32)
    assert ssim_amd.compute_ssim16_batch(pairs, 10).tobytes() == want.tobytes()


def test_entry_points_and_negative_views_give_the_same_bits(gpu_ctx):
    rng = np.random.default_rng(21)
    (a, b), = _pairs(rng, 1, (77, 301), 16)
    h, w = a.shape
    v, m = ssim_amd.compute_ssim16(a, b, 16, want_map=True)
    # a view with negative step and stride against the same pixels uploaded contiguously
    va, vm = ssim_amd.compute_ssim16(a[::-1, ::-1], b[::-1, ::-1], 16, want_map=True)
    ca, cm = ssim_amd.compute_ssim16(np.ascontiguousarray(a[::-1, ::-1]), np.ascontiguousarray(b[::-1, ::-1]), 16, want_map=True)
    assert np.float32(va).tobytes() == np.float32(ca).tobytes() and vm.tobytes() == cm.tobytes()
    # device pointers: compute_ssim16_device and enqueue_ssim16 (+ the mean over double(W) * double(H)), the original pixels addressed backwards too
    da, db = gpu_ctx.upload(a), gpu_ctx.upload(b)
    dm = gpu_ctx.alloc(h * w * 4)
    sums = gpu_ctx.alloc(8 * 2)
    try:
        ps = (ssim_amd.Params16 * 2)()
        ps[0] = ssim_amd.make_params16(w, h, da.ptr, 1, w, db.ptr, 1, w, dm.ptr)
        ps[1] = ssim_amd.make_params16(w, h, da.ptr + 2 * (h * w - 1), -1, -w, db.ptr + 2 * (h * w - 1), -1, -w)
        got = gpu_ctx.ssim16_device(ps, 2, 16)
        assert np.float32(got[0]).tobytes() == np.float32(v).tobytes()
        assert gpu_ctx.download(dm.ptr, np.float32, (h, w)).tobytes() == m.tobytes()
        assert np.float32(got[1]).tobytes() == np.float32(ca).tobytes()
        gpu_ctx.enqueue_ssim16(ps, 2, 16, sums.ptr)
        gpu_ctx.synchronize()
        s = gpu_ctx.download(sums.ptr, np.float64, (2,))
        assert np.float32(s[0] / (float(w) * float(h))).tobytes() == np.float32(v).tobytes()
        assert np.float32(s[1] / (float(w) * float(h))).tobytes() == np.float32(ca).tobytes()
    finally:
        for buf in (da, db, dm, sums):
            buf.free()


def test_map_layouts():
    rng = np.random.default_rng(8)
    (a, b), = _pairs(rng, 1, (45, 190), 10)
    h, w = a.shape
    v, dense = ssim_amd.compute_ssim16(a, b, 10, want_map=True)
    lib = ssim_amd.load_library()

    def run(map_ptr, step, stride):
        ps = (ssim_amd.Params16 * 1)()
        ps[0] = ssim_amd.make_params16(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w, map_ptr, step, stride)
        out = (ctypes.c_float * 1)()
        assert lib.rmgr_ssim_hip_compute_ssim16_host(None, 1, ps, 10, out) == 0
        return np.float32(out[0])
    wide = np.full((h, 2 * w), -7.0, np.float32)                                      # ssimStep 2
    assert run(wide.ctypes.data, 2, 2 * w).tobytes() == np.float32(v).tobytes()
    assert wide[:, 0::2].tobytes() == dense.tobytes() and np.all(wide[:, 1::2] == -7.0)
    flip = np.zeros((h, w), np.float32)                                               # negative ssimStride
    run(flip[h - 1].ctypes.data, 1, -w)
    assert flip[::-1].tobytes() == dense.tobytes()
    assert run(None, 1, w).tobytes() == np.float32(v).tobytes()                        # NULL: no map


def test_addressing_beyond_32_bits(gpu_ctx):
    """46341 x 46400 uint16 images: byte offsets pass 2^32 from row 46341 on.  The pair is built on the device from a repeated
    1024-row block (no 4 GB host array); B differs from A in a 10 x 30 patch past that offset."""
    W, H, depth = 46341, 46400, 16
    rng = np.random.default_rng(46341)
    block = rng.integers(0, 1 << depth, (1024, W)).astype(np.uint16)
    nbytes = W * H * 2
    da, db, dm = gpu_ctx.alloc(nbytes), gpu_ctx.alloc(nbytes), gpu_ctx.alloc(W * H * 4)
    try:
        lib = gpu_ctx.lib
        for r0 in range(0, H, 1024):
            rows = min(1024, H - r0)
            for buf in (da, db):
                assert lib.rmgr_ssim_hip_memcpy_h2d(gpu_ctx.handle, buf.ptr + r0 * W * 2, block.ctypes.data, rows * W * 2) == 0
        y0, y1, x0, x1 = 46370, 46380, 20000, 20030
        assert y0 * W * 2 > 1 << 32
        full = lambda y: block[y % 1024]
        for y in range(y0, y1):
            row = full(y).copy()
            row[x0:x1] = (row[x0:x1].astype(np.int64) * 7 + 12345).astype(np.uint16)
            assert lib.rmgr_ssim_hip_memcpy_h2d(gpu_ctx.handle, db.ptr + y * W * 2, row.ctypes.data, W * 2) == 0
        ps = (ssim_amd.Params16 * 1)()
        ps[0] = ssim_amd.make_params16(W, H, da.ptr, 1, W, db.ptr, 1, W, dm.ptr)
        v = gpu_ctx.ssim16_device(ps, 1, depth)[0]
        # the crop around the patch, with a 20-pixel margin (down to the image's bottom edge, which clamps like the full image)
        cy0, cy1, cx0, cx1 = y0 - 20, H, x0 - 20, x1 + 20
        ca = np.stack([full(y)[cx0:cx1] for y in range(cy0, cy1)]).astype(np.int64)
        cb = ca.copy()
        cb[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0] = (cb[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0] * 7 + 12345) % 65536
        _, gm = M.ssim(ca, cb, depth)
        got = np.stack([gpu_ctx.download(dm.ptr + (y * W + cx0) * 4, np.float32, (cx1 - cx0,)) for y in range(cy0, cy1)])
        inner = (slice(10, None), slice(10, -10))           # at least 10 pixels from the crop's cut edges
        assert float(np.abs(got[inner].astype(np.float64) - gm[inner]).max()) <= PX_TOL
        assert got[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0].max() < 0.9             # the patch is seen
        # away from the patch the map is 1: whole rows above it, below 2^32 and beyond, and the patch rows outside the patch
        for y in (0, 1, 23000, 46339, 46340, 46341, 46345, 46399):
            row = gpu_ctx.download(dm.ptr + y * W * 4, np.float32, (W,))
            assert np.abs(row.astype(np.float64) - 1.0).max() <= ONE_TOL, y
        row = gpu_ctx.download(dm.ptr + y0 * W * 4, np.float32, (W,))
        far = np.r_[0:x0 - 6, x1 + 6:W]
        assert np.abs(row[far].astype(np.float64) - 1.0).max() <= ONE_TOL
        assert 0.0 < 1.0 - float(v) < 1e-4
    finally:
        for buf in (da, db, dm):
            buf.free()


# ---- the command-line tool ----

def _write_png16(path, img):
    import struct
    import zlib
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[ch]
    raw = b"".join(b"\0" + img[y].astype(">u2").tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, ctype, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def _write_pnm16(path, img, maxval):
    h, w = img.shape[:2]
    magic = b"P5" if img.ndim == 2 else b"P6"
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n%d\n" % (magic, w, h, maxval) + img.astype(">u2").tobytes())


def test_cli_matches_the_binding(tmp_path):
    rng = np.random.default_rng(99)
    a = rng.integers(0, 65536, (60, 90, 3)).astype(np.uint16)
    b = np.clip(a.astype(np.int64) + rng.integers(-500, 501, a.shape), 0, 65535).astype(np.uint16)
    _write_png16(str(tmp_path / "a.png"), a)
    _write_png16(str(tmp_path / "b.png"), b)
    r = subprocess.run([CLI, "-d", str(tmp_path / "a.png"), str(tmp_path / "b.png")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = [ssim_amd.compute_ssim16(a[:, :, c], b[:, :, c], 16)[0] for c in range(3)]
    got = [float(line.split(":")[1]) for line in r.stdout.splitlines() if line.startswith("Channel")]
    assert np.allclose(got, want, atol=6e-5), (r.stdout, want)
    # 10-bit PGM: depth 10 from maxval 1023
    g1 = (a[:, :, 0] >> 6).astype(np.uint16)
    g2 = (b[:, :, 0] >> 6).astype(np.uint16)
    _write_pnm16(str(tmp_path / "a.pgm"), g1, 1023)
    _write_pnm16(str(tmp_path / "b.pgm"), g2, 1023)
    r = subprocess.run([CLI, "-d", str(tmp_path / "a.pgm"), str(tmp_path / "b.pgm")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [float(line.split(":")[1]) for line in r.stdout.splitlines() if line.startswith("Channel")]
    assert len(got) == 1 and abs(got[0] - float(ssim_amd.compute_ssim16(g1, g2, 10)[0])) <= 6e-5, r.stdout
