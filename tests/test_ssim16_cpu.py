"""CPU: SSIM of 9- to 16-bit samples -- its definition and its boundaries (include/rmgr/ssim-hip.h, rmgr_ssim_hip_*_ssim16).

  * the float64 model (tests/ssim16_model.py) at depth 8 with the double constants IS the reference's fp64 oracle;
  * at depth 16 the model of 257 a, 257 b is the depth-8 model of a, b (L = 257 * 255 and C1, C2 scale with L^2);
  * the fp32 emulation of the kernel stays inside the bounds tests/test_gpu_ssim16.py asserts;
  * the entry points are exported, every EINVAL comes before the device, a valid call without a device is ENODEV;
  * `rmgr-ssim --decode16` reads 16-bit PNG and 10- / 16-bit PNM samples as written; `-d` is refused with -y, -m and differing depths.
"""
import ctypes
import errno
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import ssim16_model as M
import ssim_amd
from conftest import ROOT, image_entries, load_pair

CLI = os.environ.get("RMGR_SSIM_CLI") or os.path.join(ROOT, "ssim_amd", "bin", "rmgr-ssim")
ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_ssim16", "rmgr_ssim_hip_compute_ssim16_device", "rmgr_ssim_hip_compute_ssim16_host")


def test_model_at_depth_8_is_the_reference_double_oracle(oracle, manifest):
    c1, c2 = M.constants(8, f32=False)
    g = M.gaussian_taps()
    # the oracle's window is the float64 Gaussian; the model's taps are the engine's fp32 ones unless told otherwise
    i = np.arange(-5, 6, dtype=np.float64)
    g64 = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    g64 /= g64.sum()
    assert np.abs(g - g64).max() < 1e-8
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        want, _, _ = oracle.ssim_naive_f64(a, b)
        got, _ = M.ssim(a, b, 8, c1, c2, g64)
        assert abs(got - want) <= 1e-12, (n, got, want)


def test_constants():
    assert M.constants(8) == (float(np.float32(6.5025)), float(np.float32(58.5225)))
    for d in range(8, 17):
        L = (1 << d) - 1
        c1, c2 = M.constants(d, f32=False)
        assert c1 == (0.01 * L) * (0.01 * L) and c2 == (0.03 * L) * (0.03 * L)


def test_depth_16_of_257x_is_depth_8(manifest):
    for n in image_entries(manifest)[:6]:
        a, b = load_pair(manifest[n])
        v8, m8 = M.ssim(a, b, 8, *M.constants(8, f32=False))
        v16, m16 = M.ssim(a.astype(np.int64) * 257, b.astype(np.int64) * 257, 16, *M.constants(16, f32=False))
        assert abs(v16 - v8) <= 1e-12 and np.abs(m16 - m8).max() <= 1e-12, n


def test_fp32_emulation_is_inside_the_gpu_bounds(manifest):
    """The bounds of tests/test_gpu_ssim16.py (PX_TOL 5e-4, G_TOL 1.3e-6) are twice what this emulation measures (2.3e-4 / 6.3e-7)."""
    worst_px = worst_g = 0.0
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        for depth, s in ((16, 257), (8, 1)):
            A, B = a.astype(np.int64) * s, b.astype(np.int64) * s
            gv, gm = M.ssim(A, B, depth)
            ev, em = M.emulate_fp32(A, B, depth)
            worst_px = max(worst_px, float(np.abs(em - gm).max()))
            worst_g = max(worst_g, abs(ev - gv))
    assert worst_px <= 2.5e-4 and worst_g <= 6.5e-7, (worst_px, worst_g)


def test_centres_are_per_strip_column():
    img = np.arange(7 * 300).reshape(7, 300)
    assert list(M.centres(img)) == [img[3, 64], img[3, 192], img[3, 299]]


# ---- the C ABI's validation (no device needed) ----

def _params(a, b, n=1, **over):
    ps = (ssim_amd.Params16 * n)()
    h, w = a.shape
    for i in range(n):
        ps[i] = ssim_amd.make_params16(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w)
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def test_entry_points_are_exported(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    a = np.zeros((20, 30), np.uint16)
    b = np.zeros((20, 30), np.uint16)
    out = (ctypes.c_float * 4)() if not fn.startswith("rmgr_ssim_hip_enqueue") else ctypes.c_void_p(16)   # never dereferenced
    fake_ctx = None if fn.endswith("_host") else ctypes.c_void_p(1)                                     # never dereferenced
    E = errno.EINVAL
    f = getattr(lib, fn)

    def rc(count=1, params=None, depth=10, o=out, ctx=fake_ctx):
        return f(ctx, count, _params(a, b, max(count, 1)) if params is None else params, depth, o)
    assert rc(count=0) == E
    assert f(fake_ctx, 1, None, 10, out) == E                                  # params NULL
    assert rc(o=None) == E                                                     # ssim / sumsDevice NULL
    assert rc(params=_params(a, b, width=0)) == E
    assert rc(params=_params(a, b, height=0)) == E
    two = _params(a, b, 2)
    two[1].width = 29
    assert rc(count=2, params=two) == E                                        # sizes differ
    two = _params(a, b, 2)
    two[1].height = 19
    assert rc(count=2, params=two) == E
    bad = _params(a, b)
    bad[0].imgA.topLeft = None
    assert rc(params=bad) == E
    bad = _params(a, b, 2)
    bad[1].imgB.topLeft = None
    assert rc(count=2, params=bad) == E
    bad = _params(a, b)
    bad[0].imgA.topLeft = a.ctypes.data + 1                                    # not 2-byte aligned
    assert rc(params=bad) == E
    bad = _params(a, b, 2)
    bad[1].imgB.topLeft = b.ctypes.data + 3
    assert rc(count=2, params=bad) == E
    for d in (0, 1, 7, 17, 32):
        assert rc(depth=d) == E
    if not fn.endswith("_host"):
        assert rc(ctx=None) == E                                               # these entries need a context
        assert rc(ctx=None, depth=16) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    if ssim_amd.device_count() > 0:
        v, _ = ssim_amd.compute_ssim16(np.full((8, 8), 700, np.uint16), np.full((8, 8), 700, np.uint16), 10)
        assert abs(float(v) - 1.0) < 1e-6
        return
    a = np.zeros((20, 30), np.uint16)
    out = (ctypes.c_float * 1)()
    for d in (8, 10, 16):
        assert lib.rmgr_ssim_hip_compute_ssim16_host(None, 1, _params(a, a), d, out) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssim16(a, a, 12)


# ---- the command-line tool ----

def write_png16(path, img):
    """A 16-bit grey / grey-alpha / RGB / RGBA PNG written with zlib (PIL cannot write the 48- and 64-bit ones)."""
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    raw = b"".join(b"\0" + img[y].astype(">u2").tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, {1: 0, 2: 4, 3: 2, 4: 6}[ch], 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def write_pnm16(path, img, maxval, ascii_=False):
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else 3
    magic = {(1, False): b"P5", (3, False): b"P6", (1, True): b"P2", (3, True): b"P3"}[(ch, ascii_)]
    body = (" ".join(str(int(v)) for v in img.reshape(-1)).encode() + b"\n") if ascii_ else img.astype(">u2").tobytes()
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n%d\n" % (magic, w, h, maxval) + body)


def decode16(tmp_path, path):
    out = str(tmp_path / "dump.raw")
    r = subprocess.run([CLI, "--decode16", path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    w, h, c, d = (int(t) for t in r.stdout.split())
    px = np.fromfile(out, "<u2")
    assert px.size == w * h * c
    return px.reshape(h, w, c), d


@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_decode16_png(tmp_path, ch):
    rng = np.random.default_rng(ch)
    img = rng.integers(0, 65536, (13, 21) if ch == 1 else (13, 21, ch)).astype(np.uint16)
    p = str(tmp_path / "x.png")
    write_png16(p, img)
    px, d = decode16(tmp_path, p)
    assert d == 16 and np.array_equal(px.reshape(img.shape), img)


def test_decode16_png_written_by_pil(tmp_path):
    from PIL import Image
    img = np.random.default_rng(4).integers(0, 65536, (17, 23)).astype(np.uint16)
    p = str(tmp_path / "pil.png")
    Image.fromarray(img).save(p)            # mode I;16: a 16-bit grey PNG
    px, d = decode16(tmp_path, p)
    assert d == 16 and np.array_equal(px[:, :, 0], img)


@pytest.mark.parametrize("maxval,depth", [(1023, 10), (4095, 12), (65535, 16), (1000, 10), (256, 9)])
@pytest.mark.parametrize("ch", [1, 3])
def test_decode16_pnm(tmp_path, maxval, depth, ch):
    rng = np.random.default_rng(maxval + ch)
    img = rng.integers(0, maxval + 1, (9, 14) if ch == 1 else (9, 14, 3)).astype(np.uint16)
    for ascii_ in (False, True):
        p = str(tmp_path / ("x%d.pnm" % ascii_))
        write_pnm16(p, img, maxval, ascii_)
        px, d = decode16(tmp_path, p)
        assert d == depth and np.array_equal(px.reshape(img.shape), img), ascii_


def test_decode16_of_8_bit_files_is_depth_8(tmp_path):
    img = np.random.default_rng(2).integers(0, 256, (11, 9, 3)).astype(np.uint8)
    p = str(tmp_path / "x.ppm")
    with open(p, "wb") as f:
        f.write(b"P6\n9 11\n255\n" + img.tobytes())
    px, d = decode16(tmp_path, p)
    assert d == 8 and np.array_equal(px, img.astype(np.uint16))


def test_without_d_nothing_changes(tmp_path):
    img = np.random.default_rng(6).integers(0, 65536, (5, 7)).astype(np.uint16)
    p = str(tmp_path / "x.png")
    write_png16(p, img)
    out = str(tmp_path / "x.raw")
    r = subprocess.run([CLI, "--decode", p, out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["7", "5", "1"]
    assert np.array_equal(np.fromfile(out, np.uint8).reshape(5, 7), (img >> 8).astype(np.uint8))      # most significant byte
    q = str(tmp_path / "x.pgm")
    write_pnm16(q, img, 65535)
    r = subprocess.run([CLI, "--decode", q, out], capture_output=True, text=True)
    assert r.returncode != 0 and "only maxval <= 255" in r.stderr


@pytest.mark.parametrize("args", [["-d", "-y"], ["-y", "-d"], ["-d", "-m"], ["-m", "-d"]])
def test_d_is_refused_with_y_and_m(tmp_path, args):
    r = subprocess.run([CLI] + args + [str(tmp_path / "missing_a.png"), str(tmp_path / "missing_b.png")], capture_output=True, text=True)
    assert r.returncode == 1
    assert "-d" in r.stderr and "Failed to open" not in r.stderr                  # refused while parsing


def test_d_is_refused_when_depths_differ(tmp_path):
    a = np.random.default_rng(1).integers(0, 1024, (8, 8)).astype(np.uint16)
    write_pnm16(str(tmp_path / "a.pgm"), a, 1023)
    write_pnm16(str(tmp_path / "b.pgm"), a, 4095)
    r = subprocess.run([CLI, "-d", str(tmp_path / "a.pgm"), str(tmp_path / "b.pgm")], capture_output=True, text=True)
    assert r.returncode == 1 and "depth" in r.stderr and "device" not in r.stderr


def test_cli_help_names_d():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("Usage: rmgr-ssim [options] img1 img2 [map]")
    assert "  -d  " in r.stdout
