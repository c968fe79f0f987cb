"""CPU: SSIM of float32 volumes under a caller-chosen window, its gradient and the gradient of its map -- the definition and its
boundaries (include/rmgr/ssim-hip.h, rmgr_ssim_hip_*_ssim3f_win*).  Sizes are W x H x D; arrays are (D, H, W).

  * the entry points are exported, declared and listed; the Python keywords and the torch_ops signatures exist;
  * every EINVAL of a window comes before the device, and so does every EINVAL of the entry without _win;
  * the float64 model (tests/ssim3k_model.py) is ssim3f_model / ssim3w_model exactly under the engine's window, agrees for every window
    with an independent restatement -- torch float64, F.conv3d on replicate-padded input, autograd -- within 1e-9, its Gt is the adjoint
    of its G down to axes of length 1, and a volume of one slice gives the 2-D ssimk_model's result;
  * the fp32 emulation of the kernels leaves the figures ssim3k_model.EMU hold, pinned from both sides per window;
  * tests/ssim3k_plan.py restates the planner with 2R warm-up slices; a host program holds it to the C++;
  * ssim_amd.torch_ops refuses what it documents before any GPU call, and stays importable without torch;
  * ssim3k_kernels.hip never spills, holds seven kernels per radius and keeps the budgets of the 11-tap kernels.
"""
import ctypes
import errno
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ssim3f_model as S
import ssim3k_model as K3
import ssim3k_plan as PK
import ssim3w_model as W3
import ssimk_model as K2
import ssim_amd
from conftest import ROOT

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_ssim3f_win", "rmgr_ssim_hip_compute_ssim3f_win_device", "rmgr_ssim_hip_compute_ssim3f_win_host",
                "rmgr_ssim_hip_enqueue_ssim3f_win_grad", "rmgr_ssim_hip_enqueue_ssim3f_win_map_grad")
WINDOW_IDS = [K3.name_of(w) for w in K3.WINDOWS]
HIPCC = "/opt/rocm/bin/hipcc"


# ---- symbols ------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_declared_and_listed(lib):
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS, name
        assert re.search(r"rmgr_int32_t %s\(" % name, header), name
    assert lib.rmgr_ssim_hip_get_abi_version() == 6


def test_python_keywords_and_torch_signatures_exist():
    for fn in (ssim_amd.compute_ssim3f, ssim_amd.compute_ssim3f_batch, ssim_amd.Context.enqueue_ssim3f, ssim_amd.Context.ssim3f_device,
               ssim_amd.Context.enqueue_ssim3f_grad, ssim_amd.Context.enqueue_ssim3f_map_grad):
        p = inspect.signature(fn).parameters
        assert "window" in p and p["window"].default is None, fn
    from ssim_amd import torch_ops
    for fn in (torch_ops.ssim3d, torch_ops.ssim3d_map, torch_ops.ssim3d_amp, torch_ops.ssim3d_map_amp):
        names = list(inspect.signature(fn).parameters)
        assert names == ["x", "y", "data_range", "win_size", "win_sigma", "window"], (fn, names)
    names = list(inspect.signature(torch_ops.SSIM3DLoss.__init__).parameters)
    assert names == ["self", "data_range", "reduction", "win_size", "win_sigma", "window"], names
    for fn in (torch_ops.ssim3d, torch_ops.SSIM3DLoss.__init__):
        p = inspect.signature(fn).parameters
        assert (p["win_size"].default, p["win_sigma"].default, p["window"].default) == (11, 1.5, "gaussian")
    a = np.zeros((2, 3, 4), np.float32)
    with pytest.raises(TypeError):
        ssim_amd.compute_ssim3f(a, a, 1.0, window=(7, 1.5))
    with pytest.raises(TypeError):
        ssim_amd.compute_ssim3f_batch([(a, a)], 1.0, window="uniform")


# ---- the C ABI's validation (no device needed) -----------------------------------------------------------------------------------------

def _params(a, b, n=1, **over):
    ps = (ssim_amd.Params3F * n)()
    d, h, w = a.shape
    for i in range(n):
        ps[i] = ssim_amd.make_params3f(w, h, d, a.ctypes.data, (1, w, w * h), b.ctypes.data, (1, w, w * h))
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _grads(a, n=1):
    gs = (ssim_amd.Grad3F * n)()
    for i in range(n):
        gs[i] = ssim_amd.Grad3F(a.ctypes.data, 1, a.shape[2], a.shape[2] * a.shape[1])
    return gs


def _gmaps(a, n=1):
    gs = (ssim_amd.GradOut3F * n)()
    for i in range(n):
        gs[i] = ssim_amd.GradOut3F(a.ctypes.data, 1, a.shape[2], a.shape[2] * a.shape[1])
    return gs


BAD_WINDOWS = [(1, 0, 1.5), (4, 0, 1.5), (13, 0, 1.5), (0, 1, 0.0), (2, 1, 0.0), (12, 1, 0.0), (7, 2, 1.5), (7, 0xFFFFFFFF, 1.5),
               (7, 0, 0.0), (7, 0, -1.0), (7, 0, float("nan")), (7, 0, float("inf")), (11, 0, float("-inf"))]
GOOD_WINDOWS = [None, (11, 0, 1.5), (3, 1, 0.0), (3, 1, float("nan")), (9, 0, 0.5), (7, 1, -3.0)]      # a box does not read sigma


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    """The fake context and the fake device pointers are never dereferenced: an EINVAL that came after the first use of the context
    would crash.  A valid window with a NULL context is EINVAL too (the entries that need one), which shows the window passed."""
    a = np.zeros((6, 20, 30), np.float32)
    b = np.zeros((6, 20, 30), np.float32)
    ga = np.zeros((6, 20, 30), np.float32)
    grad, mapg, host = fn.endswith("_grad"), fn.endswith("_map_grad"), fn.endswith("_host")
    out = _gmaps(ga, 2) if mapg else ((ctypes.c_float * 4)() if not fn.startswith("rmgr_ssim_hip_enqueue") else ctypes.c_void_p(16))
    fake_ctx = None if host else ctypes.c_void_p(1)
    E = errno.EINVAL
    f = getattr(lib, fn)

    def win(w):
        return None if w is None else ctypes.byref(ssim_amd.Window(*w))

    def rc(count=1, params=None, r=1.0, o=out, ctx=fake_ctx, grads=None, w=(7, 1, 0.0)):
        ps = _params(a, b, max(count, 1)) if params is None else params
        if grad:
            ga_, gb_ = (_grads(ga, max(count, 1)), None) if grads is None else grads
            return f(ctx, count, ps, r, win(w), o, ga_, gb_)
        return f(ctx, count, ps, r, win(w), o)
    # the window
    for w in BAD_WINDOWS:
        assert rc(w=w) == E, w
        assert rc(w=w, count=2) == E, w
    if not host:
        for w in GOOD_WINDOWS:
            assert rc(w=w, ctx=None) == E, w                                   # valid so far: the NULL context is what is refused
    # every EINVAL of the entry without _win, under a valid window and under NULL
    for w in ((7, 1, 0.0), None):
        assert rc(count=0, w=w) == E
        assert (f(fake_ctx, 1, None, 1.0, win(w), out, _grads(ga), None) if grad else f(fake_ctx, 1, None, 1.0, win(w), out)) == E
        assert rc(o=None, w=w) == E
        for dim in ("width", "height", "depth"):
            assert rc(params=_params(a, b, **{dim: 0}), w=w) == E
            assert rc(params=_params(a, b, **{dim: 0x7FFF0001}), w=w) == E
            two = _params(a, b, 2)
            setattr(two[1], dim, getattr(two[1], dim) - 1)
            assert rc(count=2, params=two, w=w) == E
        bad = _params(a, b)
        bad[0].imgA.topLeft = None
        assert rc(params=bad, w=w) == E
        bad = _params(a, b, 2)
        bad[1].imgB.topLeft = None
        assert rc(count=2, params=bad, w=w) == E
        for off in (1, 2, 3):
            bad = _params(a, b)
            bad[0].imgA.topLeft = a.ctypes.data + off
            assert rc(params=bad, w=w) == E
            bad = _params(a, b, 2)
            bad[1].imgB.topLeft = b.ctypes.data + off
            assert rc(count=2, params=bad, w=w) == E
            if not grad:
                bad = _params(a, b)
                bad[0].ssimMap = ga.ctypes.data + off
                assert rc(params=bad, w=w) == E
        for r in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
            assert rc(r=r, w=w) == E
        if grad:
            assert rc(grads=(None, None), w=w) == E
            g = _grads(ga, 2)
            g[1].topLeft = None
            assert rc(count=2, grads=(g, None), w=w) == E and rc(count=2, grads=(None, g), w=w) == E
            g = _grads(ga)
            g[0].topLeft = ga.ctypes.data + 2
            assert rc(grads=(g, None), w=w) == E and rc(grads=(_grads(ga), g), w=w) == E
        if mapg:
            m = _gmaps(ga, 2)
            m[1].topLeft = None
            assert rc(count=2, o=m, w=w) == E
            m = _gmaps(ga)
            m[0].topLeft = ga.ctypes.data + 2
            assert rc(o=m, w=w) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    win = ssim_amd.make_window(3, kind="uniform")
    if ssim_amd.device_count() > 0:
        v, _ = ssim_amd.compute_ssim3f(np.full((4, 8, 8), 0.25, np.float32), np.full((4, 8, 8), 0.25, np.float32), 1.0, window=win)
        assert abs(float(v) - 1.0) < 1e-6
        return
    a = np.zeros((6, 20, 30), np.float32)
    out = (ctypes.c_float * 1)()
    assert lib.rmgr_ssim_hip_compute_ssim3f_win_host(None, 1, _params(a, a), 1.0, ctypes.byref(win), out) == errno.ENODEV
    assert lib.rmgr_ssim_hip_compute_ssim3f_win_host(None, 1, _params(a, a), 1.0, None, out) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssim3f(a, a, 1.0, window=win)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssim3f_batch([(a, a), (a, a)], 1.0, window=win)


# ---- the model ---------------------------------------------------------------------------------------------------------------------

def _pair(size, seed):
    w, h, d = size
    rng = np.random.default_rng(seed)
    a = rng.random((d, h, w)).astype(np.float32)
    b = np.clip(a + 0.1 * rng.standard_normal((d, h, w)), 0, 1).astype(np.float32)
    return a, b


def test_the_engine_window_is_the_fixed_window_models_exactly():
    for size in ((13, 12, 11), (5, 3, 4), (1, 1, 1), (20, 17, 9)):
        a, b = _pair(size, sum(size))
        for r, sa, sb in ((1.0, a, b), (255.0, a * np.float32(255), b * np.float32(255))):
            v, m = K3.ssim(sa, sb, r)
            v0, m0 = S.ssim(sa, sb, r)
            assert v == v0 and np.array_equal(m, m0)
            assert all(np.array_equal(x, y) for x, y in zip(K3.grad(sa, sb, r, -0.75), S.grad(sa, sb, r, -0.75)))
            kv = np.random.default_rng(5).standard_normal(sa.shape).astype(np.float32)
            assert all(np.array_equal(x, y) for x, y in zip(K3.grad_map(sa, sb, r, kv), W3.grad_map(sa, sb, r, kv)))
            e, e0 = K3.emulate_fp32(sa, sb, r, g_out=-0.75), S.emulate_fp32(sa, sb, r, g_out=-0.75)
            assert e[0] == e0[0] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(e[1:], e0[1:]))
            e, e0 = K3.emulate_fp32(sa, sb, r, gmap=kv)[2:], W3.emulate_fp32_map_grad(sa, sb, r, kv)
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(e, e0))
    assert np.array_equal(K3.taps(), S.gaussian_taps().astype(np.float32)[5:])


def _torch_restatement(a, b, data_range, window, g_out=None, gmap=None):
    """(value, map, dA, dB) by torch float64: 1-D conv3d per axis on replicate-padded volumes, the five statistics, autograd; the
    upstream gradient is g_out on the mean or gmap on the map."""
    import torch
    import torch.nn.functional as Fn
    g = torch.tensor(K3.full_taps(window), dtype=torch.float64)
    R, n = K3.radius(window), 2 * K3.radius(window) + 1
    c1, c2 = K3.constants(data_range)

    def blur(v):
        v = v[None, None]
        v = Fn.conv3d(Fn.pad(v, (R, R, 0, 0, 0, 0), mode="replicate"), g.reshape(1, 1, 1, 1, n))
        v = Fn.conv3d(Fn.pad(v, (0, 0, R, R, 0, 0), mode="replicate"), g.reshape(1, 1, 1, n, 1))
        v = Fn.conv3d(Fn.pad(v, (0, 0, 0, 0, R, R), mode="replicate"), g.reshape(1, 1, n, 1, 1))
        return v[0, 0]
    ta = torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    tb = torch.tensor(np.asarray(b, np.float64), requires_grad=True)
    ma, mb = blur(ta), blur(tb)
    s_aa, s_bb, s_ab = blur(ta * ta) - ma * ma, blur(tb * tb) - mb * mb, blur(ta * tb) - ma * mb
    m = (2 * ma * mb + c1) * (2 * s_ab + c2) / ((ma * ma + mb * mb + c1) * (s_aa + s_bb + c2))
    value = m.sum() / K3.voxels(a.shape)
    if gmap is None:
        (g_out * value).backward()
    else:
        (m * torch.tensor(np.asarray(gmap, np.float64))).sum().backward()
    return float(value.detach()), m.detach().numpy(), ta.grad.numpy(), tb.grad.numpy()


@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_model_is_the_conv3d_restatement(window):
    for size in ((1, 1, 1), (1, 1, 2), (2, 1, 1), (5, 3, 4), (13, 12, 11)):
        a, b = _pair(size, sum(size) * 7 + window[0])
        for r, sa, sb in ((1.0, a, b), (255.0, a * np.float32(255), b * np.float32(255))):
            value, m = K3.ssim(sa, sb, r, window)
            da, db = K3.grad(sa, sb, r, -0.75, window)
            tv, tm, tda, tdb = _torch_restatement(sa, sb, r, window, g_out=-0.75)
            assert abs(value - tv) <= 1e-9 and np.abs(m - tm).max() <= 1e-9, (size, r, value, tv)
            assert np.abs(da - tda).max() <= 1e-9 and np.abs(db - tdb).max() <= 1e-9, (size, r)
            assert np.abs(tda).max() > 1e-6 / r                      # a gradient worth comparing
            kv = np.random.default_rng(9).standard_normal(sa.shape).astype(np.float32)
            da, db = K3.grad_map(sa, sb, r, kv, window)
            _, _, tda, tdb = _torch_restatement(sa, sb, r, window, gmap=kv)
            assert np.abs(da - tda).max() <= 1e-9 and np.abs(db - tdb).max() <= 1e-9, (size, r)


@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_gt_is_the_adjoint_of_g(window):
    rng = np.random.default_rng(11)
    for shape in [(12, 14, 16), (1, 1, 1), (1, 7, 3), (3, 1, 20), (6, 6, 6), (2, 5, 1), (2, 2, 2), (1, 1, 4)]:
        u, v = rng.standard_normal(shape), rng.standard_normal(shape)
        lhs, rhs = float(np.sum(K3.blur(u, window) * v)), float(np.sum(u * K3.blur_t(v, window)))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-3), (shape, lhs, rhs)


@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_a_volume_of_one_slice_is_the_2d_model(window):
    """D == 1: the z pass multiplies by the sum of the 2R + 1 float taps, which is 1 to a few 1e-8."""
    rng = np.random.default_rng(3)
    a, b = rng.random((9, 11)), rng.random((9, 11))
    v3, m3 = K3.ssim(a[None], b[None], 1.0, window)
    v2, m2 = K2.ssim(a, b, 1.0, window)
    assert abs(v3 - v2) < 1e-6 and np.abs(m3[0] - m2).max() < 1e-6
    g3, g2 = K3.grad(a[None], b[None], 1.0, 1.0, window), K2.grad(a, b, 1.0, 1.0, window)
    for x, y in zip(g3, g2):
        assert np.abs(x[0] - y).max() <= 1e-6 * np.abs(y).max()


# ---- the pinned figures ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_fp32_emulation_leaves_the_pinned_figures(manifest, window):
    """emulate_fp32 against the float64 model on the golden volumes of ssim3f_model (FIXTURES x FORMS; every fixture's A against itself
    for the identical pair; the three weight volumes of ssim3w_model for the map gradient).  The measured value is at most the recorded
    figure, and the recorded figure at most 1.25 times the measured value.  tests/test_gpu_ssim3k.py asserts twice ssim3k_model.EMU."""
    got = K3.measure(manifest, window)
    print("%s: px %.3g global %.3g grad %.3g identical %.3g map grad %.3g" % ((K3.name_of(window),) + got))
    for v, emu, tol in zip(got, K3.EMU[window], K3.tolerances(window)):
        assert v <= emu, (got, K3.EMU[window])
        assert emu <= 1.25 * v, (got, K3.EMU[window])
        assert tol == 2.0 * emu


# ---- the planner ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/src/plan3k_probe.cpp linked against the kernel object of the library under test (plan3f lives in ssim3f_kernels.o)."""
    obj3f = "build/obj/ssim3f_kernels.o"
    r = subprocess.run(["make", "-C", ROOT, obj3f], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path_factory.mktemp("plan3k_probe")
    obj, exe = str(out / "plan3k_probe.o"), str(out / "plan3k_probe")
    src = os.path.join(ROOT, "tests", "src", "plan3k_probe.cpp")
    for cmd in ([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                 "-I" + os.path.join(ROOT, "ssim_amd", "csrc"), "-c", src, "-o", obj],
                [HIPCC, "--offload-arch=gfx950", obj, os.path.join(ROOT, obj3f), "-o", exe]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]

    def run(rows):
        text = "".join("%d %d %d %d %d %d\n" % row for row in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        assert len(got) == len(rows) and all(len(g) == 6 for g in got)
        return [(PK.Geometry(*g[:5]), g[5]) for g in got]
    return run


def test_the_planner_restatement_agrees_with_the_cpp(probe):
    import ssim3f_plan as P3
    rng = np.random.default_rng(2024)
    rows = []
    for radius in (1, 2, 3, 4, 5):
        for _ in range(80):
            w, h, d = int(rng.integers(1, 300)), int(rng.integers(1, 300)), int(rng.integers(1, 1300))
            rows.append((radius, w, h, d, int(np.exp(rng.uniform(0, np.log(70000.0)))), int(rng.choice([32, 64, 256, 304, 0]))))
        for p in (8, 16, 64, 256):
            for d in (p - 1, p, p + 1):
                rows.append((radius, int(rng.integers(1, 70)), int(rng.integers(1, 70)), d, int(rng.integers(1, 2000)), 256))
        rows += [(radius, 17, 17, 131, n, 256) for n in (1, 5, 16, 31, 61, 154)]
    got = probe(rows)
    differs = 0
    for row, (geo, most) in zip(rows, got):
        radius, w, h, d, n, cus = row
        mine = PK.plan3k(radius, w, h, d, n, cus)
        assert geo == mine, (row, geo, mine)
        assert most == PK.max_count(w, h, d), row
        k = geo.chunk_slices // 8
        assert geo.chunk_slices == 8 * k and k >= 1 and k & (k - 1) == 0 and geo.chunks * geo.chunk_slices >= d > (geo.chunks - 1) * geo.chunk_slices, (row, geo)
        if radius == 5:
            assert mine == P3.plan3f(w, h, d, n, cus), row                     # 10 warm-up slices: the fixed window's planner
        else:
            differs += mine != P3.plan3f(w, h, d, n, cus)
    assert differs > 0                                                         # the warm-up is read
    print("\n%d launches agree; %d of the smaller windows' plans differ from the 11-tap plan" % (len(rows), differs))


# ---- torch_ops (CPU tensors) -----------------------------------------------------------------------------------------------------------

def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 1, 8, 16, 16)
    for fn in (torch_ops.ssim3d, torch_ops.ssim3d_map, torch_ops.ssim3d_amp, torch_ops.ssim3d_map_amp,
               lambda x, y, **kw: torch_ops.SSIM3DLoss(**kw)(x, y)):
        for kw in (dict(win_size=7.0), dict(win_size="7"), dict(win_size=True), dict(window=1), dict(window=None)):
            with pytest.raises(TypeError):
                fn(x, x, **kw)
        for kw in (dict(win_size=4), dict(win_size=13), dict(win_size=1), dict(win_size=-3), dict(win_sigma=0.0), dict(win_sigma=-1.0),
                   dict(win_sigma=float("nan")), dict(win_sigma=float("inf")), dict(window="box"), dict(window="Gaussian")):
            with pytest.raises(ValueError):
                fn(x, x, **kw)
        # valid windows reach the device check: CPU tensors
        for kw in (dict(win_size=7), dict(win_size=3, window="uniform"), dict(window="uniform", win_sigma=float("nan")), dict()):
            with pytest.raises(ValueError, match="GPU"):
                fn(x, x, **kw)
    with pytest.raises(ValueError):
        torch_ops.SSIM3DLoss(win_size=6)                                       # checked at construction
    with pytest.raises(TypeError):
        torch_ops.SSIM3DLoss(window=7)
    loss = torch_ops.SSIM3DLoss(255.0, "none", 7, 2.0, "uniform")
    assert (loss.data_range, loss.reduction, loss.win_size, loss.win_sigma, loss.window) == (255.0, "none", 7, 2.0, "uniform")


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd.torch_ops; "
                        "ssim_amd.torch_ops.SSIM3DLoss(win_size=7); assert 'torch' not in sys.modules" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the kernels' budgets ----------------------------------------------------------------------------------------------------------------

def test_window_volume_kernels_never_spill_and_keep_the_budgets_of_the_11_tap_kernels():
    """Build-time guard, compiled as tests/test_ssim3f_cpu.py compiles ssim3f_kernels.hip: no scratch, exactly 7 kernels per radius (4
    walks: value, dA, dB, both; 3 adjoint walks), 28 in all; for every radius the walks use at most 112 VGPRs at 4 waves per SIMD or
    more, the adjoint walks at most 168 VGPRs at 3 waves per SIMD or more, and LDS is at most 16 (16 + 2R)^2 + 256 (16 + 2R) + 32
    bytes: the budgets of the 11-tap kernels at their own radius."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "ssim3k_kernels.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src), "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key in ("VGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]", "LDS Size \\[bytes/block\\]"):
            m = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if m and name:
                kernels[name][key.split(" ")[0]] = int(m.group(1))
    assert len(kernels) == 28, sorted(kernels)
    for radius in (1, 2, 3, 4):
        walk = {k: v for k, v in kernels.items() if "ssim3k_walk_kernelILi%dE" % radius in k}
        adjoint = {k: v for k, v in kernels.items() if "ssim3k_adjoint_kernelILi%dE" % radius in k}
        assert len(walk) == 4 and len(adjoint) == 3, (radius, sorted(kernels))
        lds = 16 * (16 + 2 * radius) ** 2 + 256 * (16 + 2 * radius) + 32
        for k, v in walk.items():
            assert v["ScratchSize"] == 0 and v["VGPRs"] <= 112 and v["Occupancy"] >= 4 and v["LDS"] <= lds, (k, v)
        for k, v in adjoint.items():
            assert v["ScratchSize"] == 0 and v["VGPRs"] <= 168 and v["Occupancy"] >= 3 and v["LDS"] <= lds, (k, v)
