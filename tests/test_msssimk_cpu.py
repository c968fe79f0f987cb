"""CPU: multi-scale SSIM under a caller-chosen window -- the definition and its boundaries (include/rmgr/ssim-hip.h,
rmgr_ssim_hip_*_msssimf_win* and rmgr_ssim_hip_*_msssimh_win*).

  * tests/msssimk_model.py at the default window IS tests/msssimf_model.py: the float64 model returns its values exactly, the fp32
    emulation reproduces its emulation bit for bit (value, means, gradients); with one scale of weight 1 the model IS ssimk_model's;
  * the model's gradient is the derivative of the model's value under small and box windows, on planes smaller than the window at
    coarse scales;
  * per window the fp32 emulation leaves the figures of msssimk_model.EMU against the float64 model, pinned from both sides, and no
    case sits near the ReLU;
  * the eight entry points are exported, every EINVAL -- a bad window included -- comes before the device, a valid call without a device
    is ENODEV, the binding refuses a window that is no Window, ssim_amd.torch_ops refuses what it documents before any GPU call, and the
    new kernel files keep their budgets.
"""
import ctypes
import errno
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import msssimf_model as MF
import msssimk_model as MK
import ssimk_model as SK
import ssim_amd
from conftest import ROOT, load_pair

ENTRY_POINTS_F = ("rmgr_ssim_hip_enqueue_msssimf_win", "rmgr_ssim_hip_compute_msssimf_win_device", "rmgr_ssim_hip_compute_msssimf_win_host",
                  "rmgr_ssim_hip_enqueue_msssimf_win_grad")
ENTRY_POINTS_H = tuple(n.replace("msssimf", "msssimh") for n in ENTRY_POINTS_F)
ENTRY_POINTS = ENTRY_POINTS_F + ENTRY_POINTS_H


# ---- the model ----

def test_default_window_is_msssimf_model_exactly_and_its_emulation_bit_for_bit(manifest):
    assert np.array_equal(MK.padded_taps(MK.DEFAULT), MF.gaussian_taps())
    for n in ("bbb257x65_q50_ch1", "einstein_blur"):
        a, b = load_pair(manifest[n])
        for _, fa, fb, r in SK.fixture_forms(manifest, n):
            if n == "einstein_blur":
                fa, fb = fa[40:139, 10:311], fb[40:139, 10:311]            # three strip columns, odd sizes
            mod, ref = MK.model(fa, fb, r), MF.Model(fa, fb, r)
            emu, eref = MK.Emulation(fa, fb, r), MF.Emulation(fa, fb, r)
            for scales, w in MK.CONFIGS:
                (v, m), (rv, rm) = mod.msssim(scales, w), ref.msssim(scales, w)
                assert v == rv and np.array_equal(m, rm)
                for g, rg in zip(mod.grad(-0.75, scales, w), ref.grad(-0.75, scales, w)):
                    assert np.array_equal(g, rg)
                (v, m), (rv, rm) = emu.msssim(scales, w), eref.msssim(scales, w)
                assert v == rv and np.array_equal(m, rm)
                for g, rg in zip(emu.grad(-0.75, scales, w), eref.grad(-0.75, scales, w)):
                    assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), rg.view(np.uint32))


@pytest.mark.parametrize("window", SK.WINDOWS, ids=SK.name_of)
def test_one_scale_of_weight_one_is_the_ssimk_model(manifest, window):
    a, b = load_pair(manifest["bbb257x65_q50_ch1"])
    a, b = a[:40, 100:170] / 255.0, b[:40, 100:170] / 255.0
    mod = MK.model(a, b, 1.0, window)
    v, means = mod.msssim(1, (1.0,))
    want, _ = SK.ssim(a, b, 1.0, window)
    assert abs(v - want) <= 1e-12 * abs(want) and abs(means[0][1] - want) <= 1e-12 * abs(want)
    for g, wg in zip(mod.grad(-0.75, 1, (1.0,)), SK.grad(a, b, 1.0, -0.75, window)):
        assert np.abs(g - wg).max() <= 1e-12 * np.abs(wg).max()
    # the emulation of one scale is ssimk_model's emulation of that window, bit for bit
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    emu = MK.Emulation(fa, fb, 1.0, window)
    # k: ssimk rounds float(gOut / (W H)), the multi-scale form float(gOut w MS / m / (W H)) -- not the same number to the bit, so
    # ssimk's emulation is handed the multi-scale k as a constant plane (the product k d is the same operation in both forms)
    k = np.float32(MF.coefficients(emu.means(1), (1.0,), -0.75, [(fa.shape[1], fa.shape[0])])[0])
    ev, _, ea, eb = SK.emulate_fp32(fa, fb, 1.0, window, gmap=np.full(fa.shape, k, np.float32))
    assert emu.msssim(1, (1.0,))[0] == ev
    for g, wg in zip(emu.grad(-0.75, 1, (1.0,)), (ea, eb)):
        assert np.array_equal(g.view(np.uint32), wg.view(np.uint32))


def test_gradient_is_the_derivative_of_the_value_under_small_windows(manifest):
    """Central differences of the model's own MS at steps 1e-5 and 5e-6 (range 1) against grad(), as tests/test_msssimf_cpu.py has them
    and with its bound, under windows whose planes become smaller than the window at coarse scales: 33 x 17 at 4 scales ends at 5 x 3
    under 7- and 9-tap windows, 5 x 3 and 1 x 1 start there."""
    rng = np.random.default_rng(11)
    a, b = load_pair(manifest["einstein_blur"])
    cases = (((3, 0.0, "uniform"), (0, 0, 17, 33), (0.25,) * 4), ((9, 1.5, "gaussian"), (30, 40, 17, 33), (0.25,) * 4),
             ((7, 0.0, "uniform"), (100, 60, 3, 5), (0.5, 0.3, 0.2)), ((5, 0.8, "gaussian"), (50, 50, 1, 1), (0.5, 0.5)),
             ((11, 0.0, "uniform"), (7, 9, 20, 4), (0.3, 0.0, 0.7)))
    for window, (y0, x0, h, w), wts in cases:
        ca, cb = a[y0:y0 + h, x0:x0 + w] / 255.0, b[y0:y0 + h, x0:x0 + w] / 255.0
        g_out, scales = -0.75, len(wts)
        grads = MK.model(ca, cb, 1.0, window).grad(g_out, scales, wts)
        pts = {(0, 0), (h - 1, w - 1), (0, w - 1), (h // 2, w // 2)}
        while len(pts) < min(8, h * w):
            pts.add((int(rng.integers(0, h)), int(rng.integers(0, w))))
        for which, gr in enumerate(grads):
            scale = np.abs(gr).max()
            for eps in (1e-5, 5e-6):
                for (y, x) in sorted(pts):
                    p, m = [ca.copy(), cb.copy()], [ca.copy(), cb.copy()]
                    p[which][y, x] += eps
                    m[which][y, x] -= eps
                    fd = g_out * (MK.model(p[0], p[1], 1.0, window).msssim(scales, wts)[0] -
                                  MK.model(m[0], m[1], 1.0, window).msssim(scales, wts)[0]) / (2 * eps)
                    assert abs(fd - gr[y, x]) <= 1e-6 * scale, (window, (h, w), which, y, x, eps, fd, gr[y, x])


@pytest.mark.parametrize("window", SK.WINDOWS, ids=SK.name_of)
def test_fp32_emulation_leaves_the_figures_of_emu(manifest, window):
    """Emulation against the float64 model on ssimk_model.FIXTURES x FORMS at Wang's 5 scales and at uniform weights for 1, 3 and 8
    scales: value, every per-scale mean, both gradients, and the pair of identical images.  tests/test_gpu_msssimk.py asserts
    ssimk_model.TOL_FACTOR x these figures.  Conditioning: every mean that enters the product at 5 and 8 scales is at least
    msssimk_model.MIN_MEAN, so no case sits near the ReLU or divides by a small m_s."""
    v, m, g, ident, lowest = MK.measure(manifest, window)
    print("%s: value %.4g mean %.4g grad %.4g identical %.4g; lowest mean %.4f" % (SK.name_of(window), v, m, g, ident, lowest))
    for fig, emu in zip((v, m, g, ident), MK.EMU[window]):
        assert emu / 2 <= fig <= emu, (window, fig, emu)
    assert lowest >= MK.MIN_MEAN == 0.53
    assert MK.tolerances(window) == tuple(2.0 * e for e in MK.EMU[window]) and MK.TOL_FACTOR == 2.0


@pytest.mark.parametrize("window", sorted(MK.ODD_EMU), ids=SK.name_of)
def test_fp32_emulation_on_the_odd_sizes_leaves_the_figures_of_odd_emu(window):
    """The odd sizes of tests/test_gpu_msssimk.py -- (1, 1), (3, 5), (17, 33), (7, 300) at 1 .. 8 scales, (40, 300) at 4, (9, 603) at 3 --
    on their own seeded inputs: the figures the GPU is held to TOL_FACTOR times of, pinned from both sides."""
    import msssimk_inputs as IN
    assert [s for s, _ in IN.ODD_SIZES] == [(1, 1), (3, 5), (17, 33), (7, 300), (40, 300), (9, 603)]
    assert [c for _, c in IN.ODD_SIZES] == [tuple(range(1, 9))] * 4 + [(4,), (3,)]
    v, m, g, lowest = MK.measure_odd(window, IN.odd_cases())
    print("%s: value %.4g mean %.4g grad %.4g; lowest mean %.4f" % (SK.name_of(window), v, m, g, lowest))
    for fig, emu in zip((v, m, g), MK.ODD_EMU[window]):
        assert emu / 2 <= fig <= emu, (window, fig, emu)
    assert lowest >= MK.ODD_MIN_MEAN


def test_emu_covers_the_windows_and_configurations_of_the_issue():
    assert tuple(MK.EMU) == tuple(SK.WINDOWS) and len(SK.WINDOWS) == 7
    assert [(s, None if w is None else len(w)) for s, w in MK.CONFIGS] == [(5, None), (1, 1), (3, 3), (8, 8)]
    for s, w in MK.CONFIGS[1:]:
        assert abs(sum(w) - 1.0) < 1e-12 and len(set(w)) == 1


# ---- the C ABI's validation (no device needed) ----

def _is_h(fn):
    return "msssimh" in fn


def _params(fn, a, b, n=1, **over):
    h, w = a.shape
    if _is_h(fn):
        ps = (ssim_amd.Params16 * n)()
        for i in range(n):
            ps[i] = ssim_amd.make_params16(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w)
    else:
        ps = (ssim_amd.ParamsF * n)()
        for i in range(n):
            ps[i] = ssim_amd.make_params_f(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w)
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _grads(fn, a, n=1):
    G = ssim_amd.GradH if _is_h(fn) else ssim_amd.GradF
    gs = (G * n)()
    for i in range(n):
        gs[i] = G(a.ctypes.data, 1, a.shape[1])
    return gs


def _weights(w):
    return None if w is None else (ctypes.c_double * len(w))(*w)


GOOD = ssim_amd.Window(7, ssim_amd.WINDOW_UNIFORM, 0.0)


def test_entry_points_are_exported(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS, name
    assert lib.rmgr_ssim_hip_get_abi_version() == 6
    with open(os.path.join(ROOT, "ssim_amd", "csrc", "exports.map")) as f:
        assert "rmgr_ssim_*;" in f.read()
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"rmgr_int32_t %s\(" % name, header), name


def test_window_is_the_last_keyword_of_the_binding():
    fns = [ssim_amd.compute_msssimf, ssim_amd.compute_msssimf_batch, ssim_amd.compute_msssimh, ssim_amd.compute_msssimh_batch]
    fns += [getattr(ssim_amd.Context, n) for n in ("msssimf_device", "enqueue_msssimf", "enqueue_msssimf_grad", "msssimh_device",
                                                    "enqueue_msssimh", "enqueue_msssimh_grad")]
    for fn in fns:
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "window" and last.default is None, fn


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    half = _is_h(fn)
    dt = np.uint16 if half else np.float32
    a, b, ga = np.zeros((20, 30), dt), np.zeros((20, 30), dt), np.zeros((20, 30), dt)
    grad, enq = fn.endswith("_grad"), fn.endswith("_win")
    fake = ctypes.c_void_p(16)                                                                          # never dereferenced
    fake_ctx = None if fn.endswith("_host") else ctypes.c_void_p(1)                                     # never dereferenced
    out = fake if (grad or enq) else (ctypes.c_float * 4)()
    E = errno.EINVAL
    f = getattr(lib, fn)

    def rc(count=1, params=None, t=ssim_amd.SAMPLE_BF16, r=1.0, win=GOOD, scales=5, w=None, o=out, ctx=fake_ctx, grads=None, means=fake):
        ps = _params(fn, a, b, max(count, 1)) if params is None else params
        head = (ctx, count, ps, t, r) if half else (ctx, count, ps, r)
        head += (None if win is None else ctypes.byref(win), scales, _weights(w))
        if grad:
            ga_, gb_ = (_grads(fn, ga, max(count, 1)), None) if grads is None else grads
            return f(*(head + (means, o, ga_, gb_)))
        if enq:
            return f(*(head + (o, means)))
        return f(*(head + (o, None)))

    # the window: a bad size, kind or sigma, with everything else valid -- and a context that is never dereferenced
    for size in (4, 13, 0, 1, 2, 6, 12, 0xFFFFFFFF):
        assert rc(win=ssim_amd.Window(size, ssim_amd.WINDOW_GAUSSIAN, 1.5)) == E, size
        assert rc(win=ssim_amd.Window(size, ssim_amd.WINDOW_UNIFORM, 0.0)) == E, size
    for kind in (2, 7, 0xFFFFFFFF):
        assert rc(win=ssim_amd.Window(7, kind, 1.5)) == E
    for sigma in (0.0, -1.5, float("nan"), float("inf"), float("-inf")):
        for size in (3, 11):
            assert rc(win=ssim_amd.Window(size, ssim_amd.WINDOW_GAUSSIAN, sigma)) == E, (size, sigma)
    if not fn.endswith("_host"):
        assert rc(win=ssim_amd.Window(4, ssim_amd.WINDOW_GAUSSIAN, 1.5), ctx=None) == E
    # everything the entries without _win refuse, under a valid window, under NULL and under the engine's own
    for win in (GOOD, None, ssim_amd.Window(11, ssim_amd.WINDOW_GAUSSIAN, 1.5), ssim_amd.Window(3, ssim_amd.WINDOW_UNIFORM, float("nan"))):
        def k(**kw):
            return rc(win=win, **kw)
        assert k(count=0) == E
        assert k(o=None) == E                                                  # msssim / valuesDevice / gradOutDevice NULL
        if grad or enq:
            assert k(means=None) == E                                          # scaleMeansDevice NULL
        assert k(params=_params(fn, a, b, width=0)) == E
        assert k(params=_params(fn, a, b, height=0)) == E
        assert k(params=_params(fn, a, b, width=0x7FFF0001)) == E              # above the kernels' limit
        two = _params(fn, a, b, 2)
        two[1].width = 29
        assert k(count=2, params=two) == E                                     # sizes differ
        bad = _params(fn, a, b)
        bad[0].imgA.topLeft = None
        assert k(params=bad) == E
        bad = _params(fn, a, b, 2)
        bad[1].imgB.topLeft = a.ctypes.data + 1                                # not aligned to a sample
        assert k(count=2, params=bad) == E
        for r in (0.0, -1.0, float("inf"), float("nan")):
            assert k(r=r) == E
        if half:
            for t in (2, 7):
                assert k(t=t) == E
        for scales in (0, 9, 100):
            assert k(scales=scales, w=[0.1] * max(scales, 1)) == E
        for scales in (1, 4, 6, 8):
            assert k(scales=scales, w=None) == E                               # NULL weights are Wang's five
        for w in ([0.2, -0.1, 0.9], [0.2, float("nan"), 0.8], [float("inf"), 0.5, 0.5]):
            assert k(scales=3, w=w) == E
        m = np.zeros((20, 30), np.float32)
        bad = _params(fn, a, b, 2)
        bad[1].ssimMap = m.ctypes.data
        assert k(count=2, params=bad) == E                                     # a map
        if not fn.endswith("_host"):
            assert k(ctx=None) == E                                            # these entries need a context
        if grad:
            assert k(grads=(None, None)) == E                                  # both gradient arrays NULL
            g = _grads(fn, ga, 2)
            g[1].topLeft = None
            assert k(count=2, grads=(g, None)) == E and k(count=2, grads=(None, g)) == E
            g = _grads(fn, ga)
            g[0].topLeft = ga.ctypes.data + 1
            assert k(grads=(g, None)) == E
    # params NULL
    head = (fake_ctx, 1, None, ssim_amd.SAMPLE_F16, 1.0) if half else (fake_ctx, 1, None, 1.0)
    head += (ctypes.byref(GOOD), 5, None)
    tail = (fake, out, _grads(fn, ga), None) if grad else (out, fake if enq else None)
    assert f(*(head + tail)) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    box3 = ssim_amd.make_window(3, kind="uniform")
    if ssim_amd.device_count() > 0:
        v = ssim_amd.compute_msssimf(np.full((8, 8), 0.25, np.float32), np.full((8, 8), 0.25, np.float32), 1.0, window=box3)
        assert abs(float(v) - 1.0) < 1e-6
        return
    a = np.zeros((20, 30), np.float32)
    h = np.zeros((20, 30), np.uint16)
    out = (ctypes.c_float * 1)()
    wins = (None, ssim_amd.Window(11, ssim_amd.WINDOW_GAUSSIAN, 1.5), ssim_amd.Window(3, ssim_amd.WINDOW_UNIFORM, float("nan")),
            ssim_amd.Window(9, ssim_amd.WINDOW_GAUSSIAN, 0.5), ssim_amd.Window(11, ssim_amd.WINDOW_UNIFORM, 0.0))
    for win in wins:
        ref = None if win is None else ctypes.byref(win)
        for r, scales, w in ((1.0, 5, None), (255.0, 1, [1.0]), (1000.0, 8, [0.125] * 8)):
            fnf, fnh = "rmgr_ssim_hip_compute_msssimf_win_host", "rmgr_ssim_hip_compute_msssimh_win_host"
            assert lib.rmgr_ssim_hip_compute_msssimf_win_host(None, 1, _params(fnf, a, a), r, ref, scales, _weights(w), out, None) == errno.ENODEV
            for t in (ssim_amd.SAMPLE_F16, ssim_amd.SAMPLE_BF16):
                assert lib.rmgr_ssim_hip_compute_msssimh_win_host(None, 1, _params(fnh, h, h), t, r, ref, scales, _weights(w), out, None) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssimf(a, a, 1.0, window=box3)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssimf_batch([(a, a), (a, a)], 1.0, per_scale=True, window=box3)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssimh(h.view(np.float16), h.view(np.float16), 1.0, window=box3)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssimh_batch([(h, h)], 1.0, sample_type="bfloat16", window=box3)


def test_binding_refuses_a_window_that_is_no_window():
    a = np.zeros((20, 30), np.float32)
    h = np.zeros((20, 30), np.float16)
    for bad in (7, (7, 1.5), "uniform", {"size": 7}, 1.5):
        with pytest.raises(TypeError):
            ssim_amd.compute_msssimf(a, a, 1.0, window=bad)
        with pytest.raises(TypeError):
            ssim_amd.compute_msssimf_batch([(a, a)], 1.0, window=bad)
        with pytest.raises(TypeError):
            ssim_amd.compute_msssimh(h, h, 1.0, window=bad)
        with pytest.raises(TypeError):
            ssim_amd.compute_msssimh_batch([(h, h)], 1.0, window=bad)


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 3, 16, 16)
    for fn in (torch_ops.ms_ssim, torch_ops.ms_ssim_amp):
        for kw in (dict(win_size=7.0), dict(win_size="7"), dict(win_size=True), dict(win_size=None), dict(window=1), dict(window=None)):
            with pytest.raises(TypeError):
                fn(x, x, **kw)
        for kw in (dict(win_size=4), dict(win_size=13), dict(win_size=0), dict(win_size=-3), dict(window="box"), dict(window="Gaussian"),
                   dict(win_sigma=0.0), dict(win_sigma=-1.0), dict(win_sigma=float("nan")), dict(win_sigma=float("inf"))):
            with pytest.raises(ValueError):
                fn(x, x, **kw)
        # valid windows: CPU tensors are still the ValueError of every other call
        for kw in (dict(win_size=7), dict(win_size=3, window="uniform"), dict(win_sigma=2.0), dict(window="uniform", win_sigma=float("nan"))):
            with pytest.raises(ValueError, match="GPU|cuda|device"):
                fn(x, x, **kw)
    # positional: the three keywords follow weights
    with pytest.raises(ValueError):
        torch_ops.ms_ssim(x, x, 1.0, 5, None, 4)
    with pytest.raises(TypeError):
        torch_ops.ms_ssim(x, x, 1.0, 5, None, 7, 1.5, 3)
    # ms_ssim keeps its pinned refusal of 16-bit tensors, under any window; ms_ssim_amp takes them on a GPU only
    with pytest.raises(TypeError, match="float32 tensors expected"):
        torch_ops.ms_ssim(x.half(), x.half(), win_size=7)
    with pytest.raises(TypeError, match="GPU only"):
        torch_ops.ms_ssim_amp(x.bfloat16(), x.bfloat16(), win_size=7)
    # the loss checks its window where it is made
    with pytest.raises(ValueError):
        torch_ops.MSSSIMLoss(win_size=4)
    with pytest.raises(ValueError):
        torch_ops.MSSSIMLoss(window="box")
    with pytest.raises(ValueError):
        torch_ops.MSSSIMLoss(win_sigma=0.0)
    with pytest.raises(TypeError):
        torch_ops.MSSSIMLoss(win_size=7.0)
    with pytest.raises(TypeError):
        torch_ops.MSSSIMLoss(window=3)
    with pytest.raises(ValueError):
        torch_ops.MSSSIMLoss(1.0, 5, None, "mean", 4)                          # positional: after reduction
    loss = torch_ops.MSSSIMLoss(win_size=3, window="uniform")
    assert (loss.win_size, loss.window) == (3, "uniform")
    with pytest.raises(ValueError):
        loss(x, x)                                                             # CPU tensors
    with pytest.raises(ValueError):
        torch_ops.MSSSIMLoss(1.0, 5, None, "none")(x, x)                       # an existing positional call keeps working


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; "
                        "w = ssim_amd.make_window(7); assert 'window' in ssim_amd.compute_msssimf.__code__.co_varnames; "
                        "assert hasattr(ssim_amd.torch_ops, 'ms_ssim_amp') and 'torch' not in sys.modules" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- kernel budgets ----

def _resource_usage(src):
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
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
    return kernels


@pytest.mark.parametrize("stem,strips,grads", [("msssimk", 8, 24), ("msssimhk", 16, 48)])
def test_windowed_multi_scale_kernels_keep_their_budgets(stem, strips, grads):
    """Build-time guard from the compiler's remarks, with the command line and the numbers tests/test_msssimf_cpu.py holds the 11-tap
    kernels to: nothing spills; the strip kernels keep three waves per SIMD (at most 168 VGPRs, LDS for 12 waves per CU); the gradient
    kernels two workgroups of 256 lanes per CU (at most 128 VGPRs, at most 64 KiB of LDS per workgroup).  msssimk_kernels.hip: R = 1 .. 4 x
    {2 strip forms, 6 gradient forms}; msssimhk_kernels.hip: the same under two encodings; no other kernel in either file."""
    kernels = _resource_usage(os.path.join(ROOT, "ssim_amd", "csrc", stem + "_kernels.hip"))
    strip = {k: v for k, v in kernels.items() if stem + "_strip" in k}
    grad = {k: v for k, v in kernels.items() if stem + "_grad" in k}
    assert len(strip) == strips and len(grad) == grads and len(kernels) == strips + grads, sorted(kernels)
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in strip.items():
        assert v["VGPRs"] <= 168 and v["Occupancy"] >= 3 and v["LDS"] <= 13312, (k, v)
    for k, v in grad.items():
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 2 and v["LDS"] <= 65536, (k, v)
