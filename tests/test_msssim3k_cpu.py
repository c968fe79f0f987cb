"""CPU: multi-scale SSIM of volumes under a caller-chosen window -- the definition and its boundaries (include/rmgr/ssim-hip.h,
rmgr_ssim_hip_*_msssim3f_win* and rmgr_ssim_hip_*_msssim3h_win*).  Sizes are W x H x D; arrays are (D, H, W).

  * tests/msssim3k_model.py at the default window IS tests/msssim3f_model.py: the float64 model returns its values exactly, the fp32
    emulation reproduces its emulation bit for bit (value, means, gradients); with one scale of weight 1 the model is ssim3k_model's and
    the emulation is ssim3k_model.emulate_fp32 bit for bit;
  * the model's gradient is the derivative of the model's value under small and box windows, on a volume smaller than the window at
    coarse scales;
  * per window the fp32 emulation leaves the figures of msssim3k_model.EMU / ODD_EMU against the float64 model, pinned from both sides,
    and no case sits near the ReLU: every mean that enters a product is at least 0.5 on the golden volumes and 0.9 on the odd sizes;
  * the eight entry points are exported, declared and listed, every EINVAL -- a bad window included -- comes before the device, a valid
    call without a device is ENODEV, the binding refuses a window that is no Window, ssim_amd.torch_ops refuses what it documents before
    any GPU call, and the two new kernel files keep the budgets tests/test_msssim3f_cpu.py holds the 11-tap forms to.
"""
import ctypes
import errno
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import msssim3f_model as M3
import msssim3k_inputs as IN
import msssim3k_model as MK
import ssim3k_model as K3
import ssim_amd
from conftest import ROOT

ENTRY_POINTS_F = ("rmgr_ssim_hip_enqueue_msssim3f_win", "rmgr_ssim_hip_compute_msssim3f_win_device", "rmgr_ssim_hip_compute_msssim3f_win_host",
                  "rmgr_ssim_hip_enqueue_msssim3f_win_grad")
ENTRY_POINTS_H = tuple(n.replace("msssim3f", "msssim3h") for n in ENTRY_POINTS_F)
ENTRY_POINTS = ENTRY_POINTS_F + ENTRY_POINTS_H
F16, BF16 = ssim_amd.SAMPLE_F16, ssim_amd.SAMPLE_BF16


# ---- the model ----

def test_default_window_is_msssim3f_model_exactly_and_its_emulation_bit_for_bit(manifest):
    for n in ("bbb257x65_q50_ch1", "einstein_blur"):
        for _, fa, fb, r in K3.fixture_forms(manifest, n):
            fa, fb = fa[:, :33, 5:64], fb[:, :33, 5:64]                # across tiles, odd sizes; 12 slices
            mod, ref = MK.Model(fa, fb, r), M3.Model(fa, fb, r)
            emu, eref = MK.Emulation(fa, fb, r), M3.Emulation(fa, fb, r)
            for scales, w in MK.CONFIGS:
                (v, m), (rv, rm) = mod.msssim(scales, w), ref.msssim(scales, w)
                assert v == rv and np.array_equal(m, rm)
                for g, rg in zip(mod.grad(-0.75, scales, w), ref.grad(-0.75, scales, w)):
                    assert np.array_equal(g, rg)
                (v, m), (rv, rm) = emu.msssim(scales, w), eref.msssim(scales, w)
                assert v == rv and np.array_equal(m, rm)
                for g, rg in zip(emu.grad(-0.75, scales, w), eref.grad(-0.75, scales, w)):
                    assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), rg.view(np.uint32))


@pytest.mark.parametrize("window", MK.WINDOWS, ids=MK.name_of)
def test_one_scale_of_weight_one_is_the_ssim3k_model(manifest, window):
    _, a, b, r = K3.fixture_forms(manifest, "bbb257x65_q50_ch1")[0]
    a, b = a[:, :20, 100:133], b[:, :20, 100:133]
    mod = MK.Model(a, b, r, window)
    v, means = mod.msssim(1, (1.0,))
    want, _ = K3.ssim(a, b, r, window)
    assert abs(v - want) <= 1e-12 * abs(want) and abs(means[0][1] - want) <= 1e-12 * abs(want)
    for g, wg in zip(mod.grad(-0.75, 1, (1.0,)), K3.grad(a, b, r, -0.75, window)):
        assert np.abs(g - wg).max() <= 1e-12 * np.abs(wg).max()
    # the emulation of one scale is ssim3k_model's emulation of that window, bit for bit: gOut = 1 makes k_0 = float(1 w MS / m / (W H D))
    # the number float(1 / (W H D)) that family rounds
    emu = MK.Emulation(a, b, r, window)
    ev, _, ea, eb = K3.emulate_fp32(a, b, r, window, g_out=1.0)
    assert emu.msssim(1, (1.0,))[0] == ev
    for g, wg in zip(emu.grad(1.0, 1, (1.0,)), (ea, eb)):
        assert np.abs(wg).max() > 0 and np.array_equal(g.view(np.uint32), wg.view(np.uint32))


def test_gradient_is_the_derivative_of_the_value_under_small_windows():
    """Central differences of the model's own MS at steps 1e-5 and 5e-6 (range 1) against grad(), with the bound of
    tests/test_msssimk_cpu.py, on tiny volumes that become smaller than the window at coarse scales."""
    rng = np.random.default_rng(11)
    cases = (((3, 0.0, "uniform"), 0, (0.25,) * 4), ((9, 1.5, "gaussian"), 2, (0.5, 0.3, 0.2)), ((7, 0.0, "uniform"), 1, (0.5, 0.5)),
             ((5, 0.8, "gaussian"), 2, (0.3, 0.0, 0.7)))
    for window, index, wts in cases:
        ca, cb = (v.astype(np.float64) for v in IN.odd_pair(index))
        d, h, w = ca.shape
        g_out, scales = -0.75, len(wts)
        grads = MK.Model(ca, cb, 1.0, window).grad(g_out, scales, wts)
        pts = {(0, 0, 0), (d - 1, h - 1, w - 1), (d // 2, h // 2, w // 2)}
        while len(pts) < min(5, d * h * w):
            pts.add((int(rng.integers(0, d)), int(rng.integers(0, h)), int(rng.integers(0, w))))
        for which, gr in enumerate(grads):
            scale = np.abs(gr).max()
            for eps in (1e-5, 5e-6):
                for p3 in sorted(pts):
                    p, m = [ca.copy(), cb.copy()], [ca.copy(), cb.copy()]
                    p[which][p3] += eps
                    m[which][p3] -= eps
                    fd = g_out * (MK.Model(p[0], p[1], 1.0, window).msssim(scales, wts)[0] -
                                  MK.Model(m[0], m[1], 1.0, window).msssim(scales, wts)[0]) / (2 * eps)
                    assert abs(fd - gr[p3]) <= 1e-6 * scale, (window, (w, h, d), which, p3, eps, fd, gr[p3])


@pytest.mark.parametrize("window", MK.WINDOWS, ids=MK.name_of)
def test_fp32_emulation_leaves_the_figures_of_emu(manifest, window):
    """Emulation against the float64 model on ssim3f_model.FIXTURES x FORMS at Wang's 5 scales and at uniform weights for 1, 3 and 8
    scales: value, every per-scale mean, both gradients, and the pair of identical volumes.  tests/test_gpu_msssim3k.py asserts
    TOL_FACTOR x these figures.  Conditioning: every mean that enters a product is at least MIN_MEAN = 0.5."""
    v, m, g, ident, lowest = MK.measure(manifest, window)
    print("%s: value %.4g mean %.4g grad %.4g identical %.4g; lowest mean %.4f" % (MK.name_of(window), v, m, g, ident, lowest))
    for fig, emu in zip((v, m, g, ident), MK.EMU[window]):
        assert emu / 2 <= fig <= emu, (window, fig, emu)
    assert lowest >= MK.MIN_MEAN == 0.5
    assert MK.tolerances(window) == tuple(2.0 * e for e in MK.EMU[window]) and MK.TOL_FACTOR == 2.0


@pytest.mark.parametrize("window", MK.WINDOWS, ids=MK.name_of)
def test_fp32_emulation_on_the_odd_sizes(window):
    """The seeded odd sizes of tests/msssim3k_inputs.py at 8 uniform scales: every mean that enters a product is at least 0.9 under every
    window; under the two windows the GPU runs them with, the figures it is held to TOL_FACTOR times of, pinned from both sides."""
    v, m, g, lowest = MK.measure_odd(window, IN.odd_cases(), IN.ODD_SCALES)
    print("%s: value %.4g mean %.4g grad %.4g; lowest mean %.4f" % (MK.name_of(window), v, m, g, lowest))
    assert lowest >= MK.ODD_MIN_MEAN == 0.9
    if window in MK.ODD_EMU:
        for fig, emu in zip((v, m, g), MK.ODD_EMU[window]):
            assert emu / 2 <= fig <= emu, (window, fig, emu)
        assert MK.odd_tolerances(window) == tuple(2.0 * e for e in MK.ODD_EMU[window])


def test_emu_covers_the_windows_configurations_and_sizes_of_the_issue():
    assert tuple(MK.EMU) == tuple(MK.WINDOWS) and len(MK.WINDOWS) == 7
    assert [(s, None if w is None else len(w)) for s, w in MK.CONFIGS] == [(5, None), (1, 1), (3, 3), (8, 8)]
    for s, w in MK.CONFIGS[1:]:
        assert abs(sum(w) - 1.0) < 1e-12 and len(set(w)) == 1
    assert IN.ODD_SIZES == ((1, 1, 1), (2, 1, 3), (7, 5, 3), (9, 9, 9), (17, 3, 33), (33, 20, 13), (16, 16, 8), (37, 21, 44))
    assert tuple(sorted(MK.ODD_EMU)) == tuple(sorted(IN.ODD_WINDOWS)) == ((3, 0.0, "uniform"), (9, 1.5, "gaussian")) and IN.ODD_SCALES == 8
    for i, (w, h, d) in enumerate(IN.ODD_SIZES):
        a, b = IN.odd_pair(i)
        assert a.shape == b.shape == (d, h, w) and a.dtype == b.dtype == np.float32
    # the generator: a's noise first, then b's, from default_rng(0x3D00 + index)
    rng = np.random.default_rng(0x3D00 + 1)
    na = rng.standard_normal((3, 1, 2))
    a, b = IN.odd_pair(1)
    z, y, x = np.meshgrid(np.arange(3), np.arange(1), np.arange(2), indexing="ij")
    want = (0.2 + 0.6 * (x + 2 * y + 3 * z) / (2 + 2 * 1 + 3 * 3) + 0.05 * na).astype(np.float32)
    assert np.array_equal(a, want) and np.array_equal(b, (want + 0.02 * rng.standard_normal((3, 1, 2))).astype(np.float32))


# ---- the C ABI's validation (no device needed) ----

def _is_h(fn):
    return "msssim3h" in fn


def _params(fn, a, b, n=1, **over):
    d, h, w = a.shape
    P, make = (ssim_amd.Params3H, ssim_amd.make_params3h) if _is_h(fn) else (ssim_amd.Params3F, ssim_amd.make_params3f)
    ps = (P * n)()
    for i in range(n):
        ps[i] = make(w, h, d, a.ctypes.data, (1, w, w * h), b.ctypes.data, (1, w, w * h))
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _grads(fn, a, n=1):
    G = ssim_amd.Grad3H if _is_h(fn) else ssim_amd.Grad3F
    gs = (G * n)()
    for i in range(n):
        gs[i] = G(a.ctypes.data, 1, a.shape[2], a.shape[2] * a.shape[1])
    return gs


def _weights(w):
    return None if w is None else (ctypes.c_double * len(w))(*w)


GOOD = ssim_amd.Window(7, ssim_amd.WINDOW_UNIFORM, 0.0)


def test_entry_points_are_exported_declared_and_listed(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS, name
    assert lib.rmgr_ssim_hip_get_abi_version() == 6 and ssim_amd.ABI_VERSION == 6
    with open(os.path.join(ROOT, "ssim_amd", "csrc", "exports.map")) as f:
        assert "rmgr_ssim_*;" in f.read()
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"rmgr_int32_t %s\(" % name, header), name


def test_window_is_the_last_keyword_of_the_binding():
    fns = [ssim_amd.compute_msssim3f, ssim_amd.compute_msssim3f_batch, ssim_amd.compute_msssim3h, ssim_amd.compute_msssim3h_batch]
    fns += [getattr(ssim_amd.Context, n) for n in ("msssim3f_device", "enqueue_msssim3f", "enqueue_msssim3f_grad", "msssim3h_device",
                                                    "enqueue_msssim3h", "enqueue_msssim3h_grad")]
    assert len(fns) == 10
    for fn in fns:
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "window" and last.default is None, fn


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    """The fake context and the fake device pointers are never dereferenced: an EINVAL that came after the first use of the context would
    crash."""
    half = _is_h(fn)
    dt = np.uint16 if half else np.float32
    a, b, ga = np.zeros((6, 20, 30), dt), np.zeros((6, 20, 30), dt), np.zeros((6, 20, 30), dt)
    grad, enq = fn.endswith("_grad"), fn.endswith("_win")
    fake = ctypes.c_void_p(16)                                                                          # never dereferenced
    fake_ctx = None if fn.endswith("_host") else ctypes.c_void_p(1)                                     # never dereferenced
    out = fake if (grad or enq) else (ctypes.c_float * 4)()
    E = errno.EINVAL
    f = getattr(lib, fn)

    def rc(count=1, params=None, t=BF16, r=1.0, win=GOOD, scales=5, w=None, o=out, ctx=fake_ctx, grads=None, means=fake):
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
        for dim in ("width", "height", "depth"):
            assert k(params=_params(fn, a, b, **{dim: 0})) == E
            assert k(params=_params(fn, a, b, **{dim: 0x7FFF0001})) == E       # above the kernels' limit
            two = _params(fn, a, b, 2)
            setattr(two[1], dim, getattr(two[1], dim) - 1)
            assert k(count=2, params=two) == E                                 # sizes differ
        assert k(params=_params(fn, a, b, width=0x7FFF0000, height=0x7FFF0000)) == E      # more tiles than a launch holds
        bad = _params(fn, a, b)
        bad[0].imgA.topLeft = None
        assert k(params=bad) == E
        bad = _params(fn, a, b, 2)
        bad[1].imgB.topLeft = a.ctypes.data + 1                                # not aligned to a sample
        assert k(count=2, params=bad) == E
        for r in (0.0, -1.0, float("inf"), float("nan")):
            assert k(r=r) == E
        if half:
            for t in (2, 3, 0xFFFF, 0xFFFFFFFF):                               # a sampleType that is neither constant
                assert k(t=t) == E
        for scales in (0, 9, 100):
            assert k(scales=scales, w=[0.1] * max(scales, 1)) == E
        for scales in (1, 4, 6, 8):
            assert k(scales=scales, w=None) == E                               # NULL weights are Wang's five
        for w in ([0.2, -0.1, 0.9], [0.2, float("nan"), 0.8], [float("inf"), 0.5, 0.5]):
            assert k(scales=3, w=w) == E
        m = np.zeros((6, 20, 30), np.float32)
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
    head = (fake_ctx, 1, None, F16, 1.0) if half else (fake_ctx, 1, None, 1.0)
    head += (ctypes.byref(GOOD), 5, None)
    tail = (fake, out, _grads(fn, ga), None) if grad else (out, fake if enq else None)
    assert f(*(head + tail)) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    box3 = ssim_amd.make_window(3, kind="uniform")
    if ssim_amd.device_count() > 0:
        v = ssim_amd.compute_msssim3f(np.full((4, 8, 8), 0.25, np.float32), np.full((4, 8, 8), 0.25, np.float32), 1.0, window=box3)
        assert abs(float(v) - 1.0) < 1e-6
        return
    a = np.zeros((6, 20, 30), np.float32)
    h = np.zeros((6, 20, 30), np.uint16)
    out = (ctypes.c_float * 1)()
    wins = (None, ssim_amd.Window(11, ssim_amd.WINDOW_GAUSSIAN, 1.5), ssim_amd.Window(3, ssim_amd.WINDOW_UNIFORM, float("nan")),
            ssim_amd.Window(9, ssim_amd.WINDOW_GAUSSIAN, 0.5), ssim_amd.Window(11, ssim_amd.WINDOW_UNIFORM, 0.0))
    fnf, fnh = "rmgr_ssim_hip_compute_msssim3f_win_host", "rmgr_ssim_hip_compute_msssim3h_win_host"
    for win in wins:
        ref = None if win is None else ctypes.byref(win)
        for r, scales, w in ((1.0, 5, None), (255.0, 1, [1.0]), (1000.0, 8, [0.125] * 8)):
            assert lib.rmgr_ssim_hip_compute_msssim3f_win_host(None, 1, _params(fnf, a, a), r, ref, scales, _weights(w), out, None) == errno.ENODEV
            for t in (F16, BF16, 0):                                           # 0 is RMGR_SSIM_HIP_SAMPLE_F16 and valid
                assert lib.rmgr_ssim_hip_compute_msssim3h_win_host(None, 1, _params(fnh, h, h), t, r, ref, scales, _weights(w), out, None) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssim3f(a, a, 1.0, window=box3)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssim3f_batch([(a, a), (a, a)], 1.0, per_scale=True, window=box3)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssim3h(h.view(np.float16), h.view(np.float16), 1.0, window=box3)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssim3h_batch([(h, h)], 1.0, sample_type="bfloat16", window=box3)


def test_binding_refuses_a_window_that_is_no_window():
    a = np.zeros((4, 8, 8), np.float32)
    h = np.zeros((4, 8, 8), np.float16)
    for bad in (7, (7, 1.5), "uniform", {"size": 7}, 1.5):
        with pytest.raises(TypeError):
            ssim_amd.compute_msssim3f(a, a, 1.0, window=bad)
        with pytest.raises(TypeError):
            ssim_amd.compute_msssim3f_batch([(a, a)], 1.0, window=bad)
        with pytest.raises(TypeError):
            ssim_amd.compute_msssim3h(h, h, 1.0, window=bad)
        with pytest.raises(TypeError):
            ssim_amd.compute_msssim3h_batch([(h, h)], 1.0, window=bad)


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 3, 8, 16, 16)
    for fn in (torch_ops.ms_ssim3d, torch_ops.ms_ssim3d_amp):
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
        torch_ops.ms_ssim3d(x, x, 1.0, 5, None, 4)
    with pytest.raises(TypeError):
        torch_ops.ms_ssim3d(x, x, 1.0, 5, None, 7, 1.5, 3)
    # ms_ssim3d keeps its pinned refusal of 16-bit tensors, under any window; ms_ssim3d_amp takes them on a GPU only
    with pytest.raises(TypeError, match="^ms_ssim3d: the 3-D multi-scale path is float32 for now"):
        torch_ops.ms_ssim3d(x.half(), x.half(), win_size=7)
    with pytest.raises(TypeError, match="GPU only"):
        torch_ops.ms_ssim3d_amp(x.bfloat16(), x.bfloat16(), win_size=7)
    # the loss checks its window where it is made
    with pytest.raises(ValueError):
        torch_ops.MSSSIM3DLoss(win_size=4)
    with pytest.raises(ValueError):
        torch_ops.MSSSIM3DLoss(window="box")
    with pytest.raises(ValueError):
        torch_ops.MSSSIM3DLoss(win_sigma=0.0)
    with pytest.raises(TypeError):
        torch_ops.MSSSIM3DLoss(win_size=7.0)
    with pytest.raises(TypeError):
        torch_ops.MSSSIM3DLoss(window=3)
    with pytest.raises(ValueError):
        torch_ops.MSSSIM3DLoss(1.0, 5, None, "mean", 4)                        # positional: after reduction
    loss = torch_ops.MSSSIM3DLoss(win_size=3, window="uniform")
    assert (loss.win_size, loss.window) == (3, "uniform")
    with pytest.raises(ValueError):
        loss(x, x)                                                             # CPU tensors
    with pytest.raises(ValueError):
        torch_ops.MSSSIM3DLoss(1.0, 5, None, "none")(x, x)                     # an existing positional call keeps working


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; "
                        "w = ssim_amd.make_window(7); assert 'window' in ssim_amd.compute_msssim3f.__code__.co_varnames; "
                        "ssim_amd.torch_ops.MSSSIM3DLoss(win_size=3, window='uniform'); "
                        "assert hasattr(ssim_amd.torch_ops, 'ms_ssim3d_amp') and 'torch' not in sys.modules" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- kernel budgets ----

def _resource_usage(src):
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src), "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=1800)
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


@pytest.mark.parametrize("stem,encodings", [("msssim3k", 1), ("msssim3hk", 2)])
def test_windowed_multi_scale_volume_kernels_keep_the_eleven_tap_budgets(stem, encodings):
    """Build-time guard from the compiler's remarks, with the command line and the numbers tests/test_msssim3f_cpu.py holds the 11-tap
    forms to.  msssim3k_kernels.hip: R = 1 .. 4 x (7 walks: the value walk with two sums; dA, dB, both in the cs form and in the ssim
    form; 6 adjoint walks: A, B, both x coarsest / finer) = 52 kernels; msssim3hk_kernels.hip: the same under two encodings, 104; no other
    kernel in either file.  None uses scratch; every walk and every one-gradient adjoint keeps 4 waves per SIMD or more (at most 128
    VGPRs), the both-gradients adjoints 3 or more (at most 168 VGPRs); LDS at most 17536 bytes."""
    kernels = _resource_usage(os.path.join(ROOT, "ssim_amd", "csrc", stem + "_kernels.hip"))
    walks = {k: v for k, v in kernels.items() if stem + "_walk_kernel" in k}
    adjoints = {k: v for k, v in kernels.items() if stem + "_adjoint_kernel" in k}
    assert len(walks) == 28 * encodings and len(adjoints) == 24 * encodings and len(kernels) == 52 * encodings, sorted(kernels)
    for k, v in sorted(kernels.items()):
        print(k, v)
        assert v["ScratchSize"] == 0 and v["LDS"] <= 17536, (k, v)
    for k, v in walks.items():
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 4, (k, v)
    for k, v in adjoints.items():
        # template arguments <[TYPE,] R, WHICH, MS>: WHICH is the last but one
        which = int(re.search(stem + r"_adjoint_kernelI(?:Li\dE)*Li(\d)ELi\dEEE", k).group(1))
        assert v["Occupancy"] >= (3 if which == 3 else 4) and v["VGPRs"] <= (168 if which == 3 else 128), (k, v)
