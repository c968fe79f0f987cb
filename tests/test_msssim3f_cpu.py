"""CPU: multi-scale SSIM of float32 volumes and its gradient -- the definition and its boundaries (include/rmgr/ssim-hip.h,
rmgr_ssim_hip_*_msssim3f*).  Sizes are W x H x D; arrays are (D, H, W).

  * the entry points are exported, declared and listed, the Python and torch names exist, the ABI version is 6;
  * every EINVAL comes before the device, a valid call without a device is ENODEV, and ssim_amd.torch_ops refuses what it documents
    before any GPU call, the 16-bit TypeError included;
  * the float64 model (tests/msssim3f_model.py) agrees within 1e-9 with an independent torch float64 restatement -- replicate-pad to even
    sizes, avg_pool3d(2), conv3d on replicate-padded input, autograd -- for value and both gradients, and with one scale of weight 1 it
    IS ssim3f_model;
  * the fp32 emulation of the kernels leaves the figures msssim3f_model.EMU_* hold, pinned from both sides, and restates the pyramid's
    order, the centre of every scale and the accumulation;
  * the inputs of the GPU module's accuracy tests keep every m_s with a weight at 0.2 or more, and the content classes it keeps leave the
    emulation within 85 % of the EMU figures;
  * the new kernels never spill and keep their budgets;
  * the scratch and sub-batch rule (tests/msssim3f_plan.py) agrees with the C++ (tests/src/msssim3f_plan_probe.cpp).
"""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import content_classes as C
import msssim3f_model as M
import msssim3f_plan as MP
import ssim3f_model as S
import ssim_amd
from conftest import ROOT

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_msssim3f", "rmgr_ssim_hip_compute_msssim3f_device", "rmgr_ssim_hip_compute_msssim3f_host",
                "rmgr_ssim_hip_enqueue_msssim3f_grad")
HIPCC = "/opt/rocm/bin/hipcc"
# the classes tests/test_gpu_msssim3f.py leaves out of accuracy: the emulation's own figures on them, in units of (EMU_VALUE, EMU_MEAN, EMU_GRAD)
DROPPED = ("offset above the range", "unit data at range 1e-6")


def uniform(n):
    return (1.0 / n,) * n


# ---- exports and declarations -----------------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_declared_and_listed(lib):
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS
        assert re.search(r"rmgr_int32_t %s\(" % name, header), name
    for name in ("compute_msssim3f", "compute_msssim3f_batch"):
        assert hasattr(ssim_amd, name)
    for name in ("msssim3f_device", "enqueue_msssim3f", "enqueue_msssim3f_grad"):
        assert hasattr(ssim_amd.Context, name)
    from ssim_amd import torch_ops
    assert hasattr(torch_ops, "ms_ssim3d") and hasattr(torch_ops, "MSSSIM3DLoss")
    assert lib.rmgr_ssim_hip_get_abi_version() == 6 and ssim_amd.ABI_VERSION == 6
    with open(os.path.join(ROOT, "ssim_amd", "csrc", "exports.map")) as f:
        assert "rmgr_ssim_*;" in f.read()


# ---- the C ABI's validation (no device needed) ------------------------------------------------------------------------------------------------

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


def _weights(w):
    return None if w is None else (ctypes.c_double * len(w))(*w)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    """The fake context and the fake device pointers are never dereferenced: an EINVAL that came after the first use of the context would
    crash."""
    a = np.zeros((6, 20, 30), np.float32)
    b = np.zeros((6, 20, 30), np.float32)
    ga = np.zeros((6, 20, 30), np.float32)
    grad, enq = fn.endswith("_grad"), fn.endswith("enqueue_msssim3f")
    fake = ctypes.c_void_p(16)
    fake_ctx = None if fn.endswith("_host") else ctypes.c_void_p(1)
    out = fake if (grad or enq) else (ctypes.c_float * 4)()
    E = errno.EINVAL
    f = getattr(lib, fn)

    def rc(count=1, params=None, r=1.0, scales=5, w=None, o=out, ctx=fake_ctx, grads=None, means=fake):
        ps = _params(a, b, max(count, 1)) if params is None else params
        if grad:
            ga_, gb_ = (_grads(ga, max(count, 1)), None) if grads is None else grads
            return f(ctx, count, ps, r, scales, _weights(w), means, o, ga_, gb_)
        if enq:
            return f(ctx, count, ps, r, scales, _weights(w), o, means)
        return f(ctx, count, ps, r, scales, _weights(w), o, None)
    assert rc(count=0) == E
    if grad:
        assert f(fake_ctx, 1, None, 1.0, 5, None, fake, out, _grads(ga), None) == E                      # params NULL
    else:
        assert f(fake_ctx, 1, None, 1.0, 5, None, out, fake if enq else None) == E
    assert rc(o=None) == E                                                     # msssim / valuesDevice / gradOutDevice NULL
    if grad or enq:
        assert rc(means=None) == E                                             # scaleMeansDevice NULL
    for dim in ("width", "height", "depth"):
        assert rc(params=_params(a, b, **{dim: 0})) == E
        assert rc(params=_params(a, b, **{dim: 0x7FFF0001})) == E              # above the kernels' limit
        two = _params(a, b, 2)
        setattr(two[1], dim, getattr(two[1], dim) - 1)
        assert rc(count=2, params=two) == E                                    # sizes differ
    assert rc(params=_params(a, b, width=0x7FFF0000, height=0x7FFF0000)) == E  # more tiles than a launch holds
    bad = _params(a, b)
    bad[0].imgA.topLeft = None
    assert rc(params=bad) == E
    bad = _params(a, b, 2)
    bad[1].imgB.topLeft = None
    assert rc(count=2, params=bad) == E
    for off in (1, 2, 3):
        bad = _params(a, b)
        bad[0].imgA.topLeft = a.ctypes.data + off                              # not 4-byte aligned
        assert rc(params=bad) == E
        bad = _params(a, b, 2)
        bad[1].imgB.topLeft = b.ctypes.data + off
        assert rc(count=2, params=bad) == E
    for r in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert rc(r=r) == E
    # the multi-scale rules: scales, weights, no map
    for scales in (0, 9, 100):
        assert rc(scales=scales, w=[0.1] * max(scales, 1)) == E
    for scales in (1, 4, 6, 8):
        assert rc(scales=scales, w=None) == E                                  # NULL weights are Wang's five
    for w in ([0.2, -0.1, 0.9], [0.2, float("nan"), 0.8], [float("inf"), 0.5, 0.5], [0.2, 0.3, float("-inf")]):
        assert rc(scales=3, w=w) == E
    m = np.zeros((6, 20, 30), np.float32)
    bad = _params(a, b, 2)
    bad[1].ssimMap = m.ctypes.data
    assert rc(count=2, params=bad) == E                                        # a map
    if not fn.endswith("_host"):
        assert rc(ctx=None) == E                                               # these entries need a context
        assert rc(ctx=None, scales=3, w=[0.2, 0.3, 0.5], r=255.0) == E
    if grad:
        assert rc(grads=(None, None)) == E                                     # both gradient arrays NULL
        g = _grads(ga, 2)
        g[1].topLeft = None
        assert rc(count=2, grads=(g, None)) == E and rc(count=2, grads=(None, g)) == E
        g = _grads(ga)
        g[0].topLeft = ga.ctypes.data + 2
        assert rc(grads=(g, None)) == E and rc(grads=(_grads(ga), g)) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    if ssim_amd.device_count() > 0:
        v = ssim_amd.compute_msssim3f(np.full((4, 8, 8), 0.25, np.float32), np.full((4, 8, 8), 0.25, np.float32), 1.0)
        assert abs(float(v) - 1.0) < 1e-6
        return
    a = np.zeros((6, 20, 30), np.float32)
    out = (ctypes.c_float * 1)()
    for r, scales, w in ((1.0, 5, None), (255.0, 1, [1.0]), (1000.0, 8, [0.125] * 8), (1.0, 3, [0.0, 0.0, 1.0])):
        assert lib.rmgr_ssim_hip_compute_msssim3f_host(None, 1, _params(a, a), r, scales, _weights(w), out, None) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssim3f(a, a, 1.0)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssim3f_batch([(a, a), (a, a)], 1.0, per_scale=True)


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 3, 8, 16, 16)
    with pytest.raises(ValueError, match="ms_ssim3d"):
        torch_ops.ms_ssim3d(x, x)                                              # CPU tensors
    with pytest.raises(ValueError, match="ms_ssim3d"):
        torch_ops.MSSSIM3DLoss()(x, x)
    with pytest.raises(TypeError, match="ms_ssim3d"):
        torch_ops.ms_ssim3d(x.double(), x.double())
    with pytest.raises(TypeError):
        torch_ops.ms_ssim3d(x.numpy(), x.numpy())
    for half in (torch.float16, torch.bfloat16):
        for p, q in ((x.to(half), x.to(half)), (x, x.to(half))):
            with pytest.raises(TypeError, match="ms_ssim3d: the 3-D multi-scale path is float32 for now"):
                torch_ops.ms_ssim3d(p, q)
        with pytest.raises(TypeError, match="3-D multi-scale path is float32 for now"):
            torch_ops.MSSSIM3DLoss()(x.to(half), x.to(half))
    with pytest.raises(ValueError, match="shapes differ"):
        torch_ops.ms_ssim3d(x, torch.zeros(2, 3, 8, 16, 15))
    with pytest.raises(ValueError, match="D, H, W"):
        torch_ops.ms_ssim3d(torch.zeros(16, 16), torch.zeros(16, 16))
    with pytest.raises(ValueError):
        torch_ops.ms_ssim3d(x, x, data_range=0.0)
    with pytest.raises(ValueError, match="MSSSIM3DLoss"):
        torch_ops.MSSSIM3DLoss(reduction="sum")
    for kw in (dict(scales=0), dict(scales=9, weights=[0.1] * 9), dict(scales=4), dict(scales=3, weights=[0.5, 0.5]),
               dict(scales=2, weights=[0.5, -0.5]), dict(scales=2, weights=[0.5, float("nan")]), dict(scales=2, weights=[float("inf"), 0.5])):
        with pytest.raises(ValueError, match="MSSSIM3DLoss"):
            torch_ops.MSSSIM3DLoss(**kw)
    with pytest.raises(TypeError, match="MSSSIM3DLoss"):
        torch_ops.MSSSIM3DLoss(scales=2.0, weights=[0.5, 0.5])
    # ms_ssim keeps its own name in its messages
    with pytest.raises(ValueError, match="^ms_ssim: "):
        torch_ops.MSSSIMLoss(scales=4)


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; "
                        "ssim_amd.torch_ops.MSSSIM3DLoss(scales=2, weights=(0.5, 0.5)); "
                        "assert hasattr(ssim_amd.torch_ops, 'ms_ssim3d') and 'torch' not in sys.modules" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------

def _torch_restatement(a, b, data_range, scales, weights, g_out):
    """(value, means, dA, dB) by torch float64: replicate-pad to even sizes + avg_pool3d(2) for the pyramid, 1-D conv3d per axis on
    replicate-padded volumes for the statistics, the ReLU'd weighted product, autograd."""
    import torch
    import torch.nn.functional as Fn
    g = torch.tensor(S.gaussian_taps(), dtype=torch.float64)
    c1, c2 = S.constants(data_range)

    def blur(v):
        v = v[None, None]
        v = Fn.conv3d(Fn.pad(v, (5, 5, 0, 0, 0, 0), mode="replicate"), g.reshape(1, 1, 1, 1, 11))
        v = Fn.conv3d(Fn.pad(v, (0, 0, 5, 5, 0, 0), mode="replicate"), g.reshape(1, 1, 1, 11, 1))
        v = Fn.conv3d(Fn.pad(v, (0, 0, 0, 0, 5, 5), mode="replicate"), g.reshape(1, 1, 11, 1, 1))
        return v[0, 0]

    def down(v):
        d, h, w = v.shape
        v = Fn.pad(v[None, None], (0, w % 2, 0, h % 2, 0, d % 2), mode="replicate")
        return Fn.avg_pool3d(v, 2)[0, 0]
    ta = torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    tb = torch.tensor(np.asarray(b, np.float64), requires_grad=True)
    pa, pb, means, value = ta, tb, [], 1.0
    for s in range(scales):
        if s:
            pa, pb = down(pa), down(pb)
        ma, mb = blur(pa), blur(pb)
        s_aa, s_bb, s_ab = blur(pa * pa) - ma * ma, blur(pb * pb) - mb * mb, blur(pa * pb) - ma * mb
        cs = (2 * s_ab + c2) / (s_aa + s_bb + c2)
        ssim = (2 * ma * mb + c1) / (ma * ma + mb * mb + c1) * cs
        n = float(pa.numel())
        mcs, mssim = cs.sum() / n, ssim.sum() / n
        means.append((float(mcs.detach()), float(mssim.detach())))
        if weights[s] != 0.0:
            value = value * torch.relu(mssim if s == scales - 1 else mcs) ** weights[s]
    (g_out * value).backward()
    return float(value.detach()), np.array(means), ta.grad.numpy(), tb.grad.numpy()


@pytest.mark.parametrize("size", [(9, 7, 5), (16, 11, 6)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("scales", [3, 5])
def test_model_is_the_torch_restatement(size, scales):
    w, h, d = size
    rng = np.random.default_rng(w * 100 + h * 10 + d)
    a = rng.random((d, h, w)).astype(np.float32)
    b = np.clip(a + 0.1 * rng.standard_normal((d, h, w)), 0, 1).astype(np.float32)
    wts = M.WANG_WEIGHTS if scales == 5 else (0.2, 0.3, 0.5)
    for r, sa, sb in ((1.0, a, b), (255.0, a * np.float32(255), b * np.float32(255))):
        mod = M.Model(sa, sb, r)
        value, means = mod.msssim(scales, wts)
        da, db = mod.grad(-0.75, scales, wts)
        tv, tm, tda, tdb = _torch_restatement(sa, sb, r, scales, wts, -0.75)
        assert abs(value - tv) <= 1e-9 and np.abs(means - tm).max() <= 1e-9, (size, r, value, tv)
        assert np.abs(da - tda).max() <= 1e-9 and np.abs(db - tdb).max() <= 1e-9, (size, r)
        assert np.abs(tda).max() > 1e-6 / r                      # a gradient worth comparing


def test_one_scale_of_weight_one_is_the_ssim3f_model():
    a, b = C.random_pair((9, 14, 21), 3)
    v, means = M.msssim(a, b, 1.0, 1, (1.0,))
    want, _ = S.ssim(a, b, 1.0)
    assert v == want and means[0][1] == want
    ga, gb = M.grad(a, b, 1.0, -0.75, 1, (1.0,))
    wa, wb = S.grad(a, b, 1.0, -0.75)
    # the value and the mean are the same doubles; the gradient is k * Gt(d) here and Gt(k * d) there, with k = ((g m) / m) / voxels
    # against g / voxels: the same number up to the last bits of a double, as tests/test_msssimf_cpu.py holds the 2-D pair
    assert np.abs(ga - wa).max() <= 1e-12 * np.abs(wa).max() and np.abs(gb - wb).max() <= 1e-12 * np.abs(wb).max()


def test_downsample_t_is_the_adjoint_of_downsample():
    rng = np.random.default_rng(17)
    for shape in [(6, 8, 10), (7, 8, 10), (6, 9, 11), (5, 3, 1), (1, 1, 1), (1, 1, 9), (2, 2, 2), (3, 3, 3), (1000, 3, 5)]:
        u = rng.standard_normal(shape)
        d = M.downsample(u)
        assert d.shape == tuple((n + 1) // 2 for n in shape)
        v = rng.standard_normal(d.shape)
        lhs, rhs = float(np.sum(d * v)), float(np.sum(u * M.downsample_t(v, shape)))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-3), (shape, lhs, rhs)
        # the gather form of the definition: 0.125 c(x, y, z) v(x >> 1, y >> 1, z >> 1)
        cz, cy, cx = (M.box_adjoint_weight(n) for n in shape)
        gather = 0.125 * cz[:, None, None] * cy[None, :, None] * cx[None, None, :] * v[np.ix_(*(np.arange(n) >> 1 for n in shape))]
        assert np.abs(gather - M.downsample_t(v, shape)).max() <= 1e-15
    assert [tuple(d) for d in M.scale_dims(5, 3, 1000, 4)] == [(5, 3, 1000), (3, 2, 500), (2, 1, 250), (1, 1, 125)]
    assert M.downsample(np.arange(24, dtype=np.float32).reshape(2, 3, 4)).dtype == np.float32


def test_fp32_emulation_leaves_the_pinned_figures(manifest):
    """Emulation against the float64 model over ssim3f_model.FIXTURES x FORMS x {Wang's five scales, uniform weights at 1 .. 8 scales};
    every fixture's A against itself for the identical pair.  Measured: 5.52e-6 on the value, 6.39e-6 on a per-scale mean, 9.45e-5 of the
    volume's largest float64 gradient magnitude, 4.06e-4 for max|grad| * W * H * D * R on identical volumes.  tests/test_gpu_msssim3f.py
    asserts TOL_FACTOR = 2 times msssim3f_model.EMU_*."""
    got = M.measure(manifest)
    print("emulation: value %.3g mean %.3g grad %.3g identical %.3g" % got)
    assert M.TOL_FACTOR == 2.0
    for v, emu, tol in zip(got, (M.EMU_VALUE, M.EMU_MEAN, M.EMU_GRAD, M.EMU_IDENT), M.tolerances()):
        assert v <= emu, (got, emu)
        # pinned from below as well: a figure that moved far away means the emulation no longer restates these kernels
        assert v >= emu / 2, (got, emu)
        assert tol == 2.0 * emu


def test_emulation_restates_the_pyramid_order_the_centres_and_the_accumulation():
    rng = np.random.default_rng(3)
    a = (rng.random((5, 7, 30)) * 1000).astype(np.float32)
    b = (rng.random((5, 7, 30)) * 1000).astype(np.float32)
    emu = M.Emulation(a, b, 1000.0)
    s1 = emu.scale(1)
    # fp32 in the defined order; the last slice and row of odd axes are read twice
    lo = (a[4, 6, 0] + a[4, 6, 1]) + (a[4, 6, 0] + a[4, 6, 1])
    want = (lo + lo) * np.float32(0.125)
    assert s1.a.dtype == np.float32 and s1.a.shape == (3, 4, 15) and s1.a[2, 3, 0] == want
    x = ((a[0, 0, 2] + a[0, 0, 3]) + (a[0, 1, 2] + a[0, 1, 3])) + ((a[1, 0, 2] + a[1, 0, 3]) + (a[1, 1, 2] + a[1, 1, 3]))
    assert s1.a[0, 0, 1] == x * np.float32(0.125)
    # the centre of scale 1 comes from scale 1's own volume
    assert S.centre(s1.a, 1000.0) == s1.a[1, 1, 7]
    # a scale whose coefficient is 0 contributes +0, and the coarser gradient arrives through 0.125 c g(x >> 1, y >> 1, z >> 1)
    ga, _ = emu.grad(1.0, 2, (0.0, 1.0))
    k1 = np.float32(M.coefficients(emu.means(2), (0.0, 1.0), 1.0, [(5, 7, 30), (3, 4, 15)])[1])
    up, _ = s1.local(k1, True)
    assert ga[1, 2, 20] == np.float32(0.125) * up[0, 1, 10] and ga[4, 6, 29] == np.float32(0.5) * up[2, 3, 14]
    assert ga[4, 2, 3] == np.float32(0.25) * up[2, 1, 1]
    # gOut = 0: every coefficient is 0 even when a mean is NaN
    assert M.coefficients(np.full((2, 2), np.nan), (0.5, 0.5), 0.0, [(5, 7, 30), (3, 4, 15)]) == [0.0, 0.0]


# ---- the inputs of the GPU module ---------------------------------------------------------------------------------------------------------------

def _lowest_mean(means, weights):
    n = len(weights)
    return min(float(means[s][1] if s == n - 1 else means[s][0]) for s in range(n) if weights[s] > 0)


def test_accuracy_inputs_keep_every_weighted_mean_away_from_zero(manifest):
    """The gradient bound divides by m_s: every m_s with w_s > 0 of every accuracy input is at least 0.2 in the float64 model.  The golden
    volumes give at least 0.56 at all five scales, content_classes.random_pair at least 0.79 on the shapes the GPU module uses."""
    lowest = 9.0
    for name in S.FIXTURES:
        for _, fa, fb, r in S.fixture_forms(manifest, name):
            lowest = min(lowest, _lowest_mean(M.Model(fa, fb, r).means(5), M.WANG_WEIGHTS))
    print("golden volumes: lowest weighted mean %.3f" % lowest)
    assert lowest >= 0.56
    _, fa, fb, r = S.fixture_forms(manifest, "bbb257x65_q50_ch1")[0]
    assert min(_lowest_mean(M.Model(fa, fb, r).means(n), uniform(n)) for n in range(1, 9)) >= 0.2
    for shape, scales in (((44, 21, 37), 8), ((13, 20, 33), 5), ((131, 17, 17), 3), ((1000, 3, 5), 4), ((9, 17, 17), 5)):
        a, b = C.random_pair(shape, 1)
        low = _lowest_mean(M.Model(a, b, 1.0).means(scales), uniform(scales))
        print("random pair %r at %d scales: lowest weighted mean %.3f" % (shape, scales, low))
        assert low >= 0.79


def test_content_classes_leave_the_emulation_within_85_percent():
    """The finite classes of content_classes.volume_classes((12, 19, 40), 1.0) other than the two `huge centre sample` classes, at 4
    scales with uniform weights.  `anticorrelated` has negative mcs: the ReLU case, value 0 and gradient 0.  Every other class must leave
    the emulation within 85 % of the EMU figures (the catalogue's own rule) and keep m_s >= 0.2; the two that do not are DROPPED from the
    GPU accuracy test, each named there with its emulated figures."""
    sets = [(4, uniform(4))]
    over = []
    for name, a, b, r, _ in C.volume_classes((12, 19, 40), 1.0):
        if name in C.HUGE_CLASSES or name in C.NONFINITE_CLASSES:
            continue
        mod = M.Model(a, b, r)
        if name == "anticorrelated":
            assert mod.means(4)[0][0] < 0 and mod.msssim(4, uniform(4))[0] == 0.0
            ga, gb = mod.grad(1.0, 4, uniform(4))
            assert not ga.any() and not gb.any()
            ea, eb = M.Emulation(a, b, r).grad(1.0, 4, uniform(4))
            assert not ea.view(np.uint32).any() and not eb.view(np.uint32).any()
            continue
        assert _lowest_mean(mod.means(4), uniform(4)) >= 0.2, name
        if np.array_equal(a, b):
            figs = (0.0, 0.0, M.measure_ident(a, r, sets) / M.EMU_IDENT)
        else:
            v, m, g = M.measure_pair(a, b, r, sets, g_out=-0.75)
            figs = (v / M.EMU_VALUE, m / M.EMU_MEAN, g / M.EMU_GRAD)
        print("%-28s value %.2f mean %.2f gradient %.2f of EMU" % ((name,) + figs))
        if max(figs) > 0.85:
            over.append(name)
    assert sorted(over) == sorted(DROPPED), over


# ---- budgets ------------------------------------------------------------------------------------------------------------------------------------

def test_multi_scale_volume_kernels_never_spill_and_keep_the_budgets():
    """Build-time guard from the compiler's remarks, by the mechanism of tests/test_ssim3hk_cpu.py.  17 kernels: 7 walks (the value walk
    with two sums; dA, dB, both in the cs form and in the ssim form), 6 adjoint walks (A, B, both x coarsest / finer), the pyramid step, the
    reduction, the product, the coefficients.  None uses scratch; every walk keeps 4 waves per SIMD or more (at most 128 VGPRs), the
    one-gradient adjoints 4 or more, the both-gradients adjoints 3 or more (at most 168 VGPRs); LDS stays at the single-scale kernels'
    figures (17472 bytes, plus 64 for the second sum's wave totals)."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "msssim3f_kernels.hip")
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
    walks = {k: v for k, v in kernels.items() if "msssim3f_walk_kernel" in k}
    adjoints = {k: v for k, v in kernels.items() if "msssim3f_adjoint_kernel" in k}
    assert len(walks) == 7 and len(adjoints) == 6 and len(kernels) == 17, sorted(kernels)
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)
        print(k, v)
    for k, v in walks.items():
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 4 and v["LDS"] <= 17472 + 64, (k, v)
    for k, v in adjoints.items():
        both = "ILi3E" in k
        assert v["Occupancy"] >= (3 if both else 4) and v["VGPRs"] <= (168 if both else 128) and v["LDS"] <= 17472, (k, v)


# ---- the scratch rule ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/src/msssim3f_plan_probe.cpp linked against the kernel objects of the library under test (the Makefile's own rule brings them
    up to date: nothing to do after a build)."""
    objects = ["build/obj/msssim3f_kernels.o", "build/obj/ssim3f_kernels.o"]
    r = subprocess.run(["make", "-C", ROOT] + objects, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path_factory.mktemp("msssim3f_plan_probe")
    obj, exe = str(out / "probe.o"), str(out / "probe")
    src = os.path.join(ROOT, "tests", "src", "msssim3f_plan_probe.cpp")
    for cmd in ([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                 "-I" + os.path.join(ROOT, "ssim_amd", "csrc"), "-c", src, "-o", obj],
                [HIPCC, "--offload-arch=gfx950", obj] + [os.path.join(ROOT, o) for o in objects] + ["-o", exe]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]

    def run(rows):
        """rows: (W, H, D, scales, cap) -> one tuple of ints per row."""
        r = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % row for row in rows), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    return run


def test_scratch_and_sub_batches_are_the_restatement(probe):
    rows = [(96, 96, 96, 2, MP.SCRATCH_CAP), (64, 64, 64, 5, MP.SCRATCH_CAP), (37, 21, 44, 8, MP.SCRATCH_CAP), (17, 17, 131, 3, MP.SCRATCH_CAP),
            (5, 3, 1000, 4, MP.SCRATCH_CAP), (1, 1, 1, 8, MP.SCRATCH_CAP), (256, 256, 256, 5, MP.SCRATCH_CAP),
            (512, 512, 512, 5, MP.SCRATCH_CAP),                                       # one volume larger than the cap: sub-batches of one
            (40, 36, 20, 5, 1 << 20), (33, 20, 13, 1, 1 << 16), (2048, 2048, 2048, 2, MP.SCRATCH_CAP), (0x7FFF0000, 1, 1, 3, MP.SCRATCH_CAP),
            (4096, 4096, 4096, 3, MP.SCRATCH_CAP)]
    got = probe(rows)
    assert len(got) == len(rows)
    for (w, h, d, scales, cap), g in zip(rows, got):
        want = (MP.max_count(w, h, d), MP.pyramid_floats(w, h, d, scales), sum(MP.cells(w, h, d, s) for s in range(scales)) * 2)
        want += tuple(MP.scratch_bytes(w, h, d, scales, p) for p in (0, 1, 2))
        want += tuple(MP.per_sub_batch(w, h, d, scales, p, cap) for p in (0, 1, 2))
        assert g == want, ((w, h, d, scales, cap), g, want)
    # what the header states: about 8/7 bytes of pyramid per scale-0 voxel of a pair, 4/7 more per coarse gradient, 12 / 16 per voxel of
    # coefficients; a 512^3 volume is larger than the cap for the backward and runs alone
    v = 256 ** 3
    assert abs(2 * 4 * MP.pyramid_floats(256, 256, 256, 8) / v - 8 / 7) < 1e-3
    assert MP.scratch_bytes(256, 256, 256, 5, 1) - MP.scratch_bytes(256, 256, 256, 5, 0) > 12 * v
    assert MP.scratch_bytes(512, 512, 512, 5, 2) > MP.SCRATCH_CAP and MP.per_sub_batch(512, 512, 512, 5, 2) == 1
    assert MP.sub_batches(512, 512, 512, 5, 2, 3) == [(0, 1), (1, 1), (2, 1)]
    assert MP.per_sub_batch(96, 96, 96, 2, 2) == 67 and MP.sub_batches(96, 96, 96, 2, 2, 68) == [(0, 67), (67, 1)]
    assert MP.max_count(4096, 4096, 4096) == 0                                       # the first pyramid step alone needs 2^32 work-items
