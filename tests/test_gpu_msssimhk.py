"""GPU: multi-scale SSIM of float16 / bfloat16 samples under a caller-chosen window and its gradient (rmgr_ssim_hip_enqueue_msssimh_win,
rmgr_ssim_hip_compute_msssimh_win_device / _host, rmgr_ssim_hip_enqueue_msssimh_win_grad) held to the float32 windowed path, bit for bit.

The contract (include/rmgr/ssim-hip.h): the value and every per-scale mean are those of the msssimf_win entry on the samples widened to
float32 under the same window, and the gradient is the float32 value that entry's gradient would store at scale 0, rounded once, to
nearest-even, into the samples' encoding.  Both widenings are exact, so there is no tolerance and no float64 model here: the reference is
always msssimf_win run in the same test on the widened planes, and tests/halfmodel.py's rounding.  NaN is compared as NaN, never by
payload.
"""
import numpy as np
import pytest

import halfmodel as HM
import msssimk_inputs as IN
import ssimk_model as SK
import ssim_amd
from msssimk_inputs import DevicePairs, mk, same

pytestmark = pytest.mark.gpu

ENC = pytest.mark.parametrize("enc", HM.ENCODINGS)
BY_WINDOW = pytest.mark.parametrize("window", SK.WINDOWS, ids=SK.name_of)
SIZES = [(1, 1), (3, 5), (17, 33), (65, 257), (7, 300)]                 # (H, W): odd at every scale, several strip columns and tiles
CONFIGS = ((5, None), (1, (1.0,)), (3, (0.0, 0.5, 0.5)), (8, (0.125,) * 8))     # k_0 == 0 in the third: scale 0 stores the rounded upstream


def encoded_pair(fa, fb, enc):
    """float32 planes -> (bit patterns of the encoding, the float32 planes those stand for)."""
    ua, ub = HM.round_to(fa, enc), HM.round_to(fb, enc)
    return (ua, ub), (HM.widen(ua, enc), HM.widen(ub, enc))


def random_pair(h, w, rng, enc):
    return encoded_pair(*IN.random_pair(h, w, rng), enc=enc)


def check_pairs(ctx, u_pairs, f_pairs, enc, window, r, g_out, scales, weights, what):
    """Value, means, dA alone, dB alone and both of the bit patterns against msssimf_win on the widened planes.  Returns (both, the
    float32 reference gradients)."""
    win = mk(window)
    ref = DevicePairs(ctx, f_pairs, "f")
    wv, wm = ref.forward(r, win, scales, weights)
    g32 = ref.grads(r, win, g_out, scales, weights)
    ref.free()
    dp = DevicePairs(ctx, u_pairs, enc)
    v, m = dp.forward(r, win, scales, weights)
    both = dp.grads(r, win, g_out, scales, weights)
    only_a = dp.grads(r, win, g_out, scales, weights, want_b=False)
    only_b = dp.grads(r, win, g_out, scales, weights, want_a=False)
    dv, dm = dp.device(r, win, scales, weights)
    dp.free()
    assert same(v, wv) and same(m, wm), (what, enc, window, scales, v, wv)
    assert same(dv, wv.astype(np.float32)) and same(dm, wm), (what, enc, window, scales)
    for i in range(len(u_pairs)):
        for k in range(2):
            assert HM.same(both[i][k], HM.round_to(g32[i][k], enc), enc), (what, enc, window, scales, i, k)
        assert only_a[i][1] is None and only_b[i][0] is None
        assert HM.same(only_a[i][0], both[i][0], enc) and HM.same(only_b[i][1], both[i][1], enc), (what, enc, window, scales, i)
    return both, g32


@ENC
@BY_WINDOW
def test_every_window_at_odd_sizes_down_to_one_pixel(gpu_ctx, enc, window):
    rng = np.random.default_rng(41)
    for (h, w) in SIZES:
        u, f = random_pair(h, w, rng, enc)
        for scales, wts in CONFIGS:
            both, _ = check_pairs(gpu_ctx, [u], [f], enc, window, 1.0, [float(w * h)], scales, wts, "%dx%d" % (w, h))
            assert not HM.is_nan(both[0][0], enc).any()


@ENC
@pytest.mark.parametrize("window", [IN.BOX3, IN.G9], ids=SK.name_of)
def test_a_batch_and_the_host_entry(gpu_ctx, enc, window):
    rng = np.random.default_rng(43)
    pairs = [random_pair(40, 300, rng, enc) for _ in range(3)]
    u, f = [p[0] for p in pairs], [p[1] for p in pairs]
    check_pairs(gpu_ctx, u, f, enc, window, 1.0, [1200.0, 0.0, -600.0], 4, (0.25,) * 4, "batch of 3")
    hosts = [(HM.host_array(x[0], enc)[0], HM.host_array(x[1], enc)[0]) for x in u]
    st = HM.host_array(u[0][0], enc)[1]
    hv, hm = ssim_amd.compute_msssimh_batch(hosts, 1.0, sample_type=st, scales=4, weights=(0.25,) * 4, per_scale=True, window=mk(window))
    fv, fm = ssim_amd.compute_msssimf_batch(f, 1.0, 4, (0.25,) * 4, per_scale=True, window=mk(window))
    assert same(hv, fv) and same(hm, fm)


@ENC
def test_null_and_the_engines_window_give_the_bits_of_msssimh(gpu_ctx, enc):
    import ctypes
    ctx, lib = gpu_ctx, gpu_ctx.lib
    u, _ = random_pair(65, 257, np.random.default_rng(45), enc)
    dp = DevicePairs(ctx, [u], enc)
    v0, m0 = dp.forward(1.0, None)
    g0 = dp.grads(1.0, None, [500.0])[0]
    engine = mk(SK.DEFAULT)
    v1, m1 = dp.forward(1.0, engine)
    g1 = dp.grads(1.0, engine, [500.0])[0]
    assert same(v1, v0) and same(m1, m0) and HM.same(g1[0], g0[0], enc) and HM.same(g1[1], g0[1], enc)
    vals, means, go = ctx.alloc(8), ctx.alloc(80), ctx.upload(np.float32([500.0]))
    arrs, bufs, fill = dp.grad_planes()
    code = ssim_amd.sample_type_code(enc)
    assert lib.rmgr_ssim_hip_enqueue_msssimh_win(ctx.handle, 1, dp.params, code, 1.0, None, 5, None, vals.ptr, means.ptr) == 0
    assert lib.rmgr_ssim_hip_enqueue_msssimh_win_grad(ctx.handle, 1, dp.params, code, 1.0, None, 5, None, means.ptr, go.ptr, arrs[0], arrs[1]) == 0
    ctx.synchronize()
    assert same(vals.download(np.float64, (1,)), v0) and same(means.download(np.float64, (1, 5, 2)), m0)
    g2 = dp.collect(arrs, bufs, fill)[0]
    assert HM.same(g2[0], g0[0], enc) and HM.same(g2[1], g0[1], enc)
    out = (ctypes.c_float * 1)()
    assert lib.rmgr_ssim_hip_compute_msssimh_win_device(ctx.handle, 1, dp.params, code, 1.0, None, 5, None, out, None) == 0
    assert np.float32(out[0]) == np.float32(v0[0])
    for x in (vals, means, go):
        x.free()
    dp.free()


@ENC
@pytest.mark.parametrize("window", [IN.BOX3, (7, 1.5, "gaussian")], ids=SK.name_of)
def test_one_strided_view(gpu_ctx, enc, window):
    """Samples three elements apart, five elements into their buffers; gradient planes two apart, three in: the bits of the dense call."""
    win = mk(window)
    u, _ = random_pair(33, 140, np.random.default_rng(47), enc)
    dense = DevicePairs(gpu_ctx, [u], enc)
    v, m = dense.forward(1.0, win)
    g = dense.grads(1.0, win, [3000.0])[0]
    dense.free()
    view = DevicePairs(gpu_ctx, [u], enc, step=3, lead=5)
    v2, m2 = view.forward(1.0, win)
    g2 = view.grads(1.0, win, [3000.0], gstep=2, lead=3)[0]
    view.free()
    assert same(v2, v) and same(m2, m) and HM.same(g2[0], g[0], enc) and HM.same(g2[1], g[1], enc)


@ENC
@pytest.mark.parametrize("window", IN.PER_RADIUS[:4], ids=SK.name_of)
def test_64_bit_form_with_samples_far_apart(gpu_ctx, enc, window):
    """One 9 x 5 (H x W) pair at 2 scales with samples 2^22 two-byte elements apart -- the first step fitsh_narrow() refuses --, read with
    a negative step: the bits of the dense call, which has those of msssimf_win, and nothing but the gradient planes written."""
    win = mk(window)
    u, f = random_pair(9, 5, np.random.default_rng(33), enc)
    g_out, scales, wts = [45.0], 2, (0.4, 0.6)
    both, _ = check_pairs(gpu_ctx, [u], [f], enc, window, 1.0, g_out, scales, wts, "dense 5x9")
    dense = DevicePairs(gpu_ctx, [u], enc)
    v, m = dense.forward(1.0, win, scales, wts)
    dense.free()
    fv, fm, da, db, untouched = IN.far_apart_call(gpu_ctx, enc, u, 1 << 22, -1, 1.0, win, g_out, scales, wts, np.uint16(0x7FC0))
    assert same(fv, v) and same(fm, m) and HM.same(da, both[0][0], enc) and HM.same(db, both[0][1], enc) and untouched


@pytest.mark.parametrize("window", [IN.BOX3, IN.G9], ids=SK.name_of)
def test_float16_gradient_rounds_into_subnormals_and_overflows_under_a_loss_scale(gpu_ctx, window):
    """gOut carries the loss scale and stays float32: scaled down, the float16 gradient lands among the subnormals (kept, not flushed);
    scaled up, it overflows to Inf -- in both cases the float32 gradient rounded once."""
    u, f = random_pair(40, 140, np.random.default_rng(49), HM.F16)
    n = 40.0 * 140.0
    small, _ = check_pairs(gpu_ctx, [u], [f], HM.F16, window, 1.0, [n * 2.0 ** -20], 3, (0.3, 0.3, 0.4), "scaled down")
    sub = HM.is_subnormal(small[0][0], HM.F16)
    assert sub.any() and (small[0][0] & 0x7FFF).any()
    big, g32 = check_pairs(gpu_ctx, [u], [f], HM.F16, window, 1.0, [n * 2.0 ** 24], 3, (0.3, 0.3, 0.4), "scaled up")
    inf = (big[0][0] & 0x7FFF) == 0x7C00
    assert inf.any() and np.all(np.isfinite(g32[0][0])) and np.array_equal(inf, np.abs(g32[0][0]) >= 65520.0)
