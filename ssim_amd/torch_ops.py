"""SSIM and multi-scale SSIM of float32, float16 and bfloat16 tensors as differentiable PyTorch operations, on the library's fused gfx950
kernels.

    from ssim_amd.torch_ops import ssim, ssim_map, ssim_amp, ssim_map_amp, SSIMLoss, ms_ssim, ms_ssim_amp, MSSSIMLoss
    loss = 0.8 * (x - y).abs().mean() + 0.2 * SSIMLoss()(x, y)      # x, y: (N, C, H, W) float32 on the GPU
    loss = 0.16 * (x - y).abs().mean() + 0.84 * MSSSIMLoss()(x, y)
    loss.backward()

ssim(x, y, data_range) is the per-plane mean of the definition in include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_ssimf); its backward is
rmgr_ssim_hip_enqueue_ssimf_grad; ms_ssim(x, y, data_range, scales, weights) is rmgr_ssim_hip_enqueue_msssimf and its backward
rmgr_ssim_hip_enqueue_msssimf_grad.  Everything is enqueued on torch.cuda.current_stream() of the tensors' device through a Context cached
per (device, stream); neither forward nor backward waits for the host.  There is no eager fall-back: without the library this raises.

float16 and bfloat16.  x and y both float16 or both bfloat16 run rmgr_ssim_hip_enqueue_ssimh and its backward
rmgr_ssim_hip_enqueue_ssimh_grad (ms_ssim_amp and MSSSIMLoss: rmgr_ssim_hip_enqueue_msssimh and _msssimh_grad): the samples are read as
they are (2 B/px), the result is float32 per plane at every input dtype (a loss of 1 - 0.98 has no business in 8 significant bits), and
the gradient comes back in the inputs' dtype, written by the kernel into a 2 B/px tensor with one rounding and no float32 intermediate.  Two things to know:
  * inside torch.autocast the function takes its tensors as they come and is not itself autocast: a conv's bfloat16 output is read as
    bfloat16, a float32 tensor as float32, and a mixed pair is a TypeError, not a silent cast;
  * with float16 the gradient of a mean SSIM is of order 1 / (W H) and underflows without torch.amp.GradScaler.  With a scaled loss
    the scale arrives in grad_out, which stays float32, and is applied before the single rounding: the result is round(scale * g), not
    scale * round(g).
ms_ssim_amp and MSSSIMLoss take 16-bit tensors the same way: only scale 0 holds 16-bit samples (the pyramid is float32 from scale 1 on),
the value has the bits of ms_ssim(x.float(), y.float()) and the gradient is that call's float32 gradient rounded once.  Two warts, both
pinned by tests from the time there was no 16-bit multi-scale path: ms_ssim itself stays float32-only (16-bit tensors are a TypeError
there; ms_ssim_amp is the same function without that refusal), and two 16-bit CPU tensors are a TypeError in ms_ssim_amp and MSSSIMLoss
(ssim: a ValueError, like every CPU tensor).

The map.  ssim_map(x, y, data_range) returns the per-pixel SSIM, float32 of shape x.shape, for losses that are not a plain mean per plane.
The forward is the same kernel writing its map; the backward is rmgr_ssim_hip_enqueue_ssimf_map_grad / _ssimh_map_grad, the fused gradient
kernel with the upstream gradient read per pixel, in place through grad_out's own strides (the expanded zero-stride tensor that sum()
hands back is one float, not a plane).  It saves x and y only.

    m = ssim_map(x, y)                                              # (N, C, H, W), float32
    loss = 1 - (w * m).sum() / w.sum()                              # a validity mask or a saliency weight w
    photo = 0.85 * (1 - ssim_map(warped, target)) / 2 + 0.15 * (warped - target).abs()      # monodepth-style, warped: (V, N, C, H, W)
    loss = (auto_mask * photo.mean(2).min(0).values).mean()         # per-pixel minimum over the V source views, then the auto-mask

A zero weight does not hide a NaN: 0 * NaN is NaN, and the gradient of the pixels around it is NaN too.  Replace invalid samples in x and
y, not only in the weights.

The window.  ssim, ssim_map and SSIMLoss take win_size (3, 5, 7, 9 or 11), win_sigma and window ("gaussian" or "uniform", a box that
ignores win_sigma): pytorch-msssim's win_size / win_sigma, torchmetrics' and piq's kernel_size / sigma, TensorFlow's filter_size /
filter_sigma, kornia's window_size, skimage's 7 x 7 box, the 3 x 3 box of monodepth-style losses.  The defaults (11, 1.5, "gaussian") take
exactly the path above; anything else runs the _win entries of the float32 family (rmgr_ssim_hip_enqueue_ssimf_win, _ssimf_win_grad,
_ssimf_win_map_grad), the small windows on kernels of their own radius.  Edges are clamped for every window: where monodepth-style code
reflects, the interior is identical and the outermost (win_size - 1) / 2 pixels differ.  ms_ssim, ms_ssim_amp and MSSSIMLoss take the same three keywords, at every dtype their
tensors may have: one window for every scale (the msssimf_win and msssimh_win entries).

    photo = 0.85 * (1 - ssim_map(warped, target, win_size=3, window="uniform")) / 2 + 0.15 * (warped - target).abs()

The window with float16 / bfloat16 tensors.  ssim_amp(x, y, data_range, win_size, win_sigma, window), ssim_map_amp(...) and SSIMLoss on
GPU tensors take the window keywords with 16-bit tensors as well (rmgr_ssim_hip_enqueue_ssimh_win, _ssimh_win_grad, _ssimh_win_map_grad):
the value and the map have the bits of ssim(x.float(), y.float(), win_size=...) / ssim_map(...), and the gradient is that call's float32
gradient rounded once by the kernel into the inputs' dtype -- 2 B/px of torch memory for it instead of the 4 + 4 + 4 of x.float(),
y.float() and a float32 gradient.  float32 pairs and the default keywords take exactly the path of ssim / ssim_map.  The wart of
ms_ssim / ms_ssim_amp again: ssim and ssim_map themselves refuse a non-default window with 16-bit tensors (a TypeError, "fixed window",
pinned by tests from the time there was no such path; the _amp functions are the same functions without that refusal), and SSIMLoss is
pinned the same way on CPU tensors: it is 1 - ssim_amp(x, y) when both tensors are on a GPU and raises what ssim raises otherwise, so
two 16-bit CPU tensors under a window still say "fixed window" where every other CPU pair is the "GPU" ValueError.

    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = SSIMLoss(win_size=7)(net(x), y.bfloat16())              # read as bfloat16; the gradient is bfloat16
        photo = 0.85 * (1 - ssim_map_amp(warped, target, win_size=3, window="uniform")) / 2 + 0.15 * (warped - target).abs()

Volumes.  ssim3d(x, y, data_range) and SSIM3DLoss take (..., D, H, W) float32 tensors and apply the window over x, y and z
(rmgr_ssim_hip_enqueue_ssim3f, _ssim3f_grad): the 3-D SSIM of pytorch-msssim (spatial_dims=3), torchmetrics, MONAI and skimage.  ssim() on
a 5-D tensor keeps its meaning -- one 2-D SSIM per slice --; the end of this file has the rest.

    loss = SSIM3DLoss()(x, y)                                       # x, y: (N, C, D, H, W) float32 on the GPU

ssim3d_map(x, y, data_range) is the per-voxel map of the same definition, float32 of shape x.shape, for losses that are not a plain mean
per volume; its backward is rmgr_ssim_hip_enqueue_ssim3f_map_grad, which reads grad_out per voxel, in place.

    m = ssim3d_map(x, y)                                            # (N, C, D, H, W), float32
    loss = 1 - (mask * m).sum() / mask.sum()                        # SSIM inside a brain or body mask

float16 and bfloat16 volumes.  ssim3d_amp(x, y, data_range), ssim3d_map_amp(x, y, data_range) and SSIM3DLoss take two float32, two
float16 or two bfloat16 tensors as they come under torch.autocast (rmgr_ssim_hip_enqueue_ssim3h, _ssim3h_grad, _ssim3h_map_grad): the
samples are read as they are (2 B/voxel), the value and the map are float32 with the bits of ssim3d(x.float(), y.float()) /
ssim3d_map(x.float(), y.float()), and the gradient comes back in the inputs' dtype, that call's float32 gradient rounded once by the
kernel; grad_out stays float32, so a GradScaler's scale arrives before the rounding.  They take the window keywords with 16-bit tensors
as well (rmgr_ssim_hip_enqueue_ssim3h_win, _ssim3h_win_grad, _ssim3h_win_map_grad): the bits of ssim3d(x.float(), y.float(), win_size=...)
and that call's gradient rounded once, without the float32 copies.  The wart of ms_ssim / ms_ssim_amp again: ssim3d and
ssim3d_map themselves stay float32-only (16-bit tensors are a TypeError there, pinned by tests from the time there was no 16-bit volume
path; the _amp functions are the same functions without that refusal), and two 16-bit CPU tensors are a TypeError in the _amp functions
and SSIM3DLoss.

    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = SSIM3DLoss()(net(x), y.bfloat16())                   # read as bfloat16; the gradient is bfloat16
        loss = SSIM3DLoss(win_size=7, window="uniform")(net(x), y.bfloat16())      # MONAI's / skimage's 7-tap box, still 2 B/voxel

Multi-scale SSIM of volumes.  ms_ssim3d(x, y, data_range, scales, weights) and MSSSIM3DLoss take (..., D, H, W) float32 tensors
(rmgr_ssim_hip_enqueue_msssim3f, _msssim3f_grad): ms_ssim's product over a pyramid that halves all three axes, as pytorch-msssim's
MS_SSIM(spatial_dims=3) does with avg_pool3d.  That one uses a valid window and zero-padded pooling and refuses small sides; this one
clamps the window and the pooling at the borders and runs down to 1 x 1 x 1, so the values are close, not equal.  The 11-tap window
only for now.  ms_ssim3d_amp(x, y, data_range, scales, weights) and MSSSIM3DLoss take two float16 or two bfloat16 tensors as well
(rmgr_ssim_hip_enqueue_msssim3h, _msssim3h_grad), as ms_ssim_amp and MSSSIMLoss do in 2-D: only scale 0 holds 16-bit samples, the value
has the bits of ms_ssim3d(x.float(), y.float()) and the gradient is that call's float32 gradient rounded once by the kernel, 2 B/voxel of
torch memory for it instead of the 4 + 4 + 4 of x.float(), y.float() and a float32 gradient.  The warts of MSSSIMLoss again, both pinned
by tests from the time there was no 16-bit path: ms_ssim3d itself stays float32-only (16-bit tensors are a TypeError there), and two
16-bit CPU tensors are a TypeError in ms_ssim3d_amp and MSSSIM3DLoss; a third: that TypeError keeps the words "the 3-D multi-scale path is
float32 for now", which the same tests match on MSSSIM3DLoss.

    loss = 0.16 * (x - y).abs().mean() + 0.84 * MSSSIM3DLoss()(x, y)       # x, y: (N, C, D, H, W) float32 on the GPU
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = MSSSIM3DLoss()(net(x), y.bfloat16())                        # read as bfloat16; the gradient is bfloat16

torch is imported on first use, so `import ssim_amd` stays torch-free.
"""
import ctypes
import math

from . import api

_contexts = {}      # (device index, stream handle) -> (Context, the torch stream it is bound to)
_side = {}          # device index -> torch stream that stands in for the legacy default stream
_function = None
_map_function = None
_ms_function = None


def _working_stream(torch, device):
    """(current stream, stream the library's context is bound to).  The legacy default stream has no handle a context could adopt
    (NULL means `create one`), so its work runs on a side stream that waits for it and that it waits for: device-side ordering only."""
    cur = torch.cuda.current_stream(device)
    if cur.cuda_stream != 0:
        return cur, cur
    side = _side.get(device.index)
    if side is None:
        side = _side[device.index] = torch.cuda.Stream(device)
    return cur, side


def _context(device, stream):
    key = (device.index, stream.cuda_stream)
    ent = _contexts.get(key)
    if ent is None:
        ent = _contexts[key] = (api.Context(device.index, ctypes.c_void_p(stream.cuda_stream)), stream)
    return ent[0]


def _sample_type(torch, dtype):
    """None for float32, the library's sample type code for float16 / bfloat16."""
    return {torch.float16: api.SAMPLE_F16, torch.bfloat16: api.SAMPLE_BF16}.get(dtype)


def _check(x, y, data_range, half=False, name="ssim"):
    """The documented errors (`name`: the function the message names), before any GPU call.  Returns data_range as a float.  half: float16
    and bfloat16 pairs are taken too."""
    import torch
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise TypeError("%s: x and y must be torch tensors" % name)
    if half:
        if x.dtype != y.dtype or x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError("%s: two float32, two float16 or two bfloat16 tensors expected, got %s and %s" % (name, x.dtype, y.dtype))
    elif x.dtype != torch.float32 or y.dtype != torch.float32:
        raise TypeError("%s: float32 tensors expected, got %s and %s" % (name, x.dtype, y.dtype))
    if x.dim() < 2:
        raise ValueError("%s: tensors of shape (..., H, W) expected, got %d dimension(s)" % (name, x.dim()))
    if x.shape != y.shape:
        raise ValueError("%s: shapes differ: %s and %s" % (name, tuple(x.shape), tuple(y.shape)))
    if not x.is_cuda or not y.is_cuda:
        raise ValueError("%s: the tensors must be on a GPU (there is no CPU path)" % name)
    if x.device != y.device:
        raise ValueError("%s: the tensors are on different devices: %s and %s" % (name, x.device, y.device))
    if x.shape[-1] == 0 or x.shape[-2] == 0:
        raise ValueError("%s: empty planes: %s" % (name, tuple(x.shape)))
    r = float(data_range)
    if not (r > 0.0) or math.isinf(r):
        raise ValueError("%s: data_range must be finite and > 0, got %r" % (name, data_range))
    return r


def _window(x, y, win_size, win_sigma, window, name="ssim", fixed16=True):
    """The documented errors of the window arguments (`name`: the function the message names), before any GPU call.  Returns None for
    the defaults (today's path) or an api.Window.  fixed16 (the 2-D names): float16 / bfloat16 tensors keep the fixed window; the 3-D
    names and the 2-D _amp names pass False, their 16-bit path takes a window (ssim3d and ssim3d_map go on to refuse the tensors themselves)."""
    if not isinstance(window, str):
        raise TypeError("%s: window must be 'gaussian' or 'uniform', got %s" % (name, type(window).__name__))
    win = api.make_window(win_size, 1.5 if window == "uniform" else win_sigma, window)      # TypeError / ValueError
    if win.size == 11 and win.kind == api.WINDOW_GAUSSIAN and win.sigma == 1.5:
        return None
    for t in (x, y) if fixed16 else ():
        if str(getattr(t, "dtype", "")) in ("torch.float16", "torch.bfloat16"):
            raise TypeError("%s: float16 / bfloat16 tensors keep the fixed window (win_size=11, win_sigma=1.5, window='gaussian'); "
                            "a configurable window needs float32 tensors" % name)
    return win


def _win_kw(win):
    """The keyword that selects a _win entry; none at all for the default window: exactly the call made before windows existed."""
    return {} if win is None else {"window": win}


def _plane_offsets(t):
    """Element offset of every (H, W) plane of t from t.data_ptr(), in the order of t.reshape(-1, H, W)."""
    offs = [0]
    for size, stride in zip(t.shape[:-2], t.stride()[:-2]):
        offs = [o + i * stride for o in offs for i in range(size)]
    return offs


def _params(x, y):
    h, w = x.shape[-2], x.shape[-1]
    ox, oy = _plane_offsets(x), _plane_offsets(y)
    n = len(ox)
    es = x.element_size()                      # 4: ParamsF; 2 (float16, bfloat16): Params16 -- steps and strides count samples in both
    make, params = (api.make_params_f, (api.ParamsF * max(n, 1))()) if es == 4 else (api.make_params16, (api.Params16 * max(n, 1))())
    px, py = x.data_ptr(), y.data_ptr()
    xs, xr, ys, yr = x.stride(-1), x.stride(-2), y.stride(-1), y.stride(-2)
    for i in range(n):
        params[i] = make(w, h, px + es * ox[i], xs, xr, py + es * oy[i], ys, yr)
    return params, n


def _grad_planes(g, n, h, w):
    """GradF (float32) or GradH (float16, bfloat16) array over the n contiguous planes of g."""
    es = g.element_size()
    cls = api.GradF if es == 4 else api.GradH
    arr = (cls * max(n, 1))()
    base = g.data_ptr()
    for i in range(n):
        arr[i] = cls(base + es * i * h * w, 1, w)
    return arr


def _make_function():
    import torch

    class _SSIM(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, data_range, win):
            lead, h, w = x.shape[:-2], x.shape[-2], x.shape[-1]
            params, n = _params(x, y)
            sums = torch.empty(n, dtype=torch.float64, device=x.device)
            if n:
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                if st is None:
                    _context(x.device, work).enqueue_ssimf(params, n, data_range, sums.data_ptr(), **_win_kw(win))
                else:
                    _context(x.device, work).enqueue_ssimh(params, n, data_range, st, sums.data_ptr(), **_win_kw(win))
                if work is not cur:
                    cur.wait_stream(work)
            ctx.save_for_backward(x, y)
            ctx.data_range, ctx.win = data_range, win
            return (sums / (float(w) * float(h))).to(torch.float32).reshape(lead)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            x, y = ctx.saved_tensors
            h, w = x.shape[-2], x.shape[-1]
            want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if not (want_x or want_y):
                return None, None, None, None
            params, n = _params(x, y)
            g = grad_out.to(torch.float32).reshape(-1).contiguous()
            gx = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_x else None     # the inputs' dtype: the kernel rounds once
            gy = torch.empty(y.shape, dtype=y.dtype, device=y.device) if want_y else None
            if n:
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                ga = _grad_planes(gx, n, h, w) if want_x else None
                gb = _grad_planes(gy, n, h, w) if want_y else None
                if st is None:
                    _context(x.device, work).enqueue_ssimf_grad(params, n, ctx.data_range, g.data_ptr(), ga, gb, **_win_kw(ctx.win))
                else:
                    _context(x.device, work).enqueue_ssimh_grad(params, n, ctx.data_range, st, g.data_ptr(), ga, gb, **_win_kw(ctx.win))
                if work is not cur:
                    cur.wait_stream(work)
            return gx, gy, None, None

    return _SSIM


def ssim(x, y, data_range=1.0, win_size=11, win_sigma=1.5, window="gaussian"):
    """Per-plane SSIM of two GPU tensors of identical shape (..., H, W), both float32, both float16 or both bfloat16, any strides (each
    plane is addressed in place, no copy): a float32 tensor of shape x.shape[:-2] at every input dtype.  Differentiable with respect to
    x, y or both; the gradient is computed only for the inputs that need it and has the inputs' dtype (float16 and bfloat16: the
    float32 value rounded once; see the top of this file for autocast and loss scaling).  TypeError: not tensors, mixed dtypes, any
    other dtype.  ValueError: CPU tensors, differing shapes or devices, fewer than 2 dimensions, empty planes, a data_range that is not
    finite and > 0.
    The window: win_size taps per axis (3, 5, 7, 9 or 11), window "gaussian" with win_sigma or "uniform" (a box; win_sigma ignored); the
    defaults are the engine's window and take exactly the path without these arguments.  TypeError: a win_size that is not an int, a
    window that is not a str, a non-default window with float16 / bfloat16 tensors (they keep the fixed window).  ValueError: any other
    win_size, an unknown window name, a win_sigma that is not finite and > 0."""
    global _function
    win = _window(x, y, win_size, win_sigma, window)
    r = _check(x, y, data_range, half=True)
    if _function is None:
        _function = _make_function()
    return _function.apply(x, y, r, win)


def _with_maps(params, n, m, h, w):
    """params with ssimMap pointing at the n contiguous (H, W) planes of the float32 tensor m."""
    base = m.data_ptr()
    for i in range(n):
        params[i].ssimMap, params[i].ssimStep, params[i].ssimStride = base + 4 * i * h * w, 1, w
    return params


def _grad_out_planes(g, n):
    """GradOutF array over the n (H, W) planes of the float32 tensor g, each where it is: any strides, 0 (an expanded tensor) included."""
    arr = (api.GradOutF * max(n, 1))()
    base, step, stride = g.data_ptr(), g.stride(-1), g.stride(-2)
    for i, off in enumerate(_plane_offsets(g)):
        arr[i] = api.GradOutF(base + 4 * off, step, stride)
    return arr


def _make_map_function():
    import torch

    class _SSIMMap(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, data_range, win):
            h, w = x.shape[-2], x.shape[-1]
            params, n = _params(x, y)
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            if n:
                sums = torch.empty(n, dtype=torch.float64, device=x.device)      # the kernel's other output, thrown away; freed into the
                                                                                 # current stream's pool, which waits for the work below
                _with_maps(params, n, out, h, w)
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                if st is None:
                    _context(x.device, work).enqueue_ssimf(params, n, data_range, sums.data_ptr(), **_win_kw(win))
                else:
                    _context(x.device, work).enqueue_ssimh(params, n, data_range, st, sums.data_ptr(), **_win_kw(win))
                if work is not cur:
                    cur.wait_stream(work)
            ctx.save_for_backward(x, y)
            ctx.data_range, ctx.win = data_range, win
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            x, y = ctx.saved_tensors
            h, w = x.shape[-2], x.shape[-1]
            want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if not (want_x or want_y):
                return None, None, None, None
            params, n = _params(x, y)
            g = grad_out if grad_out.dtype == torch.float32 else grad_out.to(torch.float32)      # read in place, through its own strides
            gx = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_x else None     # the inputs' dtype: the kernel rounds once
            gy = torch.empty(y.shape, dtype=y.dtype, device=y.device) if want_y else None
            if n:
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                maps = _grad_out_planes(g, n)
                ga = _grad_planes(gx, n, h, w) if want_x else None
                gb = _grad_planes(gy, n, h, w) if want_y else None
                if st is None:
                    _context(x.device, work).enqueue_ssimf_map_grad(params, n, ctx.data_range, maps, ga, gb, **_win_kw(ctx.win))
                else:
                    _context(x.device, work).enqueue_ssimh_map_grad(params, n, ctx.data_range, st, maps, ga, gb, **_win_kw(ctx.win))
                if work is not cur:
                    cur.wait_stream(work)
            return gx, gy, None, None

    return _SSIMMap


def ssim_map(x, y, data_range=1.0, win_size=11, win_sigma=1.5, window="gaussian"):
    """Per-pixel SSIM of two GPU tensors of identical shape (..., H, W), both float32, both float16 or both bfloat16, any strides (each
    plane is addressed in place, no copy): a float32 tensor of shape x.shape at every input dtype, the map rmgr_ssim_hip_enqueue_ssimf /
    _ssimh write.  Differentiable with respect to x, y or both for ANY upstream gradient: the backward reads grad_out per pixel, in place
    (expanded and non-contiguous tensors included; another dtype is cast to float32 once), computes the gradient only for the inputs
    that need it and returns it in the inputs' dtype (float16 and bfloat16: the float32 value rounded once).  It keeps x and y, not the
    map.  A zero in grad_out does not hide a NaN in the images.  win_size, win_sigma, window: as ssim().  Errors: as ssim()."""
    global _map_function
    win = _window(x, y, win_size, win_sigma, window)
    r = _check(x, y, data_range, half=True)
    if _map_function is None:
        _map_function = _make_map_function()
    return _map_function.apply(x, y, r, win)


def ssim_amp(x, y, data_range=1.0, win_size=11, win_sigma=1.5, window="gaussian"):
    """ssim() for tensors as they come under mixed precision, with the window: ssim() without its refusal of a non-default window for
    float16 / bfloat16 tensors.  float32 pairs, and every pair under the default keywords, take exactly ssim()'s path.  Two float16 or two
    bfloat16 GPU tensors under another window run rmgr_ssim_hip_enqueue_ssimh_win, and the backward rmgr_ssim_hip_enqueue_ssimh_win_grad
    under the window kept on the autograd context: the value has the bits of ssim(x.float(), y.float(), ...) under that window, the
    gradient has the inputs' dtype and is that call's float32 gradient rounded once by the kernel (grad_out stays float32: a GradScaler's
    scale arrives before the rounding).  Every other error is ssim()'s, under this function's name."""
    global _function
    win = _window(x, y, win_size, win_sigma, window, "ssim_amp", fixed16=False)
    r = _check(x, y, data_range, half=True, name="ssim_amp")
    if _function is None:
        _function = _make_function()
    return _function.apply(x, y, r, win)


def ssim_map_amp(x, y, data_range=1.0, win_size=11, win_sigma=1.5, window="gaussian"):
    """ssim_map() without its refusal of a non-default window for float16 / bfloat16 tensors, as ssim_amp() is to ssim(): the map is
    float32 with the bits of ssim_map(x.float(), y.float(), ...) under that window (rmgr_ssim_hip_enqueue_ssimh_win), and the backward
    (rmgr_ssim_hip_enqueue_ssimh_win_map_grad) reads grad_out per pixel, in place, and writes the gradient in the inputs' dtype with one
    rounding.  float32 pairs and the default keywords take exactly ssim_map()'s path.  Every other error is ssim_map()'s, under this
    function's name."""
    global _map_function
    win = _window(x, y, win_size, win_sigma, window, "ssim_map_amp", fixed16=False)
    r = _check(x, y, data_range, half=True, name="ssim_map_amp")
    if _map_function is None:
        _map_function = _make_map_function()
    return _map_function.apply(x, y, r, win)


class SSIMLoss(object):
    """1 - ssim_amp(x, y, data_range): reduction "mean" (a scalar) or "none" (one value per plane), float32 whatever the inputs' dtype
    (float32, float16 or bfloat16).  win_size, win_sigma, window: the window, as ssim(), checked here; GPU tensors take it at every dtype,
    16-bit ones through the rmgr_ssim_hip_*_ssimh_win* entries.  A wart, pinned by tests from the time 16-bit tensors kept the fixed
    window: unless both tensors are on a GPU this raises exactly what ssim() raises, so two float16 / bfloat16 CPU tensors under a
    non-default window are a TypeError that says "fixed window", not the "GPU" ValueError of every other CPU pair.  A plain callable: it
    has no parameters."""

    def __init__(self, data_range=1.0, reduction="mean", win_size=11, win_sigma=1.5, window="gaussian"):
        if reduction not in ("mean", "none"):
            raise ValueError("SSIMLoss: reduction must be 'mean' or 'none', got %r" % (reduction,))
        _window(None, None, win_size, win_sigma, window)
        self.data_range, self.reduction = data_range, reduction
        self.win_size, self.win_sigma, self.window = win_size, win_sigma, window

    def __call__(self, x, y):
        on_gpu = bool(getattr(x, "is_cuda", False)) and bool(getattr(y, "is_cuda", False))
        loss = 1.0 - (ssim_amp if on_gpu else ssim)(x, y, self.data_range, self.win_size, self.win_sigma, self.window)
        return loss.mean() if self.reduction == "mean" else loss


def _check_scales(scales, weights, name="ms_ssim"):
    """The documented errors of ms_ssim's scales and weights (`name`: the function the message names), before any GPU call.  Returns
    (scales, weights as a tuple of floats or None)."""
    if isinstance(scales, bool) or not isinstance(scales, int):
        raise TypeError("%s: scales must be an int, got %r" % (name, scales))
    if not 1 <= scales <= api.MSSSIM_MAX_SCALES:
        raise ValueError("%s: scales must be 1 .. %d, got %d" % (name, api.MSSSIM_MAX_SCALES, scales))
    if weights is None:
        if scales != 5:
            raise ValueError("%s: the default weights are Wang's five: pass %d weights for scales=%d" % (name, scales, scales))
        return scales, None
    w = tuple(float(v) for v in weights)
    if len(w) != scales:
        raise ValueError("%s: %d weights for %d scales" % (name, len(w), scales))
    for v in w:
        if not (v >= 0.0) or math.isinf(v):
            raise ValueError("%s: weights must be finite and >= 0, got %r" % (name, weights))
    return scales, w


def _make_ms_function():
    import torch

    class _MSSSIM(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, data_range, scales, weights, win):
            lead = x.shape[:-2]
            params, n = _params(x, y)
            values = torch.empty(n, dtype=torch.float64, device=x.device)
            means = torch.empty((n, scales, 2), dtype=torch.float64, device=x.device)
            if n:
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                if st is None:
                    _context(x.device, work).enqueue_msssimf(params, n, data_range, values.data_ptr(), means.data_ptr(), scales, weights,
                                                             **_win_kw(win))
                else:
                    _context(x.device, work).enqueue_msssimh(params, n, data_range, st, values.data_ptr(), means.data_ptr(), scales, weights,
                                                             **_win_kw(win))
                if work is not cur:
                    cur.wait_stream(work)
            ctx.save_for_backward(x, y, means)
            ctx.data_range, ctx.scales, ctx.weights, ctx.win = data_range, scales, weights, win
            return values.to(torch.float32).reshape(lead)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            x, y, means = ctx.saved_tensors
            h, w = x.shape[-2], x.shape[-1]
            want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if not (want_x or want_y):
                return None, None, None, None, None, None
            params, n = _params(x, y)
            g = grad_out.to(torch.float32).reshape(-1).contiguous()
            gx = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_x else None     # the inputs' dtype: the kernel rounds once
            gy = torch.empty(y.shape, dtype=y.dtype, device=y.device) if want_y else None
            if n:
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                ga = _grad_planes(gx, n, h, w) if want_x else None
                gb = _grad_planes(gy, n, h, w) if want_y else None
                if st is None:
                    _context(x.device, work).enqueue_msssimf_grad(params, n, ctx.data_range, means.data_ptr(), g.data_ptr(), ga, gb, ctx.scales, ctx.weights,
                                                                  **_win_kw(ctx.win))
                else:
                    _context(x.device, work).enqueue_msssimh_grad(params, n, ctx.data_range, st, means.data_ptr(), g.data_ptr(), ga, gb, ctx.scales,
                                                                  ctx.weights, **_win_kw(ctx.win))
                if work is not cur:
                    cur.wait_stream(work)
            return gx, gy, None, None, None, None

    return _MSSSIM


def _is_half_pair(x, y):
    """Two tensors, both float16 or both bfloat16."""
    import torch
    return isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.dtype == y.dtype and x.dtype in (torch.float16, torch.bfloat16)


def _ms_ssim(x, y, r, scales, weights, win):
    global _ms_function
    scales, w = _check_scales(scales, weights)
    if _ms_function is None:
        _ms_function = _make_ms_function()
    return _ms_function.apply(x, y, r, scales, w, win)


def ms_ssim(x, y, data_range=1.0, scales=5, weights=None, win_size=11, win_sigma=1.5, window="gaussian"):
    """Per-plane multi-scale SSIM of two float32 GPU tensors of identical shape (..., H, W), any strides (each plane is addressed in
    place, no copy): a float32 tensor of shape x.shape[:-2].  weights None: Wang's five (scales must be 5); else `scales` finite weights
    >= 0.  Differentiable with respect to x, y or both; the gradient is computed only for the inputs that need it, from x, y and the
    (planes, scales, 2) float64 per-scale means the forward keeps.  TypeError / ValueError as ssim(), plus ValueError for scales outside
    1 .. 8, a wrong number of weights, a negative or non-finite weight (TypeError: scales is not an int).  float16 and bfloat16 tensors
    are a TypeError here, on any device: tests/tools/ssimh_torch_checks.py and tests/test_ssimh_cpu.py pin that refusal from the time
    there was no 16-bit path.  ms_ssim_amp() and MSSSIMLoss take them.
    The window: win_size, win_sigma and window are ssim()'s keywords with ssim()'s errors, and mean the same window at EVERY scale
    (rmgr_ssim_hip_enqueue_msssimf_win, _msssimf_win_grad; pytorch-msssim's ms_ssim(win_size, win_sigma)); the defaults are the engine's
    window and take exactly the path without these arguments.  Planes smaller than the window at coarse scales clamp."""
    if _is_half_pair(x, y):
        raise TypeError("ms_ssim: float32 tensors expected, got %s; ms_ssim_amp() and MSSSIMLoss take float16 / bfloat16 tensors" % (x.dtype,))
    win = _window(x, y, win_size, win_sigma, window, "ms_ssim", fixed16=False)
    return _ms_ssim(x, y, _check(x, y, data_range), scales, weights, win)


def ms_ssim_amp(x, y, data_range=1.0, scales=5, weights=None, win_size=11, win_sigma=1.5, window="gaussian"):
    """ms_ssim() for tensors as they come under mixed precision: two GPU tensors of identical shape (..., H, W), both float32, both float16
    or both bfloat16, any strides (each plane is addressed in place, no copy or widening): a float32 tensor of shape x.shape[:-2] at every
    input dtype.  float32 tensors: exactly ms_ssim().  float16 and bfloat16: the value has the bits of ms_ssim(x.float(), y.float()),
    the gradient has the inputs' dtype and is that call's float32 gradient rounded once (see the top of this file for autocast and loss
    scaling); saved for the backward are x, y and the float64 means.  Errors: as ms_ssim(), and -- unlike ssim(), where every CPU tensor
    is a ValueError -- two float16 or two bfloat16 CPU tensors are a TypeError: 16-bit tensors are taken on a GPU only (one of the two
    on a GPU: the ValueError).  win_size, win_sigma, window: as ms_ssim(), at every input dtype: with float16 and bfloat16 tensors
    (rmgr_ssim_hip_enqueue_msssimh_win, _msssimh_win_grad) the value has the bits of ms_ssim(x.float(), y.float(), win_size=...) under the
    same window and the gradient is that call's, rounded once."""
    win = _window(x, y, win_size, win_sigma, window, "ms_ssim_amp", fixed16=False)
    if _is_half_pair(x, y) and not x.is_cuda and not y.is_cuda:
        raise TypeError("ms_ssim_amp: float16 / bfloat16 tensors are taken on a GPU only, got %s on %s and %s" % (x.dtype, x.device, y.device))
    return _ms_ssim(x, y, _check(x, y, data_range, half=True), scales, weights, win)


class MSSSIMLoss(object):
    """1 - ms_ssim_amp(x, y, data_range, scales, weights): reduction "mean" (a scalar) or "none" (one value per plane).  A plain callable:
    it has no parameters.  float32, float16 or bfloat16 tensors, as ms_ssim_amp(); the loss is float32 at every input dtype.  win_size,
    win_sigma, window: the window of every scale, as ms_ssim(), checked here; GPU tensors take it at every dtype."""

    def __init__(self, data_range=1.0, scales=5, weights=None, reduction="mean", win_size=11, win_sigma=1.5, window="gaussian"):
        if reduction not in ("mean", "none"):
            raise ValueError("MSSSIMLoss: reduction must be 'mean' or 'none', got %r" % (reduction,))
        _check_scales(scales, weights)
        _window(None, None, win_size, win_sigma, window, "MSSSIMLoss", fixed16=False)
        self.data_range, self.scales, self.weights, self.reduction = data_range, scales, weights, reduction
        self.win_size, self.win_sigma, self.window = win_size, win_sigma, window

    def __call__(self, x, y):
        loss = 1.0 - ms_ssim_amp(x, y, self.data_range, self.scales, self.weights, self.win_size, self.win_sigma, self.window)
        return loss.mean() if self.reduction == "mean" else loss


# ---- volumes: SSIM under the three-dimensional window -----------------------------------------------------------------------------------
# ssim3d(x, y, data_range) is the per-volume mean of the definition in include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_ssim3f): the 11-tap
# Gaussian over x, y AND z, what pytorch-msssim (spatial_dims=3), torchmetrics (5-D input), MONAI (SSIMLoss(spatial_dims=3)) and skimage
# (n-D arrays) compute for volumes.  It has a name of its own because ssim() on an (N, C, D, H, W) tensor already has a meaning: N * C * D
# independent 2-D SSIMs with no window across slices.  The backward is rmgr_ssim_hip_enqueue_ssim3f_grad.  ssim3d and ssim3d_map are
# float32-only; ssim3d_amp and ssim3d_map_amp (the end of the file) take float16 / bfloat16 volumes as well, on the ssim3h entries, through
# the same two autograd functions.
# The window: win_size, win_sigma and window are ssim()'s keywords, checked by the same helper, and mean the same window on all three axes
# (the rmgr_ssim_hip_*_ssim3f_win* entries; what MONAI, torchmetrics and pytorch-msssim call win_size / kernel_size / sigma with
# spatial_dims=3, and skimage's 7-tap box).  The defaults are the engine's window and take exactly the path without these arguments; any
# other window is stored on the autograd context and the backward runs under it -- for float16 / bfloat16 volumes too, on the
# rmgr_ssim_hip_*_ssim3h_win* entries.  The multi-scale form, ms_ssim3d, ms_ssim3d_amp and MSSSIM3DLoss, is at the end of the file: the
# engine's window only.

_function3d = None


def _check3d(x, y, data_range, name="ssim3d", half=False):
    """The documented errors of ssim3d and ssim3d_map (`name`: the one the message names), before any GPU call.  Returns data_range as a
    float.  half (ssim3d_amp, ssim3d_map_amp): float16 and bfloat16 pairs are taken too, on a GPU."""
    import torch
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise TypeError("%s: x and y must be torch tensors" % name)
    if half:
        if x.dtype != y.dtype or x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError("%s: two float32, two float16 or two bfloat16 tensors expected, got %s and %s" % (name, x.dtype, y.dtype))
        if x.dtype != torch.float32 and not x.is_cuda and not y.is_cuda:
            raise TypeError("%s: float16 / bfloat16 tensors are taken on a GPU only, got %s on %s and %s" % (name, x.dtype, x.device, y.device))
    elif x.dtype in (torch.float16, torch.bfloat16) or y.dtype in (torch.float16, torch.bfloat16):
        raise TypeError("%s: the 3-D path is float32 for now, got %s and %s; %s_amp() takes float16 / bfloat16 tensors" % (name, x.dtype, y.dtype, name))
    elif x.dtype != torch.float32 or y.dtype != torch.float32:
        raise TypeError("%s: float32 tensors expected, got %s and %s" % (name, x.dtype, y.dtype))
    if x.dim() < 3:
        raise ValueError("%s: tensors of shape (..., D, H, W) expected, got %d dimension(s)" % (name, x.dim()))
    if x.shape != y.shape:
        raise ValueError("%s: shapes differ: %s and %s" % (name, tuple(x.shape), tuple(y.shape)))
    if not x.is_cuda or not y.is_cuda:
        raise ValueError("%s: the tensors must be on a GPU (there is no CPU path)" % name)
    if x.device != y.device:
        raise ValueError("%s: the tensors are on different devices: %s and %s" % (name, x.device, y.device))
    if x.shape[-1] == 0 or x.shape[-2] == 0 or x.shape[-3] == 0:
        raise ValueError("%s: empty volumes: %s" % (name, tuple(x.shape)))
    r = float(data_range)
    if not (r > 0.0) or math.isinf(r):
        raise ValueError("%s: data_range must be finite and > 0, got %r" % (name, data_range))
    return r


def _volume_offsets(t):
    """Element offset of every (D, H, W) volume of t from t.data_ptr(), in the order of t.reshape(-1, D, H, W)."""
    offs = [0]
    for size, stride in zip(t.shape[:-3], t.stride()[:-3]):
        offs = [o + i * stride for o in offs for i in range(size)]
    return offs


def _params3d(x, y):
    d, h, w = x.shape[-3], x.shape[-2], x.shape[-1]
    ox, oy = _volume_offsets(x), _volume_offsets(y)
    n = len(ox)
    es = x.element_size()                      # 4: Params3F; 2 (float16, bfloat16): Params3H -- steps and strides count samples in both
    make, params = (api.make_params3f, (api.Params3F * max(n, 1))()) if es == 4 else (api.make_params3h, (api.Params3H * max(n, 1))())
    px, py = x.data_ptr(), y.data_ptr()
    sx, sy = (x.stride(-1), x.stride(-2), x.stride(-3)), (y.stride(-1), y.stride(-2), y.stride(-3))
    for i in range(n):
        params[i] = make(w, h, d, px + es * ox[i], sx, py + es * oy[i], sy)
    return params, n


def _grad_volumes(g, n, d, h, w):
    """Grad3F (float32) or Grad3H (float16, bfloat16) array over the n contiguous volumes of g."""
    es = g.element_size()
    cls = api.Grad3F if es == 4 else api.Grad3H
    arr = (cls * max(n, 1))()
    base = g.data_ptr()
    for i in range(n):
        arr[i] = cls(base + es * i * d * h * w, 1, w, w * h)
    return arr


def _make_function3d():
    import torch

    class _SSIM3D(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, data_range, win):
            lead, d, h, w = x.shape[:-3], x.shape[-3], x.shape[-2], x.shape[-1]
            params, n = _params3d(x, y)
            sums = torch.empty(n, dtype=torch.float64, device=x.device)
            if n:
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                if st is None:
                    _context(x.device, work).enqueue_ssim3f(params, n, data_range, sums.data_ptr(), **_win_kw(win))
                else:
                    _context(x.device, work).enqueue_ssim3h(params, n, data_range, st, sums.data_ptr(), **_win_kw(win))
                if work is not cur:
                    cur.wait_stream(work)
            ctx.save_for_backward(x, y)
            ctx.data_range, ctx.win = data_range, win
            return (sums / (float(w) * float(h) * float(d))).to(torch.float32).reshape(lead)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            x, y = ctx.saved_tensors
            d, h, w = x.shape[-3], x.shape[-2], x.shape[-1]
            want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if not (want_x or want_y):
                return None, None, None, None
            params, n = _params3d(x, y)
            g = grad_out.to(torch.float32).reshape(-1).contiguous()
            gx = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_x else None     # the inputs' dtype: the kernel rounds once
            gy = torch.empty(y.shape, dtype=y.dtype, device=y.device) if want_y else None
            if n:
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                ga = _grad_volumes(gx, n, d, h, w) if want_x else None
                gb = _grad_volumes(gy, n, d, h, w) if want_y else None
                if st is None:
                    _context(x.device, work).enqueue_ssim3f_grad(params, n, ctx.data_range, g.data_ptr(), ga, gb, **_win_kw(ctx.win))
                else:
                    _context(x.device, work).enqueue_ssim3h_grad(params, n, ctx.data_range, st, g.data_ptr(), ga, gb, **_win_kw(ctx.win))
                if work is not cur:
                    cur.wait_stream(work)
            return gx, gy, None, None

    return _SSIM3D


def ssim3d(x, y, data_range=1.0, win_size=11, win_sigma=1.5, window="gaussian"):
    """Per-volume SSIM of two float32 GPU tensors of identical shape (..., D, H, W) under the three-dimensional 11-tap Gaussian window
    (sigma 1.5, clamped edges on every axis), any strides (each volume is addressed in place, no copy): a float32 tensor of shape
    x.shape[:-3].  Differentiable with respect to x, y or both; the gradient is computed only for the inputs that need it.  It runs on
    torch's current stream through the cached context, as ssim() does.  TypeError: not tensors, float16 / bfloat16 tensors (the 3-D path
    is float32 for now: ssim3d_amp() takes them), any other dtype.  ValueError: CPU tensors, differing shapes or devices, fewer than 3
    dimensions, empty volumes, a data_range that is not finite and > 0.  Not ssim() on a 5-D tensor: that is one 2-D SSIM per slice.
    The window: win_size taps on every one of the three axes (3, 5, 7, 9 or 11), window "gaussian" with win_sigma or "uniform" (a box;
    win_sigma ignored; edges are clamped, where skimage reflects); the defaults are the engine's window and take exactly the path without
    these arguments.  TypeError: a win_size that is not an int, a window that is not a str.  ValueError: any other win_size, an unknown
    window name, a win_sigma that is not finite and > 0."""
    win = _window(x, y, win_size, win_sigma, window, "ssim3d", fixed16=False)
    return _ssim3d(x, y, _check3d(x, y, data_range), win)


def _ssim3d(x, y, r, win=None):
    global _function3d
    if _function3d is None:
        _function3d = _make_function3d()
    return _function3d.apply(x, y, r, win)


class SSIM3DLoss(object):
    """1 - ssim3d_amp(x, y, data_range): reduction "mean" (a scalar) or "none" (one value per volume).  A plain callable: it has no
    parameters.  float32, float16 or bfloat16 tensors, as ssim3d_amp(); the loss is float32 at every input dtype.  win_size, win_sigma,
    window: the window, as ssim3d_amp() (every input dtype), checked here."""

    def __init__(self, data_range=1.0, reduction="mean", win_size=11, win_sigma=1.5, window="gaussian"):
        if reduction not in ("mean", "none"):
            raise ValueError("SSIM3DLoss: reduction must be 'mean' or 'none', got %r" % (reduction,))
        _window(None, None, win_size, win_sigma, window, "SSIM3DLoss")
        self.data_range, self.reduction = data_range, reduction
        self.win_size, self.win_sigma, self.window = win_size, win_sigma, window

    def __call__(self, x, y):
        loss = 1.0 - ssim3d_amp(x, y, self.data_range, self.win_size, self.win_sigma, self.window)
        return loss.mean() if self.reduction == "mean" else loss


# ---- volumes: the per-voxel map -----------------------------------------------------------------------------------------------------------
# ssim3d_map(x, y, data_range) is the map rmgr_ssim_hip_enqueue_ssim3f writes; its backward is rmgr_ssim_hip_enqueue_ssim3f_map_grad, the
# backward of ssim3d with the upstream gradient read per voxel, in place through grad_out's own strides.

_map_function3d = None


def _grad_out_volumes(g, n):
    """GradOut3F array over the n (D, H, W) volumes of the float32 tensor g, each where it is: any strides, 0 (an expanded tensor)
    included."""
    arr = (api.GradOut3F * max(n, 1))()
    base, strides = g.data_ptr(), (g.stride(-1), g.stride(-2), g.stride(-3))
    for i, off in enumerate(_volume_offsets(g)):
        arr[i] = api.GradOut3F(base + 4 * off, *strides)
    return arr


def _make_map_function3d():
    import torch

    class _SSIM3DMap(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, data_range, win):
            d, h, w = x.shape[-3], x.shape[-2], x.shape[-1]
            params, n = _params3d(x, y)
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            if n:
                sums = torch.empty(n, dtype=torch.float64, device=x.device)      # the kernel's other output, thrown away (ssim_map)
                base = out.data_ptr()
                for i in range(n):
                    params[i].ssimMap = base + 4 * i * d * h * w
                    params[i].ssimStep, params[i].ssimStride, params[i].ssimSliceStride = 1, w, w * h
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                if st is None:
                    _context(x.device, work).enqueue_ssim3f(params, n, data_range, sums.data_ptr(), **_win_kw(win))
                else:
                    _context(x.device, work).enqueue_ssim3h(params, n, data_range, st, sums.data_ptr(), **_win_kw(win))
                if work is not cur:
                    cur.wait_stream(work)
            ctx.save_for_backward(x, y)
            ctx.data_range, ctx.win = data_range, win
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            x, y = ctx.saved_tensors
            d, h, w = x.shape[-3], x.shape[-2], x.shape[-1]
            want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if not (want_x or want_y):
                return None, None, None, None
            params, n = _params3d(x, y)
            g = grad_out if grad_out.dtype == torch.float32 else grad_out.to(torch.float32)      # read in place, through its own strides
            gx = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_x else None     # the inputs' dtype: the kernel rounds once
            gy = torch.empty(y.shape, dtype=y.dtype, device=y.device) if want_y else None
            if n:
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                maps = _grad_out_volumes(g, n)
                ga = _grad_volumes(gx, n, d, h, w) if want_x else None
                gb = _grad_volumes(gy, n, d, h, w) if want_y else None
                if st is None:
                    _context(x.device, work).enqueue_ssim3f_map_grad(params, n, ctx.data_range, maps, ga, gb, **_win_kw(ctx.win))
                else:
                    _context(x.device, work).enqueue_ssim3h_map_grad(params, n, ctx.data_range, st, maps, ga, gb, **_win_kw(ctx.win))
                if work is not cur:
                    cur.wait_stream(work)
            return gx, gy, None, None

    return _SSIM3DMap


def ssim3d_map(x, y, data_range=1.0, win_size=11, win_sigma=1.5, window="gaussian"):
    """Per-voxel SSIM of two float32 GPU tensors of identical shape (..., D, H, W) under the three-dimensional window of ssim3d(), any
    strides (each volume is addressed in place, no copy): a float32 tensor of shape x.shape, the map rmgr_ssim_hip_enqueue_ssim3f
    writes.  Differentiable with respect to x, y or both for ANY upstream gradient: the backward reads grad_out per voxel, in place
    (expanded, sliced and permuted tensors included; another dtype is cast to float32 once) and computes the gradient only for the
    inputs that need it.  It keeps x and y, not the map.  A zero in grad_out does not hide a NaN in the volumes.  win_size, win_sigma,
    window: as ssim3d().  Errors: as ssim3d().

        m = ssim3d_map(x, y)                                  # (N, C, D, H, W)
        loss = 1 - (mask * m).sum() / mask.sum()              # SSIM inside a brain mask"""
    win = _window(x, y, win_size, win_sigma, window, "ssim3d_map", fixed16=False)
    return _ssim3d_map(x, y, _check3d(x, y, data_range, "ssim3d_map"), win)


def _ssim3d_map(x, y, r, win=None):
    global _map_function3d
    if _map_function3d is None:
        _map_function3d = _make_map_function3d()
    return _map_function3d.apply(x, y, r, win)


# ---- volumes: float16 and bfloat16 ----------------------------------------------------------------------------------------------------------
# ssim3d_amp and ssim3d_map_amp are ssim3d and ssim3d_map without their refusal of 16-bit tensors (the top of this file has why there are
# two names): float32 pairs take exactly the path above, float16 and bfloat16 pairs the rmgr_ssim_hip_*_ssim3h* entries.

def ssim3d_amp(x, y, data_range=1.0, win_size=11, win_sigma=1.5, window="gaussian"):
    """ssim3d() for tensors as they come under mixed precision: two GPU tensors of identical shape (..., D, H, W), both float32, both
    float16 or both bfloat16, any strides (each volume is addressed in place, no copy or widening): a float32 tensor of shape
    x.shape[:-3] at every input dtype.  float32 tensors: exactly ssim3d().  float16 and bfloat16: the value has the bits of
    ssim3d(x.float(), y.float()), the gradient has the inputs' dtype and is that call's float32 gradient rounded once, by the kernel
    (see the top of this file for autocast and loss scaling).  Errors: as ssim3d(), under this function's name, except that a mixed pair
    is a TypeError and two float16 or two bfloat16 CPU tensors are a TypeError too: 16-bit tensors are taken on a GPU only (one of the
    two on a GPU: the ValueError).  win_size, win_sigma, window: as ssim3d(), at every input dtype: with float16 and bfloat16 tensors
    the value has the bits of ssim3d(x.float(), y.float(), win_size=...) under the same window and the gradient is that call's, rounded
    once (the rmgr_ssim_hip_*_ssim3h_win* entries; the window is stored on the autograd context and the backward runs under it)."""
    win = _window(x, y, win_size, win_sigma, window, "ssim3d_amp", fixed16=False)
    return _ssim3d(x, y, _check3d(x, y, data_range, "ssim3d_amp", half=True), win)


def ssim3d_map_amp(x, y, data_range=1.0, win_size=11, win_sigma=1.5, window="gaussian"):
    """ssim3d_map() for tensors as they come under mixed precision: two float32, two float16 or two bfloat16 GPU tensors of identical
    shape (..., D, H, W), any strides: the per-voxel map, float32 of shape x.shape at every input dtype (16-bit inputs: the bits of
    ssim3d_map(x.float(), y.float())).  The backward reads grad_out per voxel, in place, as ssim3d_map's does, keeps x and y, not the
    map, and returns the gradient in the inputs' dtype, the float32 value rounded once.  win_size, win_sigma, window: as ssim3d_amp().
    Errors: as ssim3d_amp(), under this function's name.

        m = ssim3d_map_amp(x, y)                              # x, y: (N, C, D, H, W) bfloat16; m: float32
        loss = 1 - (mask * m).sum() / mask.sum()"""
    win = _window(x, y, win_size, win_sigma, window, "ssim3d_map_amp", fixed16=False)
    return _ssim3d_map(x, y, _check3d(x, y, data_range, "ssim3d_map_amp", half=True), win)


# ---- volumes: multi-scale SSIM ----------------------------------------------------------------------------------------------------------------
# ms_ssim3d(x, y, data_range, scales, weights) is the definition in include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_msssim3f): ms_ssim's
# weighted product with ssim3d's per-voxel terms over a pyramid that halves x, y and z.  The backward is
# rmgr_ssim_hip_enqueue_msssim3f_grad, from x, y and the (volumes, scales, 2) float64 per-scale means the forward keeps.  ms_ssim3d_amp and
# MSSSIM3DLoss take float16 / bfloat16 volumes as well, on the msssim3h entries, through the same autograd function.  win_size, win_sigma
# and window are ssim3d()'s keywords and mean the same window on all three axes at EVERY scale (the msssim3f_win and msssim3h_win
# entries); the defaults take exactly the path without them.  A multi-scale map gradient is a follow-up.

_ms_function3d = None


def _make_ms_function3d():
    import torch

    class _MSSSIM3D(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, data_range, scales, weights, win):
            lead = x.shape[:-3]
            params, n = _params3d(x, y)
            values = torch.empty(n, dtype=torch.float64, device=x.device)
            means = torch.empty((n, scales, 2), dtype=torch.float64, device=x.device)
            if n:
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                st = _sample_type(torch, x.dtype)
                if st is None:
                    _context(x.device, work).enqueue_msssim3f(params, n, data_range, values.data_ptr(), means.data_ptr(), scales, weights,
                                                              **_win_kw(win))
                else:
                    _context(x.device, work).enqueue_msssim3h(params, n, data_range, st, values.data_ptr(), means.data_ptr(), scales, weights,
                                                              **_win_kw(win))
                if work is not cur:
                    cur.wait_stream(work)
            ctx.save_for_backward(x, y, means)
            ctx.data_range, ctx.scales, ctx.weights, ctx.win = data_range, scales, weights, win
            return values.to(torch.float32).reshape(lead)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            x, y, means = ctx.saved_tensors
            d, h, w = x.shape[-3], x.shape[-2], x.shape[-1]
            want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if not (want_x or want_y):
                return None, None, None, None, None, None
            params, n = _params3d(x, y)
            g = grad_out.to(torch.float32).reshape(-1).contiguous()
            gx = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_x else None     # the inputs' dtype: the kernel rounds once
            gy = torch.empty(y.shape, dtype=y.dtype, device=y.device) if want_y else None
            if n:
                cur, work = _working_stream(torch, x.device)
                if work is not cur:
                    work.wait_stream(cur)
                ga = _grad_volumes(gx, n, d, h, w) if want_x else None
                gb = _grad_volumes(gy, n, d, h, w) if want_y else None
                st = _sample_type(torch, x.dtype)
                if st is None:
                    _context(x.device, work).enqueue_msssim3f_grad(params, n, ctx.data_range, means.data_ptr(), g.data_ptr(), ga, gb, ctx.scales, ctx.weights,
                                                                   **_win_kw(ctx.win))
                else:
                    _context(x.device, work).enqueue_msssim3h_grad(params, n, ctx.data_range, st, means.data_ptr(), g.data_ptr(), ga, gb, ctx.scales,
                                                                   ctx.weights, **_win_kw(ctx.win))
                if work is not cur:
                    cur.wait_stream(work)
            return gx, gy, None, None, None, None

    return _MSSSIM3D


def _ms_ssim3d(x, y, r, scales, weights, name, win=None):
    global _ms_function3d
    scales, w = _check_scales(scales, weights, name)
    if _ms_function3d is None:
        _ms_function3d = _make_ms_function3d()
    return _ms_function3d.apply(x, y, r, scales, w, win)


def ms_ssim3d(x, y, data_range=1.0, scales=5, weights=None, win_size=11, win_sigma=1.5, window="gaussian"):
    """Per-volume multi-scale SSIM of two float32 GPU tensors of identical shape (..., D, H, W), any strides (each volume is addressed in
    place, no copy): a float32 tensor of shape x.shape[:-3].  The 11-tap Gaussian window (sigma 1.5, clamped edges) on all three axes at
    every scale; all three axes are halved from scale to scale, down to 1 x 1 x 1 if need be.  weights None: Wang's five (scales must be
    5); else `scales` finite weights >= 0.  Differentiable with respect to x, y or both; the gradient is computed only for the inputs that
    need it, from x, y and the (volumes, scales, 2) float64 per-scale means the forward keeps.  It runs on torch's current stream through
    the cached context, as ssim() does.  TypeError / ValueError as ssim3d() and ms_ssim(), under this function's name; float16 and
    bfloat16 tensors are a TypeError here ("the 3-D multi-scale path is float32 for now": pinned by tests from the time there was no
    16-bit path): ms_ssim3d_amp() and MSSSIM3DLoss take them.
    The window: win_size, win_sigma and window are ssim3d()'s keywords with ssim3d()'s errors, and mean the same window on all three axes
    at EVERY scale (rmgr_ssim_hip_enqueue_msssim3f_win, _msssim3f_win_grad; pytorch-msssim's MS_SSIM(spatial_dims=3, win_size,
    win_sigma)); the defaults are the engine's window and take exactly the path without these arguments.  Volumes smaller than the window
    at coarse scales clamp: a 12-frame clip has depth 12, 6, 3, 2, 1, which is what a window of 7 or 3 taps is for."""
    import torch
    if isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and (x.dtype in (torch.float16, torch.bfloat16) or y.dtype in (torch.float16, torch.bfloat16)):
        raise TypeError("ms_ssim3d: the 3-D multi-scale path is float32 for now, got %s and %s; ms_ssim3d_amp() takes float16 / bfloat16 tensors"
                        % (x.dtype, y.dtype))
    win = _window(x, y, win_size, win_sigma, window, "ms_ssim3d", fixed16=False)
    return _ms_ssim3d(x, y, _check3d(x, y, data_range, "ms_ssim3d"), scales, weights, "ms_ssim3d", win)


def ms_ssim3d_amp(x, y, data_range=1.0, scales=5, weights=None, win_size=11, win_sigma=1.5, window="gaussian"):
    """ms_ssim3d() for tensors as they come under mixed precision: two GPU tensors of identical shape (..., D, H, W), both float32, both
    float16 or both bfloat16, any strides (each volume is addressed in place, no copy or widening): a float32 tensor of shape
    x.shape[:-3] at every input dtype.  float32 tensors: exactly ms_ssim3d().  float16 and bfloat16 (rmgr_ssim_hip_enqueue_msssim3h,
    _msssim3h_grad): the value has the bits of ms_ssim3d(x.float(), y.float()), the gradient has the inputs' dtype and is that call's
    float32 gradient rounded once, by the kernel (see the top of this file for autocast and loss scaling); saved for the backward are x, y
    and the float64 means.  Errors: as ms_ssim3d(), under this function's name, except that a mixed pair is a TypeError and two float16 or
    two bfloat16 CPU tensors are a TypeError too: 16-bit tensors are taken on a GPU only (one of the two on a GPU: the ValueError).  That
    message keeps the words "the 3-D multi-scale path is float32 for now", which tests/test_msssim3f_cpu.py pins for
    MSSSIM3DLoss()(x16_cpu, x16_cpu) from the time there was no 16-bit path.  win_size, win_sigma, window: as ms_ssim3d(), at every input
    dtype: with float16 and bfloat16 tensors (rmgr_ssim_hip_enqueue_msssim3h_win, _msssim3h_win_grad) the value has the bits of
    ms_ssim3d(x.float(), y.float(), win_size=...) under the same window and the gradient is that call's, rounded once."""
    win = _window(x, y, win_size, win_sigma, window, "ms_ssim3d_amp", fixed16=False)
    if _is_half_pair(x, y) and not x.is_cuda and not y.is_cuda:
        raise TypeError("ms_ssim3d_amp: float16 / bfloat16 tensors are taken on a GPU only (on the CPU the 3-D multi-scale path is float32 for "
                        "now), got %s on %s and %s" % (x.dtype, x.device, y.device))
    return _ms_ssim3d(x, y, _check3d(x, y, data_range, "ms_ssim3d_amp", half=True), scales, weights, "ms_ssim3d_amp", win)


class MSSSIM3DLoss(object):
    """1 - ms_ssim3d_amp(x, y, data_range, scales, weights): reduction "mean" (a scalar) or "none" (one value per volume).  A plain
    callable: it has no parameters.  float32, float16 or bfloat16 tensors, as ms_ssim3d_amp(); the loss is float32 at every input dtype.
    win_size, win_sigma, window: the window of every scale, as ms_ssim3d(), checked here; GPU tensors take it at every dtype."""

    def __init__(self, data_range=1.0, scales=5, weights=None, reduction="mean", win_size=11, win_sigma=1.5, window="gaussian"):
        if reduction not in ("mean", "none"):
            raise ValueError("MSSSIM3DLoss: reduction must be 'mean' or 'none', got %r" % (reduction,))
        _check_scales(scales, weights, "MSSSIM3DLoss")
        _window(None, None, win_size, win_sigma, window, "MSSSIM3DLoss", fixed16=False)
        self.data_range, self.scales, self.weights, self.reduction = data_range, scales, weights, reduction
        self.win_size, self.win_sigma, self.window = win_size, win_sigma, window

    def __call__(self, x, y):
        loss = 1.0 - ms_ssim3d_amp(x, y, self.data_range, self.scales, self.weights, self.win_size, self.win_sigma, self.window)
        return loss.mean() if self.reduction == "mean" else loss
