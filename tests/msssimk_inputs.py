"""What tests/test_gpu_msssimk.py and tests/test_gpu_msssimhk.py share: pairs in device memory under a window (the DevicePairs of
tests/test_gpu_msssimh.py with one more argument), and a pair whose samples lie far apart (the 64-bit forms of the kernels)."""
import numpy as np

import ssim_amd

BOX3, G9 = (3, 0.0, "uniform"), (9, 1.5, "gaussian")
# One window per radius 1 .. 4 (the kernels of msssimk_kernels.hip / msssimhk_kernels.hip), and radius 5 with other taps.
PER_RADIUS = ((3, 0.0, "uniform"), (5, 0.8, "gaussian"), (7, 0.0, "uniform"), (9, 1.5, "gaussian"), (11, 0.0, "uniform"))


def mk(window):
    """ssim_amd.Window of a (size, sigma, kind) triple; None stays None (the entries without _win)."""
    if window is None:
        return None
    size, sigma, kind = window
    return ssim_amd.make_window(size, sigma if kind == "gaussian" else 1.5, kind)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def same(got, want):
    """Arrays of one dtype with the same bit patterns."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def random_pair(h, w, rng, r=1.0):
    a = rng.random((h, w), dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal((h, w)).astype(np.float32), 0, 1).astype(np.float32)
    return a * np.float32(r), b * np.float32(r)


# Odd sizes whose planes are smaller than the window at coarse scales, (H, W) and the numbers of scales (uniform weights) each is run at:
# down to 1 x 1; (40, 300) has two strip columns at scale 1; (9, 603) has multi-cell strips.
ODD_SIZES = (((1, 1), tuple(range(1, 9))), ((3, 5), tuple(range(1, 9))), ((17, 33), tuple(range(1, 9))), ((7, 300), tuple(range(1, 9))),
             ((40, 300), (4,)), ((9, 603), (3,)))
ODD_G_OUT = -0.75


def odd_cases():
    """(h, w, scales to run, a, b, data range) of ODD_SIZES at ranges 1 and 255: seeded, a smooth ramp under noise and a lightly
    disturbed copy, so that every per-scale mean stays well above the ReLU down to the 1 x 1 planes."""
    for i, ((h, w), configs) in enumerate(ODD_SIZES):
        rng = np.random.default_rng(700 + i)
        yy, xx = np.mgrid[0:h, 0:w]
        a = (0.25 + 0.5 * (xx + 2 * yy) / float(w + 2 * h) + 0.1 * rng.random((h, w))).astype(np.float32)
        b = (a + np.float32(0.03) * rng.standard_normal((h, w)).astype(np.float32)).astype(np.float32)
        for r in (1.0, 255.0):
            yield h, w, configs, a * np.float32(r), b * np.float32(r), r


class DevicePairs(object):
    """Pairs of one size in device memory, each image in a buffer of its own, samples `step` apart and `lead` elements into the buffer.
    kind "f": float32 planes (ParamsF, the msssimf entries); else the encoding of uint16 bit patterns (Params16, the msssimh entries).
    window: an ssim_amd.Window, or None for the entries without _win."""

    def __init__(self, ctx, pairs, kind="f", step=1, lead=0):
        self.ctx, self.n, self.kind = ctx, len(pairs), kind
        self.h, self.w = pairs[0][0].shape
        self.dt, self.es = (np.float32, 4) if kind == "f" else (np.uint16, 2)
        self.bufs = []
        self.params = ((ssim_amd.ParamsF if kind == "f" else ssim_amd.Params16) * self.n)()
        make = ssim_amd.make_params_f if kind == "f" else ssim_amd.make_params16
        for i, (a, b) in enumerate(pairs):
            d = []
            for img in (a, b):
                store = np.zeros(lead + self.h * self.w * step, self.dt)
                store[lead:].reshape(self.h, self.w, step)[:, :, step - 1] = img
                d.append(ctx.upload(store))
            self.bufs += d
            off = self.es * (lead + step - 1)
            self.params[i] = make(self.w, self.h, d[0].ptr + off, step, self.w * step, d[1].ptr + off, step, self.w * step)

    def enqueue(self, r, vals_ptr, means_ptr, scales, weights, window):
        if self.kind == "f":
            self.ctx.enqueue_msssimf(self.params, self.n, r, vals_ptr, means_ptr, scales, weights, window=window)
        else:
            self.ctx.enqueue_msssimh(self.params, self.n, r, self.kind, vals_ptr, means_ptr, scales, weights, window=window)

    def enqueue_grad(self, r, means_ptr, go_ptr, ga, gb, scales, weights, window):
        if self.kind == "f":
            self.ctx.enqueue_msssimf_grad(self.params, self.n, r, means_ptr, go_ptr, ga, gb, scales, weights, window=window)
        else:
            self.ctx.enqueue_msssimh_grad(self.params, self.n, r, self.kind, means_ptr, go_ptr, ga, gb, scales, weights, window=window)

    def forward(self, r, window, scales=5, weights=None, keep=False):
        """(values float64 (n,), means float64 (n, scales, 2)) through the enqueue entry; keep: also the device buffer of the means."""
        vals, means = self.ctx.alloc(8 * self.n), self.ctx.alloc(16 * self.n * scales)
        self.enqueue(r, vals.ptr, means.ptr, scales, weights, window)
        self.ctx.synchronize()
        v, m = vals.download(np.float64, (self.n,)), means.download(np.float64, (self.n, scales, 2))
        vals.free()
        if keep:
            return v, m, means
        means.free()
        return v, m

    def device(self, r, window, scales=5, weights=None):
        if self.kind == "f":
            return self.ctx.msssimf_device(self.params, self.n, r, scales, weights, per_scale=True, window=window)
        return self.ctx.msssimh_device(self.params, self.n, r, self.kind, scales, weights, per_scale=True, window=window)

    def grad_planes(self, want_a=True, want_b=True, gstep=1, lead=0):
        """(GradF / GradH arrays [dA, dB] (None where not wanted), their buffers, the filler)."""
        n, h, w = self.n, self.h, self.w
        mark = self.dt(-777.0) if self.kind == "f" else np.uint16(0xABCD)
        fill = np.full(lead + h * w * gstep, mark, self.dt)
        cls = ssim_amd.GradF if self.kind == "f" else ssim_amd.GradH
        arrs, bufs = [None, None], [[], []]
        for k, want in enumerate((want_a, want_b)):
            if not want:
                continue
            arrs[k] = (cls * n)()
            for i in range(n):
                buf = self.ctx.upload(fill)
                bufs[k].append(buf)
                arrs[k][i] = cls(buf.ptr + self.es * lead, gstep, w * gstep)
        return arrs, bufs, fill

    def collect(self, arrs, bufs, fill, gstep=1, lead=0):
        """[(dA or None, dB or None)] per pair from grad_planes()' buffers, everything but the gradient samples checked untouched; frees."""
        n, h, w = self.n, self.h, self.w
        out = []
        for i in range(n):
            pair = []
            for k in range(2):
                if arrs[k] is None:
                    pair.append(None)
                    continue
                raw = bufs[k][i].download(self.dt, (lead + h * w * gstep,))
                g = raw[lead:].reshape(h, w, gstep)
                assert np.all(bits(raw[:lead]) == bits(fill[:1])[0]) and np.all(bits(g[:, :, 1:]) == bits(fill[:1])[0])
                pair.append(np.ascontiguousarray(g[:, :, 0]))
            out.append(tuple(pair))
        for b in bufs[0] + bufs[1]:
            b.free()
        return out

    def grads(self, r, window, g_out, scales=5, weights=None, want_a=True, want_b=True, gstep=1, lead=0, means=None):
        """[(dLoss/dA or None, dLoss/dB or None)] per pair, forward then backward, in the pairs' sample type; gradient planes with samples
        gstep apart and `lead` elements into their buffer.  means: a float64 (n, scales, 2) array handed to the backward in place of
        this forward's."""
        ctx, n = self.ctx, self.n
        if means is None:
            _, _, means = self.forward(r, window, scales, weights, keep=True)
        else:
            means = np.ascontiguousarray(means, np.float64)
            assert means.shape == (n, scales, 2)
            means = ctx.upload(means)
        go = ctx.upload(np.asarray(g_out, np.float32))
        arrs, bufs, fill = self.grad_planes(want_a, want_b, gstep, lead)
        self.enqueue_grad(r, means.ptr, go.ptr, arrs[0], arrs[1], scales, weights, window)
        ctx.synchronize()
        out = self.collect(arrs, bufs, fill, gstep, lead)
        go.free()
        means.free()
        return out

    def free(self):
        for b in self.bufs:
            b.free()


def far_apart_call(ctx, kind, planes, far, sign, r, window, g_out, scales, weights, filler):
    """One H x W pair (H <= 16) whose samples lie `far` elements apart -- one volume of W columns `far` elements apart, rows one element
    apart: A in rows 0 .., B in rows 16 .., dLoss/dA in rows 32 .., dLoss/dB in rows 48 .. of every column, read forwards (sign 1) or with
    a negative step.  Returns (values, means, dA, dB, untouched): untouched says that nothing but the two gradient planes changed."""
    h, w = planes[0].shape
    assert h <= 16
    dt, es = (np.float32, 4) if kind == "f" else (np.uint16, 2)
    vol = np.full(w * far, filler, dt)
    cols = vol.reshape(w, far)
    for x in range(w):
        c = x if sign > 0 else w - 1 - x
        for k, plane in enumerate(planes):
            cols[c, 16 * k:16 * k + h] = plane[:, x]
    dvol = ctx.upload(vol)
    first = 0 if sign > 0 else (w - 1) * far                  # the element of column x = 0
    P, make, G = (ssim_amd.ParamsF, ssim_amd.make_params_f, ssim_amd.GradF) if kind == "f" else (ssim_amd.Params16, ssim_amd.make_params16, ssim_amd.GradH)
    ps = (P * 1)()
    ps[0] = make(w, h, dvol.ptr + es * first, sign * far, 1, dvol.ptr + es * (first + 16), sign * far, 1)
    ga, gb = (G * 1)(), (G * 1)()
    ga[0], gb[0] = G(dvol.ptr + es * (first + 32), sign * far, 1), G(dvol.ptr + es * (first + 48), sign * far, 1)
    vals, means, go = ctx.alloc(8), ctx.alloc(16 * scales), ctx.upload(np.asarray(g_out, np.float32))
    if kind == "f":
        ctx.enqueue_msssimf(ps, 1, r, vals.ptr, means.ptr, scales, weights, window=window)
        ctx.enqueue_msssimf_grad(ps, 1, r, means.ptr, go.ptr, ga, gb, scales, weights, window=window)
    else:
        ctx.enqueue_msssimh(ps, 1, r, kind, vals.ptr, means.ptr, scales, weights, window=window)
        ctx.enqueue_msssimh_grad(ps, 1, r, kind, means.ptr, go.ptr, ga, gb, scales, weights, window=window)
    ctx.synchronize()
    fv, fm = vals.download(np.float64, (1,)), means.download(np.float64, (1, scales, 2))
    got = dvol.download(dt, (w, far))
    for x in (dvol, vals, means, go):
        x.free()
    order = slice(None) if sign > 0 else slice(None, None, -1)
    da = np.ascontiguousarray(got[order, 32:32 + h].T)
    db = np.ascontiguousarray(got[order, 48:48 + h].T)
    got[:, 32:32 + h] = cols[:, 32:32 + h]
    got[:, 48:48 + h] = cols[:, 48:48 + h]
    return fv, fm, da, db, np.array_equal(bits(got), bits(cols))
