"""GPU: the host flow that the 16-bit, float32 and float16 / bfloat16 SSIM entry points share (ssim_amd/csrc/ssim_samples_abi.cpp), held
for every encoding to the same two properties, bit for bit:

  * host pointers: staging of a view whose sample range starts below topLeft (negative step and stride) and of an interleaved one, and
    the copy-back of the map at a step and stride of its own, against the binding's dense call on contiguous copies of the pixels;
  * the ring of descriptor tables: more back-to-back enqueues than the ring has slots, against the blocking call on each pair alone.

No tolerance: both sides run the same kernels on the same pixels.  The inputs are those of tests/sample_forms_inputs.py and the
generators it draws from.
"""
import ctypes

import numpy as np
import pytest

import halfmodel as HM
import sample_forms_inputs as S
import ssim_amd

pytestmark = pytest.mark.gpu

ENCODINGS = ("uint16", "float32") + HM.ENCODINGS
ENC = pytest.mark.parametrize("enc", ENCODINGS)
DEPTH = 10
SF_SLOTS = 8            # kSfSlots of ssim_context.h


class Family(object):
    """What differs between the encodings: the pixels, the parameter block, the entry points and their extra arguments."""

    def __init__(self, enc):
        self.enc = enc
        self.half = enc in HM.ENCODINGS
        self.dtype = np.dtype(np.float32 if enc == "float32" else np.uint16)
        self.params, self.make = (ssim_amd.ParamsF, ssim_amd.make_params_f) if enc == "float32" else (ssim_amd.Params16, ssim_amd.make_params16)
        self.name = {"uint16": "ssim16", "float32": "ssimf"}.get(enc, "ssimh")
        u32, f32 = ctypes.c_uint32, ctypes.c_float
        self.extra = {"uint16": (u32(DEPTH),), "float32": (f32(S.RANGE),)}.get(enc) or (u32(ssim_amd.sample_type_code(enc)), f32(S.RANGE))

    def pair(self, shape):
        if self.enc == "uint16":
            return S.pair_16(shape, DEPTH)
        return S.pair_h(shape, self.enc)[0] if self.half else S.pair_f(shape)

    def pairs(self, n, shape):
        """n different pairs of one shape."""
        h, w = shape
        if self.enc == "uint16":
            return S.pairs16(np.random.default_rng(S.SEED), n, shape, DEPTH)
        if self.half:
            return [S.random_pair_h(h, w, np.random.default_rng(S.SEED + i), self.enc)[0] for i in range(n)]
        return [S.random_pair_f(h, w, np.random.default_rng(S.SEED + i)) for i in range(n)]

    def dense(self, a, b):
        """(value, map) of the binding's host call on contiguous arrays."""
        if self.enc == "uint16":
            return ssim_amd.compute_ssim16(a, b, DEPTH, want_map=True)
        if self.enc == "float32":
            return ssim_amd.compute_ssimf(a, b, S.RANGE, want_map=True)
        return ssim_amd.compute_ssimh(HM.host_array(a, self.enc)[0], HM.host_array(b, self.enc)[0], S.RANGE,
                                      sample_type=HM.host_array(a, self.enc)[1], want_map=True)

    def host(self, ps):
        """rmgr_ssim_hip_compute_*_host of one Params block on a default context (ctx == NULL): the float32 value."""
        out = (ctypes.c_float * 1)()
        fn = getattr(ssim_amd.load_library(), "rmgr_ssim_hip_compute_%s_host" % self.name)
        assert fn(None, 1, ps, *(self.extra + (out,))) == 0
        return np.float32(out[0])

    def enqueue(self, ctx, ps, sums_ptr):
        fn = getattr(ctx.lib, "rmgr_ssim_hip_enqueue_%s" % self.name)
        assert fn(ctx.handle, 1, ps, *(self.extra + (sums_ptr,))) == 0

    def device(self, ctx, ps):
        out = (ctypes.c_float * 1)()
        fn = getattr(ctx.lib, "rmgr_ssim_hip_compute_%s_device" % self.name)
        assert fn(ctx.handle, 1, ps, *(self.extra + (out,))) == 0
        return np.float32(out[0])


@ENC
def test_host_staging_and_strided_map_copy_back(enc):
    """130 x 19: two strips, map rows that are no multiple of 64 bytes.  A is read mirrored and bottom-up (its sample range lies below
    topLeft: lo < 0), B interleaved at step 2; the map goes to every second float of a sentinel-filled buffer, to a bottom-up buffer,
    and nowhere (ssimMap == NULL)."""
    fam = Family(enc)
    a, b = (np.ascontiguousarray(x) for x in fam.pair(S.BIG))
    h, w = a.shape
    assert (w, h) == (130, 19) and a.dtype == fam.dtype
    v, dense = fam.dense(a, b)
    es = fam.dtype.itemsize
    store_a = np.ascontiguousarray(a[::-1, ::-1])                      # pixel (x, y) at store_a[h-1-y, w-1-x]
    store_b = np.zeros((h, w, 2), fam.dtype)
    store_b[:, :, 0] = b

    def run(map_ptr, step, stride):
        ps = (fam.params * 1)()
        ps[0] = fam.make(w, h, store_a.ctypes.data + es * (h * w - 1), -1, -w, store_b.ctypes.data, 2, 2 * w, map_ptr, step, stride)
        return fam.host(ps)
    wide = np.full((h, 2 * w), -7.0, np.float32)                       # ssimStep 2
    assert run(wide.ctypes.data, 2, 2 * w).tobytes() == np.float32(v).tobytes()
    assert wide[:, 0::2].tobytes() == dense.tobytes() and np.all(wide[:, 1::2] == -7.0)
    flip = np.zeros((h, w), np.float32)                                # negative ssimStride
    assert run(flip[h - 1].ctypes.data, 1, -w).tobytes() == np.float32(v).tobytes()
    assert flip[::-1].tobytes() == dense.tobytes()
    assert run(None, 1, w).tobytes() == np.float32(v).tobytes()        # NULL: no map


@ENC
def test_enqueues_beyond_the_ring_keep_their_order(gpu_ctx, enc):
    """33 x 17, 2 * kSfSlots + 1 different pairs: one enqueue each into sums[i], back to back, one synchronise.  Every sum gives the
    float of the blocking device call on its pair alone."""
    fam = Family(enc)
    n, (h, w) = 2 * SF_SLOTS + 1, (17, 33)
    pairs = fam.pairs(n, (h, w))
    assert len(set(np.ascontiguousarray(a).tobytes() for a, _ in pairs)) == n
    bufs, blocks = [], []
    for a, b in pairs:
        da, db = gpu_ctx.upload(a), gpu_ctx.upload(b)
        bufs += [da, db]
        ps = (fam.params * 1)()
        ps[0] = fam.make(w, h, da.ptr, 1, w, db.ptr, 1, w)
        blocks.append(ps)
    sums = gpu_ctx.alloc(8 * n)
    try:
        want = [fam.device(gpu_ctx, ps) for ps in blocks]
        assert len(set(x.tobytes() for x in want)) > 1
        for i, ps in enumerate(blocks):
            fam.enqueue(gpu_ctx, ps, ctypes.c_void_p(sums.ptr + 8 * i))
        gpu_ctx.synchronize()
        got = sums.download(np.float64, (n,))
        for i in range(n):
            assert np.float32(got[i] / np.float64(w * h)).tobytes() == want[i].tobytes(), (enc, i, got[i], float(want[i]))
    finally:
        for buf in bufs + [sums]:
            buf.free()
