"""The two 16-bit float encodings of rmgr_ssim_hip_*_ssimh* (include/rmgr/ssim-hip.h) on numpy arrays of bit patterns: the exact
widening to float32 and the single round-to-nearest-even back.

float16: numpy's own np.float16 is the reference (astype rounds to nearest-even, keeps subnormals, overflows to Inf).
bfloat16: numpy has no such dtype; a sample is the upper half of a float32, so widening is a shift and rounding is integer arithmetic on
the float32 bit pattern.  tests/test_ssimh_cpu.py holds both helpers to torch's CPU conversions.

Samples travel as uint16 arrays (the bit patterns) in both encodings.
"""
import numpy as np

F16, BF16 = "float16", "bfloat16"
ENCODINGS = (F16, BF16)


def widen(u16, enc):
    """uint16 bit patterns -> the float32 values they stand for, exactly."""
    u16 = np.ascontiguousarray(u16, np.uint16)
    if enc == F16:
        return u16.view(np.float16).astype(np.float32)
    assert enc == BF16
    return (u16.astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_to(f32, enc):
    """float32 values -> uint16 bit patterns of the encoding, one rounding to nearest-even.  NaN gives a NaN (payload unspecified)."""
    f32 = np.ascontiguousarray(f32, np.float32)
    if enc == F16:
        with np.errstate(over="ignore"):
            return f32.astype(np.float16).view(np.uint16)
    assert enc == BF16
    u = f32.view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x0040, r).astype(np.uint16)


def is_nan(u16, enc):
    u16 = np.asarray(u16, np.uint16)
    return (u16 & 0x7FFF) > (0x7C00 if enc == F16 else 0x7F80)


def is_subnormal(u16, enc):
    """Non-zero with a zero exponent field."""
    u16 = np.asarray(u16, np.uint16)
    return ((u16 & (0x7C00 if enc == F16 else 0x7F80)) == 0) & ((u16 & 0x7FFF) != 0)


def same(got, want, enc):
    """The same bit patterns, NaN compared as NaN."""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    gn, wn = is_nan(got, enc), is_nan(want, enc)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(got[~gn], want[~wn])


def same_f32(got, want):
    """float32 arrays with the same bit patterns, NaN compared as NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(got[~gn].view(np.uint32), want[~wn].view(np.uint32))


def host_array(u16, enc):
    """What ssim_amd.compute_ssimh takes for these bit patterns: an np.float16 view, or the uint16 array and sample_type="bfloat16"."""
    return (u16.view(np.float16), None) if enc == F16 else (u16, BF16)
