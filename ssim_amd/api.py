"""ctypes binding of the C ABI in include/rmgr/ssim-hip.h and include/rmgr/ssim.h.

This module is plumbing for tests and bench.py: the product is the shared library
(ssim_amd/lib/librmgr-ssim-hip.so) and its C/C++ headers.  Struct layouts mirror
include/rmgr/ssim.h field for field (reference include/rmgr/ssim.h:469-533).

There is no fallback of any kind: if the library is missing, or no gfx950 device is usable,
calls raise (ImportError / SsimError with the errno the C ABI returned).
"""
import ctypes
import errno
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RMGR_SSIM_LIB") or os.path.join(_HERE, "lib", "librmgr-ssim-hip.so")   # env override: A/B builds in tools/

MODE_EXACT, MODE_FAST, MODE_DOUBLE, MODE_UNFUSED, MODE_SEPARABLE = 0, 1, 2, 3, 4

c_pd = ctypes.c_ssize_t  # ptrdiff_t

AllocFct = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t)
DeallocFct = ctypes.CFUNCTYPE(None, ctypes.c_void_p)
ThreadFct = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint32)
ThreadPoolFct = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ThreadFct, ctypes.POINTER(ctypes.c_void_p),
                                 ctypes.c_uint32, ctypes.c_uint32)


class Version(ctypes.Structure):
    _fields_ = [("major", ctypes.c_uint32), ("minor", ctypes.c_uint32), ("patch", ctypes.c_uint32),
                ("string", ctypes.c_char_p)]


class ImgParams(ctypes.Structure):
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd)]


class Params(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("imgA", ImgParams), ("imgB", ImgParams),
                ("ssimMap", ctypes.c_void_p), ("ssimStep", c_pd), ("ssimStride", c_pd),
                ("alloc", AllocFct), ("dealloc", DeallocFct)]


class Img16(ctypes.Structure):
    """rmgr_ssim_hip_Img16: step and stride count uint16 samples, not bytes."""
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd)]


class Params16(ctypes.Structure):
    """rmgr_ssim_hip_Params16: ssimStep and ssimStride count floats; ssimMap None = no map."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("imgA", Img16), ("imgB", Img16),
                ("ssimMap", ctypes.c_void_p), ("ssimStep", c_pd), ("ssimStride", c_pd)]


class ImgF(ctypes.Structure):
    """rmgr_ssim_hip_ImgF: step and stride count floats, not bytes."""
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd)]


class ParamsF(ctypes.Structure):
    """rmgr_ssim_hip_ParamsF: ssimStep and ssimStride count floats; ssimMap None = no map."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("imgA", ImgF), ("imgB", ImgF),
                ("ssimMap", ctypes.c_void_p), ("ssimStep", c_pd), ("ssimStride", c_pd)]


class GradF(ctypes.Structure):
    """rmgr_ssim_hip_GradF: one gradient plane in device memory; step and stride count floats."""
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd)]


class Img3F(ctypes.Structure):
    """rmgr_ssim_hip_Img3F: one float32 volume; step, stride and sliceStride count floats, not bytes."""
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd), ("sliceStride", c_pd)]


class Params3F(ctypes.Structure):
    """rmgr_ssim_hip_Params3F: ssimStep, ssimStride and ssimSliceStride count floats; ssimMap None = no map."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("depth", ctypes.c_uint32),
                ("imgA", Img3F), ("imgB", Img3F),
                ("ssimMap", ctypes.c_void_p), ("ssimStep", c_pd), ("ssimStride", c_pd), ("ssimSliceStride", c_pd)]


class Grad3F(ctypes.Structure):
    """rmgr_ssim_hip_Grad3F: one gradient volume in device memory; step, stride and sliceStride count floats."""
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd), ("sliceStride", c_pd)]


class Img3H(ctypes.Structure):
    """rmgr_ssim_hip_Img3H: one float16 / bfloat16 volume; step, stride and sliceStride count 16-bit samples, not bytes."""
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd), ("sliceStride", c_pd)]


class Params3H(ctypes.Structure):
    """rmgr_ssim_hip_Params3H: the map is float32 -- ssimStep, ssimStride and ssimSliceStride count floats; ssimMap None = no map."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("depth", ctypes.c_uint32),
                ("imgA", Img3H), ("imgB", Img3H),
                ("ssimMap", ctypes.c_void_p), ("ssimStep", c_pd), ("ssimStride", c_pd), ("ssimSliceStride", c_pd)]


class Grad3H(ctypes.Structure):
    """rmgr_ssim_hip_Grad3H: one float16 / bfloat16 gradient volume in device memory; step, stride and sliceStride count 16-bit samples."""
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd), ("sliceStride", c_pd)]


class GradH(ctypes.Structure):
    """rmgr_ssim_hip_GradH: one float16 / bfloat16 gradient plane in device memory; step and stride count 16-bit samples."""
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd)]


class GradOutF(ctypes.Structure):
    """rmgr_ssim_hip_GradOutF: one float32 plane dLoss/dssim(p) in device memory; step and stride count floats, 0 allowed (both 0: one
    float stands for the whole plane)."""
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd)]


class GradOut3F(ctypes.Structure):
    """rmgr_ssim_hip_GradOut3F: one float32 volume dLoss/dssim(p) in device memory; step, stride and sliceStride count floats, negatives
    and 0 allowed (all three 0: one float stands for the whole volume)."""
    _fields_ = [("topLeft", ctypes.c_void_p), ("step", c_pd), ("stride", c_pd), ("sliceStride", c_pd)]


class Window(ctypes.Structure):
    """rmgr_ssim_hip_Window: the window of the _ssimf_win entries -- size taps per axis (3, 5, 7, 9 or 11), kind WINDOW_GAUSSIAN (sigma
    finite, > 0) or WINDOW_UNIFORM (a box; sigma ignored)."""
    _fields_ = [("size", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("sigma", ctypes.c_float)]


WINDOW_GAUSSIAN, WINDOW_UNIFORM = 0, 1      # RMGR_SSIM_HIP_WINDOW_GAUSSIAN / _UNIFORM
WINDOW_SIZES = (3, 5, 7, 9, 11)
_WINDOW_KINDS = {"gaussian": WINDOW_GAUSSIAN, "uniform": WINDOW_UNIFORM}


def make_window(size=11, sigma=1.5, kind="gaussian"):
    """A Window of `size` taps per axis: kind "gaussian" with `sigma`, or "uniform" (a box; sigma is ignored).  TypeError: a size that is
    not an int, a kind that is not a str.  ValueError: a size outside 3, 5, 7, 9, 11, an unknown kind, a Gaussian sigma that is not finite
    or not > 0 as a float32 -- what the library answers with EINVAL."""
    if isinstance(size, bool) or not isinstance(size, int):
        raise TypeError("window size must be an int, not %s" % type(size).__name__)
    if not isinstance(kind, str):
        raise TypeError("window kind must be a str, not %s" % type(kind).__name__)
    if size not in WINDOW_SIZES:
        raise ValueError("window size %d: must be one of 3, 5, 7, 9, 11" % size)
    if kind not in _WINDOW_KINDS:
        raise ValueError("window kind %r: must be 'gaussian' or 'uniform'" % (kind,))
    if kind == "uniform":
        return Window(size, WINDOW_UNIFORM, 0.0)
    s = float(np.float32(sigma))
    if not (s > 0.0 and s != float("inf")):
        raise ValueError("window sigma %r: must be finite and > 0" % (sigma,))
    return Window(size, WINDOW_GAUSSIAN, s)


def _window_ref(window):
    """The `window` argument of a _win entry: a Window by reference (None: NULL, the engine's window)."""
    if window is None:
        return None
    if not isinstance(window, Window):
        raise TypeError("window must be an ssim_amd.Window (make_window) or None")
    return ctypes.byref(window)


SAMPLE_F16, SAMPLE_BF16 = 0, 1      # RMGR_SSIM_HIP_SAMPLE_F16 / _BF16
_SAMPLE_TYPES = {"float16": SAMPLE_F16, "bfloat16": SAMPLE_BF16}


class Plan(ctypes.Structure):
    _fields_ = [("structSize", ctypes.c_uint32), ("stripWidth", ctypes.c_uint32), ("stripRows", ctypes.c_uint32), ("stripsX", ctypes.c_uint32),
                ("stripsY", ctypes.c_uint32), ("wavefronts", ctypes.c_uint32), ("waveSlots", ctypes.c_uint32), ("earlyRowSums", ctypes.c_uint32),
                ("cellRows", ctypes.c_uint32), ("cellsX", ctypes.c_uint32), ("cellsY", ctypes.c_uint32),
                ("balancedChunks", ctypes.c_uint32), ("balancedChunkRows", ctypes.c_uint32), ("balancedInterleave", ctypes.c_uint32)]


class TunedEntry(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("count", ctypes.c_uint32), ("withMap", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("variant", ctypes.c_int32), ("stripRows", ctypes.c_uint32)]


class TuneResult(ctypes.Structure):
    _fields_ = [("structSize", ctypes.c_uint32), ("candidates", ctypes.c_uint32), ("bestVariant", ctypes.c_int32), ("bestStripRows", ctypes.c_uint32),
                ("defaultMs", ctypes.c_double), ("bestMs", ctypes.c_double),
                ("candidateVariant", ctypes.c_int32 * 8), ("candidateStripRows", ctypes.c_uint32 * 8), ("candidateMs", ctypes.c_double * 8)]


ABI_VERSION = 6      # RMGR_SSIM_HIP_ABI_VERSION of include/rmgr/ssim-hip.h this binding was written against


class ThreadPool(ctypes.Structure):
    _fields_ = [("dispatch", ThreadPoolFct), ("context", ctypes.c_void_p), ("threadCount", ctypes.c_uint32)]


class SsimError(RuntimeError):
    def __init__(self, fn, code):
        self.errno = code
        RuntimeError.__init__(self, "%s failed: errno %d (%s)" % (fn, code, errno.errorcode.get(code, "?")))


# every symbol include/rmgr/*.h declares with C linkage (tests check the library exports them all)
C_SYMBOLS = [
    "rmgr_ssim_get_version", "rmgr_ssim_init_interleaved", "rmgr_ssim_init_planar", "rmgr_ssim_use_default_allocator",
    "rmgr_ssim_compute_ssim", "rmgr_ssim_compute_ssim_openmp",
    "rmgr_ssim_hip_get_device_count", "rmgr_ssim_hip_create", "rmgr_ssim_hip_destroy", "rmgr_ssim_hip_set_mode",
    "rmgr_ssim_hip_get_mode", "rmgr_ssim_hip_set_tuning", "rmgr_ssim_hip_get_plan", "rmgr_ssim_hip_compute_ssim_host",
    "rmgr_ssim_hip_compute_ssim_device", "rmgr_ssim_hip_compute_ssim_batch_host", "rmgr_ssim_hip_compute_ssim_batch_host_devices",
    "rmgr_ssim_hip_enqueue_batch", "rmgr_ssim_hip_finalize",
    "rmgr_ssim_hip_synchronize", "rmgr_ssim_hip_malloc", "rmgr_ssim_hip_free", "rmgr_ssim_hip_memcpy_h2d",
    "rmgr_ssim_hip_memcpy_d2h", "rmgr_ssim_hip_set_profiling", "rmgr_ssim_hip_get_profile", "rmgr_ssim_hip_describe",
    "rmgr_ssim_hip_compute_ssim_channels_host", "rmgr_ssim_hip_compute_ssim_luminance_host", "rmgr_ssim_hip_luminance_device",
    "rmgr_ssim_hip_synth_pair_device",
    "rmgr_ssim_hip_comm_get_unique_id", "rmgr_ssim_hip_comm_init", "rmgr_ssim_hip_comm_allreduce_sums", "rmgr_ssim_hip_comm_destroy",
    "rmgr_ssim_hip_comm_rank_count", "rmgr_ssim_hip_comm_describe", "rmgr_ssim_hip_get_abi_version", "rmgr_ssim_hip_get_default_pool", "rmgr_ssim_hip_get_kernel_source_id",
    "rmgr_ssim_hip_enqueue_rows", "rmgr_ssim_hip_reduce_cells", "rmgr_ssim_hip_probe_valu",
    "rmgr_ssim_hip_trim", "rmgr_ssim_hip_trim_default_pool", "rmgr_ssim_hip_get_default_pool_memory", "rmgr_ssim_hip_get_memory_info",
    "rmgr_ssim_hip_tune", "rmgr_ssim_hip_clear_tuned", "rmgr_ssim_hip_get_tuned", "rmgr_ssim_hip_set_tuned", "rmgr_ssim_hip_get_profile_clock",
    "rmgr_ssim_hip_compute_msssim_device", "rmgr_ssim_hip_compute_msssim_host",
    "rmgr_ssim_hip_enqueue_ssim16", "rmgr_ssim_hip_compute_ssim16_device", "rmgr_ssim_hip_compute_ssim16_host",
    "rmgr_ssim_hip_enqueue_ssimf", "rmgr_ssim_hip_compute_ssimf_device", "rmgr_ssim_hip_compute_ssimf_host", "rmgr_ssim_hip_enqueue_ssimf_grad",
    "rmgr_ssim_hip_enqueue_msssimf", "rmgr_ssim_hip_compute_msssimf_device", "rmgr_ssim_hip_compute_msssimf_host", "rmgr_ssim_hip_enqueue_msssimf_grad",
    "rmgr_ssim_hip_enqueue_ssimh", "rmgr_ssim_hip_compute_ssimh_device", "rmgr_ssim_hip_compute_ssimh_host", "rmgr_ssim_hip_enqueue_ssimh_grad",
    "rmgr_ssim_hip_enqueue_ssimf_map_grad", "rmgr_ssim_hip_enqueue_ssimh_map_grad",
    "rmgr_ssim_hip_enqueue_ssimf_win", "rmgr_ssim_hip_compute_ssimf_win_device", "rmgr_ssim_hip_compute_ssimf_win_host",
    "rmgr_ssim_hip_enqueue_ssimf_win_grad", "rmgr_ssim_hip_enqueue_ssimf_win_map_grad",
    "rmgr_ssim_hip_enqueue_ssimh_win", "rmgr_ssim_hip_compute_ssimh_win_device", "rmgr_ssim_hip_compute_ssimh_win_host",
    "rmgr_ssim_hip_enqueue_ssimh_win_grad", "rmgr_ssim_hip_enqueue_ssimh_win_map_grad",
    "rmgr_ssim_hip_enqueue_msssimh", "rmgr_ssim_hip_compute_msssimh_device", "rmgr_ssim_hip_compute_msssimh_host", "rmgr_ssim_hip_enqueue_msssimh_grad",
    "rmgr_ssim_hip_enqueue_msssimf_win", "rmgr_ssim_hip_compute_msssimf_win_device", "rmgr_ssim_hip_compute_msssimf_win_host",
    "rmgr_ssim_hip_enqueue_msssimf_win_grad",
    "rmgr_ssim_hip_enqueue_msssimh_win", "rmgr_ssim_hip_compute_msssimh_win_device", "rmgr_ssim_hip_compute_msssimh_win_host",
    "rmgr_ssim_hip_enqueue_msssimh_win_grad",
    "rmgr_ssim_hip_enqueue_ssim3f", "rmgr_ssim_hip_compute_ssim3f_device", "rmgr_ssim_hip_compute_ssim3f_host", "rmgr_ssim_hip_enqueue_ssim3f_grad",
    "rmgr_ssim_hip_enqueue_ssim3f_map_grad",
    "rmgr_ssim_hip_enqueue_ssim3h", "rmgr_ssim_hip_compute_ssim3h_device", "rmgr_ssim_hip_compute_ssim3h_host", "rmgr_ssim_hip_enqueue_ssim3h_grad",
    "rmgr_ssim_hip_enqueue_ssim3h_map_grad",
    "rmgr_ssim_hip_enqueue_ssim3f_win", "rmgr_ssim_hip_compute_ssim3f_win_device", "rmgr_ssim_hip_compute_ssim3f_win_host",
    "rmgr_ssim_hip_enqueue_ssim3f_win_grad", "rmgr_ssim_hip_enqueue_ssim3f_win_map_grad",
    "rmgr_ssim_hip_enqueue_ssim3h_win", "rmgr_ssim_hip_compute_ssim3h_win_device", "rmgr_ssim_hip_compute_ssim3h_win_host",
    "rmgr_ssim_hip_enqueue_ssim3h_win_grad", "rmgr_ssim_hip_enqueue_ssim3h_win_map_grad",
    "rmgr_ssim_hip_enqueue_msssim3f", "rmgr_ssim_hip_compute_msssim3f_device", "rmgr_ssim_hip_compute_msssim3f_host", "rmgr_ssim_hip_enqueue_msssim3f_grad",
    "rmgr_ssim_hip_enqueue_msssim3h", "rmgr_ssim_hip_compute_msssim3h_device", "rmgr_ssim_hip_compute_msssim3h_host", "rmgr_ssim_hip_enqueue_msssim3h_grad",
    "rmgr_ssim_hip_enqueue_msssim3f_win", "rmgr_ssim_hip_compute_msssim3f_win_device", "rmgr_ssim_hip_compute_msssim3f_win_host",
    "rmgr_ssim_hip_enqueue_msssim3f_win_grad",
    "rmgr_ssim_hip_enqueue_msssim3h_win", "rmgr_ssim_hip_compute_msssim3h_win_device", "rmgr_ssim_hip_compute_msssim3h_win_host",
    "rmgr_ssim_hip_enqueue_msssim3h_win_grad",
]
# non-inline C++ entry points of the reference, Itanium-mangled
CXX_SYMBOLS = [
    "_ZN4rmgr4ssim12compute_ssimEPfRK17rmgr_ssim_Params_PK21rmgr_ssim_ThreadPool_",
    "_ZN4rmgr4ssim12compute_ssimERKNS0_6ParamsE",
    "_ZN4rmgr4ssim11select_implENS0_14ImplementationE",
]

_lib = None


def load_library(path=None):
    """dlopen the product library.  Raises ImportError when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError("%s not found: build it with `make lib` (hipcc --offload-arch=gfx950); "
                          "ssim_amd has no CPU fallback" % p)
    lib = ctypes.CDLL(p)
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    PP = ctypes.POINTER(Params)
    PW = ctypes.POINTER(Window)
    sig = {
        "rmgr_ssim_get_version": [ctypes.POINTER(Version)],
        "rmgr_ssim_init_interleaved": [ctypes.POINTER(ImgParams), vp, c_pd, u32, u32],
        "rmgr_ssim_init_planar": [ctypes.POINTER(ImgParams), ctypes.POINTER(vp), ctypes.POINTER(c_pd), u32],
        "rmgr_ssim_use_default_allocator": [PP],
        "rmgr_ssim_compute_ssim": [ctypes.POINTER(ctypes.c_float), PP, ctypes.POINTER(ThreadPool)],
        "rmgr_ssim_compute_ssim_openmp": [ctypes.POINTER(ctypes.c_float), PP],
        "rmgr_ssim_hip_get_device_count": [ctypes.POINTER(i32)],
        "rmgr_ssim_hip_create": [ctypes.POINTER(vp), i32, vp],
        "rmgr_ssim_hip_destroy": [vp],
        "rmgr_ssim_hip_set_mode": [vp, i32],
        "rmgr_ssim_hip_get_mode": [vp, ctypes.POINTER(i32)],
        "rmgr_ssim_hip_set_tuning": [vp, i32, i32],
        "rmgr_ssim_hip_get_plan": [vp, u32, u32, u32, ctypes.POINTER(Plan)],
        "rmgr_ssim_hip_compute_ssim_host": [vp, ctypes.POINTER(ctypes.c_float), PP, ctypes.POINTER(ThreadPool)],
        "rmgr_ssim_hip_compute_ssim_device": [vp, ctypes.POINTER(ctypes.c_float), PP],
        "rmgr_ssim_hip_enqueue_batch": [vp, u32, PP, vp],
        "rmgr_ssim_hip_compute_ssim_batch_host": [vp, u32, PP, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_compute_ssim_batch_host_devices": [ctypes.POINTER(i32), u32, i32, u32, PP, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_finalize": [u32, ctypes.POINTER(ctypes.c_double), u32, u32, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_synchronize": [vp],
        "rmgr_ssim_hip_malloc": [vp, ctypes.POINTER(vp), ctypes.c_size_t],
        "rmgr_ssim_hip_free": [vp, vp],
        "rmgr_ssim_hip_memcpy_h2d": [vp, vp, vp, ctypes.c_size_t],
        "rmgr_ssim_hip_memcpy_d2h": [vp, vp, vp, ctypes.c_size_t],
        "rmgr_ssim_hip_set_profiling": [vp, i32],
        "rmgr_ssim_hip_get_profile": [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_compute_ssim_channels_host": [vp, ctypes.POINTER(ctypes.c_float), vp, c_pd, vp, c_pd, u32, u32, u32, vp],
        "rmgr_ssim_hip_compute_ssim_luminance_host": [vp, ctypes.POINTER(ctypes.c_float), vp, c_pd, vp, c_pd, u32, u32, u32, vp],
        "rmgr_ssim_hip_luminance_device": [vp, vp, c_pd, vp, c_pd, c_pd, u32, u32],
        "rmgr_ssim_hip_synth_pair_device": [vp, vp, c_pd, vp, c_pd, u32, u32, ctypes.c_uint64],
        "rmgr_ssim_hip_comm_get_unique_id": [ctypes.c_char_p],
        "rmgr_ssim_hip_comm_init": [vp, ctypes.c_char_p, i32, i32],
        "rmgr_ssim_hip_comm_allreduce_sums": [vp, vp, u32],
        "rmgr_ssim_hip_comm_destroy": [vp],
        "rmgr_ssim_hip_comm_rank_count": [vp, ctypes.POINTER(i32)],
        "rmgr_ssim_hip_enqueue_rows": [vp, PP, u32, u32, vp],
        "rmgr_ssim_hip_reduce_cells": [vp, u32, u32, u32, vp, vp],
        "rmgr_ssim_hip_probe_valu": [vp, i32, i32, i32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_get_profile_clock": [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)],
        "rmgr_ssim_hip_trim": [vp],
        "rmgr_ssim_hip_tune": [vp, u32, u32, u32, i32, ctypes.POINTER(TuneResult)],
        "rmgr_ssim_hip_clear_tuned": [vp],
        "rmgr_ssim_hip_get_tuned": [vp, u32, ctypes.POINTER(TunedEntry)],
        "rmgr_ssim_hip_set_tuned": [vp, u32, u32, u32, i32, i32, u32],
        "rmgr_ssim_hip_trim_default_pool": [],
        "rmgr_ssim_hip_get_default_pool_memory": [ctypes.POINTER(ctypes.c_uint64)] * 3,
        "rmgr_ssim_hip_get_memory_info": [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
        "rmgr_ssim_hip_compute_msssim_device": [vp, u32, PP, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_compute_msssim_host": [vp, u32, PP, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_enqueue_ssim16": [vp, u32, ctypes.POINTER(Params16), u32, vp],
        "rmgr_ssim_hip_compute_ssim16_device": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_compute_ssim16_host": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_enqueue_ssimf": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, vp],
        "rmgr_ssim_hip_compute_ssimf_device": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_compute_ssimf_host": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_enqueue_ssimf_grad": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, vp, ctypes.POINTER(GradF), ctypes.POINTER(GradF)],
        "rmgr_ssim_hip_enqueue_ssimh": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, vp],
        "rmgr_ssim_hip_compute_ssimh_device": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_compute_ssimh_host": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_enqueue_ssimh_grad": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, vp, ctypes.POINTER(GradH), ctypes.POINTER(GradH)],
        "rmgr_ssim_hip_enqueue_ssim3f": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, vp],
        "rmgr_ssim_hip_compute_ssim3f_device": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_compute_ssim3f_host": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_enqueue_ssim3f_grad": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, vp, ctypes.POINTER(Grad3F), ctypes.POINTER(Grad3F)],
        "rmgr_ssim_hip_enqueue_ssim3f_map_grad": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, ctypes.POINTER(GradOut3F), ctypes.POINTER(Grad3F), ctypes.POINTER(Grad3F)],
        "rmgr_ssim_hip_enqueue_ssim3f_win": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, PW, vp],
        "rmgr_ssim_hip_compute_ssim3f_win_device": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, PW, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_compute_ssim3f_win_host": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, PW, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_enqueue_ssim3f_win_grad": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, PW, vp, ctypes.POINTER(Grad3F), ctypes.POINTER(Grad3F)],
        "rmgr_ssim_hip_enqueue_ssim3f_win_map_grad": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, PW, ctypes.POINTER(GradOut3F), ctypes.POINTER(Grad3F), ctypes.POINTER(Grad3F)],
        "rmgr_ssim_hip_enqueue_ssim3h": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, vp],
        "rmgr_ssim_hip_compute_ssim3h_device": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_compute_ssim3h_host": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_enqueue_ssim3h_grad": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, vp, ctypes.POINTER(Grad3H), ctypes.POINTER(Grad3H)],
        "rmgr_ssim_hip_enqueue_ssim3h_map_grad": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, ctypes.POINTER(GradOut3F), ctypes.POINTER(Grad3H), ctypes.POINTER(Grad3H)],
        "rmgr_ssim_hip_enqueue_ssimh_win": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, PW, vp],
        "rmgr_ssim_hip_compute_ssimh_win_device": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, PW, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_compute_ssimh_win_host": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, PW, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_enqueue_ssimh_win_grad": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, PW, vp, ctypes.POINTER(GradH), ctypes.POINTER(GradH)],
        "rmgr_ssim_hip_enqueue_ssimh_win_map_grad": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, PW, ctypes.POINTER(GradOutF), ctypes.POINTER(GradH), ctypes.POINTER(GradH)],
        "rmgr_ssim_hip_enqueue_ssim3h_win": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, PW, vp],
        "rmgr_ssim_hip_compute_ssim3h_win_device": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, PW, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_compute_ssim3h_win_host": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, PW, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_enqueue_ssim3h_win_grad": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, PW, vp, ctypes.POINTER(Grad3H), ctypes.POINTER(Grad3H)],
        "rmgr_ssim_hip_enqueue_ssim3h_win_map_grad": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, PW, ctypes.POINTER(GradOut3F), ctypes.POINTER(Grad3H), ctypes.POINTER(Grad3H)],
        "rmgr_ssim_hip_enqueue_ssimf_map_grad": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, ctypes.POINTER(GradOutF), ctypes.POINTER(GradF), ctypes.POINTER(GradF)],
        "rmgr_ssim_hip_enqueue_ssimh_map_grad": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, ctypes.POINTER(GradOutF), ctypes.POINTER(GradH), ctypes.POINTER(GradH)],
        "rmgr_ssim_hip_enqueue_ssimf_win": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, PW, vp],
        "rmgr_ssim_hip_compute_ssimf_win_device": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, PW, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_compute_ssimf_win_host": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, PW, ctypes.POINTER(ctypes.c_float)],
        "rmgr_ssim_hip_enqueue_ssimf_win_grad": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, PW, vp, ctypes.POINTER(GradF), ctypes.POINTER(GradF)],
        "rmgr_ssim_hip_enqueue_ssimf_win_map_grad": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, PW, ctypes.POINTER(GradOutF), ctypes.POINTER(GradF), ctypes.POINTER(GradF)],
        "rmgr_ssim_hip_enqueue_msssim3f": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), vp, vp],
        "rmgr_ssim_hip_compute_msssim3f_device": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_compute_msssim3f_host": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_enqueue_msssim3f_grad": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), vp, vp, ctypes.POINTER(Grad3F), ctypes.POINTER(Grad3F)],
        "rmgr_ssim_hip_enqueue_msssimf": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), vp, vp],
        "rmgr_ssim_hip_compute_msssimf_device": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_compute_msssimf_host": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_enqueue_msssimf_grad": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), vp, vp, ctypes.POINTER(GradF), ctypes.POINTER(GradF)],
        "rmgr_ssim_hip_enqueue_msssim3h": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), vp, vp],
        "rmgr_ssim_hip_compute_msssim3h_device": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_compute_msssim3h_host": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_enqueue_msssim3h_grad": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), vp, vp, ctypes.POINTER(Grad3H), ctypes.POINTER(Grad3H)],
        "rmgr_ssim_hip_enqueue_msssimh": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), vp, vp],
        "rmgr_ssim_hip_compute_msssimh_device": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_compute_msssimh_host": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_enqueue_msssimh_grad": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, u32, ctypes.POINTER(ctypes.c_double), vp, vp, ctypes.POINTER(GradH), ctypes.POINTER(GradH)],
        "rmgr_ssim_hip_enqueue_msssim3f_win": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), vp, vp],
        "rmgr_ssim_hip_compute_msssim3f_win_device": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_compute_msssim3f_win_host": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_enqueue_msssim3f_win_grad": [vp, u32, ctypes.POINTER(Params3F), ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), vp, vp, ctypes.POINTER(Grad3F), ctypes.POINTER(Grad3F)],
        "rmgr_ssim_hip_enqueue_msssim3h_win": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), vp, vp],
        "rmgr_ssim_hip_compute_msssim3h_win_device": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_compute_msssim3h_win_host": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_enqueue_msssim3h_win_grad": [vp, u32, ctypes.POINTER(Params3H), u32, ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), vp, vp, ctypes.POINTER(Grad3H), ctypes.POINTER(Grad3H)],
        "rmgr_ssim_hip_enqueue_msssimf_win": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), vp, vp],
        "rmgr_ssim_hip_compute_msssimf_win_device": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_compute_msssimf_win_host": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_enqueue_msssimf_win_grad": [vp, u32, ctypes.POINTER(ParamsF), ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), vp, vp, ctypes.POINTER(GradF), ctypes.POINTER(GradF)],
        "rmgr_ssim_hip_enqueue_msssimh_win": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), vp, vp],
        "rmgr_ssim_hip_compute_msssimh_win_device": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_compute_msssimh_win_host": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)],
        "rmgr_ssim_hip_enqueue_msssimh_win_grad": [vp, u32, ctypes.POINTER(Params16), u32, ctypes.c_float, PW, u32, ctypes.POINTER(ctypes.c_double), vp, vp, ctypes.POINTER(GradH), ctypes.POINTER(GradH)],
    }
    for name, args in sig.items():
        if path is None and os.environ.get("RMGR_SSIM_LIB") and not hasattr(lib, name):
            continue                      # A/B runs against an older build of the library (tools/ab_libs.sh)
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = i32
    if hasattr(lib, "rmgr_ssim_hip_get_abi_version"):
        lib.rmgr_ssim_hip_get_abi_version.argtypes = []
        lib.rmgr_ssim_hip_get_abi_version.restype = i32
        if path is None and not os.environ.get("RMGR_SSIM_LIB") and lib.rmgr_ssim_hip_get_abi_version() != ABI_VERSION:
            raise ImportError("%s implements rmgr/ssim-hip.h interface version %d, this binding expects %d: rebuild with `make lib`"
                              % (p, lib.rmgr_ssim_hip_get_abi_version(), ABI_VERSION))
    lib.rmgr_ssim_hip_describe.argtypes = [vp]
    lib.rmgr_ssim_hip_describe.restype = ctypes.c_char_p
    if hasattr(lib, "rmgr_ssim_hip_comm_describe"):
        lib.rmgr_ssim_hip_comm_describe.argtypes = []
        lib.rmgr_ssim_hip_comm_describe.restype = ctypes.c_char_p
    if path is None:
        _lib = lib
    return lib


def get_plan(width, height, count=1, ctx=None):
    """Strip geometry of a launch (include/rmgr/ssim-hip.h rmgr_ssim_hip_get_plan); needs no device when ctx is None."""
    lib = load_library()
    out = Plan()
    out.structSize = ctypes.sizeof(Plan)
    _check("rmgr_ssim_hip_get_plan", lib.rmgr_ssim_hip_get_plan(ctx.handle if ctx is not None else None, width, height, count, ctypes.byref(out)))
    return out


def _check(name, rc):
    if rc != 0:
        raise SsimError(name, rc)


def device_count():
    n = ctypes.c_int32(0)
    _check("rmgr_ssim_hip_get_device_count", load_library().rmgr_ssim_hip_get_device_count(ctypes.byref(n)))
    return n.value


def get_version():
    v = Version()
    _check("rmgr_ssim_get_version", load_library().rmgr_ssim_get_version(ctypes.byref(v)))
    return (v.major, v.minor, v.patch, v.string.decode())


def make_params(width, height, a_ptr, a_step, a_stride, b_ptr, b_step, b_stride, map_ptr=None, map_step=1, map_stride=None):
    p = Params()
    p.width, p.height = width, height
    p.imgA = ImgParams(a_ptr, a_step, a_stride)
    p.imgB = ImgParams(b_ptr, b_step, b_stride)
    p.ssimMap = map_ptr
    p.ssimStep = map_step
    p.ssimStride = width if map_stride is None else map_stride
    return p


def finalize(sums, width, height):
    """float(sum / double(width*height)) per entry, computed by the library (src/ssim.cpp:1102)."""
    sums = np.ascontiguousarray(sums, np.float64)
    out = np.empty(sums.shape, np.float32)
    _check("rmgr_ssim_hip_finalize", load_library().rmgr_ssim_hip_finalize(
        sums.size, sums.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), width, height,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return out


def compute_ssim(a, b, want_map=False, openmp=False, allocator=False, out_map=None):
    """The drop-in entry point rmgr_ssim_compute_ssim() on two host uint8 planes (H x W numpy).
    out_map: reuse this H x W float32 array for the map (avoids first-touch page faults in timing loops)."""
    lib = load_library()
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    h, w = a.shape
    if out_map is not None:
        assert out_map.shape == (h, w) and out_map.dtype == np.float32 and out_map.flags.c_contiguous
        want_map = True
    m = (out_map if out_map is not None else np.empty((h, w), np.float32)) if want_map else None
    p = make_params(w, h, a.ctypes.data, 1, a.strides[0], b.ctypes.data, 1, b.strides[0],
                    m.ctypes.data if want_map else None, 1, w)
    if allocator:
        _check("rmgr_ssim_use_default_allocator", lib.rmgr_ssim_use_default_allocator(ctypes.byref(p)))
    out = ctypes.c_float()
    if openmp:
        _check("rmgr_ssim_compute_ssim_openmp", lib.rmgr_ssim_compute_ssim_openmp(ctypes.byref(out), ctypes.byref(p)))
    else:
        _check("rmgr_ssim_compute_ssim", lib.rmgr_ssim_compute_ssim(ctypes.byref(out), ctypes.byref(p), None))
    return np.float32(out.value), m


def kernel_source_id():
    """sha256 of the kernel source the loaded library was compiled from (rmgr_ssim_hip_get_kernel_source_id)."""
    lib = load_library()
    lib.rmgr_ssim_hip_get_kernel_source_id.restype = ctypes.c_char_p
    lib.rmgr_ssim_hip_get_kernel_source_id.argtypes = []
    return lib.rmgr_ssim_hip_get_kernel_source_id().decode()


def default_pool():
    """(contexts that exist, calls that may be in flight at a time) of the ctx == NULL entry points' default contexts."""
    lib = load_library()
    n, lim = ctypes.c_int32(), ctypes.c_int32()
    lib.rmgr_ssim_hip_get_default_pool.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    _check("rmgr_ssim_hip_get_default_pool", lib.rmgr_ssim_hip_get_default_pool(ctypes.byref(n), ctypes.byref(lim)))
    return n.value, lim.value


def default_pool_memory():
    """(device bytes, pinned host bytes) the default contexts held when their last call ended, and the retain cap in bytes (per context)."""
    d, p, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _check("rmgr_ssim_hip_get_default_pool_memory", load_library().rmgr_ssim_hip_get_default_pool_memory(ctypes.byref(d), ctypes.byref(p), ctypes.byref(c)))
    return d.value, p.value, c.value


def trim_default_pool():
    """Releases the staging of every default context that is not inside a call (rmgr_ssim_hip_trim_default_pool)."""
    _check("rmgr_ssim_hip_trim_default_pool", load_library().rmgr_ssim_hip_trim_default_pool())


def memory_info(ctx=None):
    """(free, total) bytes of the context's device (ctx None: the default contexts' device)."""
    f, t = ctypes.c_uint64(), ctypes.c_uint64()
    _check("rmgr_ssim_hip_get_memory_info", load_library().rmgr_ssim_hip_get_memory_info(ctx.handle if ctx is not None else None, ctypes.byref(f), ctypes.byref(t)))
    return f.value, t.value


def compute_ssim_batch(pairs, ctx=None):
    """Global SSIM of many host image pairs of one size (rmgr_ssim_hip_compute_ssim_batch_host: pipelined staging).
    pairs: sequence of (a, b) uint8 arrays, H x W (any strides numpy can express along both axes)."""
    lib = load_library()
    n = len(pairs)
    params = (Params * n)()
    for i, (a, b) in enumerate(pairs):
        h, w = a.shape
        params[i] = make_params(w, h, a.ctypes.data, a.strides[1], a.strides[0], b.ctypes.data, b.strides[1], b.strides[0])
    out = (ctypes.c_float * n)()
    _check("rmgr_ssim_hip_compute_ssim_batch_host", lib.rmgr_ssim_hip_compute_ssim_batch_host(ctx.handle if ctx is not None else None, n, params, out))
    return np.array(out[:], np.float32)


def compute_ssim_batch_devices(pairs, devices=None, mode=MODE_EXACT):
    """compute_ssim_batch() sharded by image over `devices` (a list of device indices; None: all visible) from this one
    process (rmgr_ssim_hip_compute_ssim_batch_host_devices)."""
    lib = load_library()
    n = len(pairs)
    params = (Params * max(n, 1))()
    for i, (a, b) in enumerate(pairs):
        h, w = a.shape
        params[i] = make_params(w, h, a.ctypes.data, a.strides[1], a.strides[0], b.ctypes.data, b.strides[1], b.strides[0])
    out = (ctypes.c_float * max(n, 1))()
    devs = (ctypes.c_int32 * len(devices))(*devices) if devices is not None else None
    _check("rmgr_ssim_hip_compute_ssim_batch_host_devices",
           lib.rmgr_ssim_hip_compute_ssim_batch_host_devices(devs, len(devices) if devices is not None else 0, mode, n, params, out))
    return np.array(out[:n], np.float32)


def compute_ssim_channels(a, b, want_map=False):
    """All channels of two interleaved H x W x C uint8 arrays in one launch (host pointers)."""
    lib = load_library()
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    h, w, ch = a.shape
    out = (ctypes.c_float * ch)()
    m = np.empty((h, w, ch), np.float32) if want_map else None
    _check("rmgr_ssim_hip_compute_ssim_channels_host", lib.rmgr_ssim_hip_compute_ssim_channels_host(
        None, out, a.ctypes.data, w * ch, b.ctypes.data, w * ch, w, h, ch, m.ctypes.data if want_map else None))
    return np.array(out[:], np.float32), m


def compute_ssim_luminance(a, b, want_map=False):
    """SSIM of the BT.601 luminance (computed on the GPU) of two interleaved H x W x C (C >= 3) uint8 arrays."""
    lib = load_library()
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    h, w, ch = a.shape
    out = ctypes.c_float()
    m = np.empty((h, w), np.float32) if want_map else None
    _check("rmgr_ssim_hip_compute_ssim_luminance_host", lib.rmgr_ssim_hip_compute_ssim_luminance_host(
        None, ctypes.byref(out), a.ctypes.data, w * ch, b.ctypes.data, w * ch, w, h, ch, m.ctypes.data if want_map else None))
    return np.float32(out.value), m


MSSSIM_MAX_SCALES = 8     # RMGR_SSIM_HIP_MSSSIM_MAX_SCALES
MSSSIM_WANG_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _msssim_call(fn_name, handle, params, count, scales, weights, per_scale):
    lib = load_library()
    w = None
    if weights is not None:
        w = (ctypes.c_double * max(len(weights), 1))(*[float(x) for x in weights])
    out = (ctypes.c_float * max(count, 1))()
    means = (ctypes.c_double * max(count * scales * 2, 1))() if per_scale else None
    _check(fn_name, getattr(lib, fn_name)(handle, count, params, scales, w, out, means))
    vals = np.array(out[:count], np.float32)
    if not per_scale:
        return vals
    return vals, np.array(means[:count * scales * 2], np.float64).reshape(count, scales, 2)


def compute_msssim(a, b, scales=5, weights=None, per_scale=False, ctx=None):
    """Multi-scale SSIM of two H x W uint8 host arrays (any strides numpy can express, negative ones included) through
    rmgr_ssim_hip_compute_msssim_host.  weights None: Wang's five (scales must be 5).  Returns a float32, and with
    per_scale=True also a (scales, 2) float64 array of [scale]{mcs, mssim}."""
    assert a.shape == b.shape and a.ndim == 2 and a.dtype == np.uint8 and b.dtype == np.uint8
    h, w = a.shape
    params = (Params * 1)()
    params[0] = make_params(w, h, a.ctypes.data, a.strides[1], a.strides[0], b.ctypes.data, b.strides[1], b.strides[0])
    r = _msssim_call("rmgr_ssim_hip_compute_msssim_host", ctx.handle if ctx is not None else None, params, 1, scales, weights, per_scale)
    return (r[0][0], r[1][0]) if per_scale else r[0]


def compute_msssim_batch(pairs, scales=5, weights=None, per_scale=False, ctx=None):
    """compute_msssim() of many host pairs of one size in one call: a float32 array (and a (count, scales, 2) array with per_scale)."""
    n = len(pairs)
    params = (Params * max(n, 1))()
    for i, (a, b) in enumerate(pairs):
        h, w = a.shape
        params[i] = make_params(w, h, a.ctypes.data, a.strides[1], a.strides[0], b.ctypes.data, b.strides[1], b.strides[0])
    return _msssim_call("rmgr_ssim_hip_compute_msssim_host", ctx.handle if ctx is not None else None, params, n, scales, weights, per_scale)


def make_params16(width, height, a_ptr, a_step, a_stride, b_ptr, b_step, b_stride, map_ptr=None, map_step=1, map_stride=None):
    """rmgr_ssim_hip_Params16; steps and strides in samples (images) and floats (map)."""
    p = Params16()
    p.width, p.height = width, height
    p.imgA = Img16(a_ptr, a_step, a_stride)
    p.imgB = Img16(b_ptr, b_step, b_stride)
    p.ssimMap = map_ptr
    p.ssimStep = map_step
    p.ssimStride = width if map_stride is None else map_stride
    return p


def _u16_view(x):
    """A host-byte-order uint16 array whose strides are whole samples: x itself when it already is one (negative strides kept)."""
    assert x.ndim == 2 and x.dtype.kind == "u" and x.dtype.itemsize == 2, "H x W uint16 expected"
    if not x.dtype.isnative:
        x = x.astype(np.uint16)
    if x.strides[0] % 2 or x.strides[1] % 2 or x.ctypes.data % 2:
        x = np.ascontiguousarray(x)
    return x


def _params16_of(a, b, map_ptr=None):
    h, w = a.shape
    return make_params16(w, h, a.ctypes.data, a.strides[1] // 2, a.strides[0] // 2, b.ctypes.data, b.strides[1] // 2, b.strides[0] // 2,
                         map_ptr, 1, w)


def compute_ssim16(a, b, bit_depth, want_map=False, ctx=None):
    """SSIM of two H x W uint16 host arrays of `bit_depth` (8..16) bits (any strides numpy can express, negative ones included)
    through rmgr_ssim_hip_compute_ssim16_host.  Returns (float32 value, H x W float32 map or None)."""
    a, b = _u16_view(a), _u16_view(b)
    assert a.shape == b.shape
    h, w = a.shape
    m = np.empty((h, w), np.float32) if want_map else None
    params = (Params16 * 1)()
    params[0] = _params16_of(a, b, m.ctypes.data if want_map else None)
    out = (ctypes.c_float * 1)()
    _check("rmgr_ssim_hip_compute_ssim16_host", load_library().rmgr_ssim_hip_compute_ssim16_host(
        ctx.handle if ctx is not None else None, 1, params, bit_depth, out))
    return np.float32(out[0]), m


def compute_ssim16_batch(pairs, bit_depth, ctx=None):
    """compute_ssim16() of many host pairs of one size in one call (no maps): a float32 array."""
    pairs = [(_u16_view(a), _u16_view(b)) for a, b in pairs]
    n = len(pairs)
    params = (Params16 * max(n, 1))()
    for i, (a, b) in enumerate(pairs):
        params[i] = _params16_of(a, b)
    out = (ctypes.c_float * max(n, 1))()
    _check("rmgr_ssim_hip_compute_ssim16_host", load_library().rmgr_ssim_hip_compute_ssim16_host(
        ctx.handle if ctx is not None else None, n, params, bit_depth, out))
    return np.array(out[:n], np.float32)


def make_params_f(width, height, a_ptr, a_step, a_stride, b_ptr, b_step, b_stride, map_ptr=None, map_step=1, map_stride=None):
    """rmgr_ssim_hip_ParamsF; steps and strides in floats (images and map)."""
    p = ParamsF()
    p.width, p.height = width, height
    p.imgA = ImgF(a_ptr, a_step, a_stride)
    p.imgB = ImgF(b_ptr, b_step, b_stride)
    p.ssimMap = map_ptr
    p.ssimStep = map_step
    p.ssimStride = width if map_stride is None else map_stride
    return p


def _f32_view(x):
    """A native float32 array whose strides are whole floats: x itself when it already is one (negative strides kept)."""
    assert x.ndim == 2 and x.dtype.kind == "f" and x.dtype.itemsize == 4, "H x W float32 expected"
    if not x.dtype.isnative:
        x = x.astype(np.float32)
    if x.strides[0] % 4 or x.strides[1] % 4 or x.ctypes.data % 4:
        x = np.ascontiguousarray(x)
    return x


def _params_f_of(a, b, map_ptr=None):
    h, w = a.shape
    return make_params_f(w, h, a.ctypes.data, a.strides[1] // 4, a.strides[0] // 4, b.ctypes.data, b.strides[1] // 4, b.strides[0] // 4,
                         map_ptr, 1, w)


def _ssimf_host(handle, count, params, data_range, window, out):
    """rmgr_ssim_hip_compute_ssimf_host, or -- a window given -- rmgr_ssim_hip_compute_ssimf_win_host."""
    lib = load_library()
    if window is None:
        _check("rmgr_ssim_hip_compute_ssimf_host", lib.rmgr_ssim_hip_compute_ssimf_host(handle, count, params, data_range, out))
    else:
        _check("rmgr_ssim_hip_compute_ssimf_win_host", lib.rmgr_ssim_hip_compute_ssimf_win_host(handle, count, params, data_range, _window_ref(window), out))


def compute_ssimf(a, b, data_range, want_map=False, ctx=None, window=None):
    """SSIM of two H x W float32 host arrays at `data_range` (any strides numpy can express, negative ones included) through
    rmgr_ssim_hip_compute_ssimf_host; window (a Window, make_window): through rmgr_ssim_hip_compute_ssimf_win_host under that window.
    Returns (float32 value, H x W float32 map or None)."""
    a, b = _f32_view(a), _f32_view(b)
    assert a.shape == b.shape
    h, w = a.shape
    m = np.empty((h, w), np.float32) if want_map else None
    params = (ParamsF * 1)()
    params[0] = _params_f_of(a, b, m.ctypes.data if want_map else None)
    out = (ctypes.c_float * 1)()
    _ssimf_host(ctx.handle if ctx is not None else None, 1, params, data_range, window, out)
    return np.float32(out[0]), m


def compute_ssimf_batch(pairs, data_range, ctx=None, window=None):
    """compute_ssimf() of many host pairs of one size in one call (no maps): a float32 array."""
    pairs = [(_f32_view(a), _f32_view(b)) for a, b in pairs]
    n = len(pairs)
    params = (ParamsF * max(n, 1))()
    for i, (a, b) in enumerate(pairs):
        params[i] = _params_f_of(a, b)
    out = (ctypes.c_float * max(n, 1))()
    _ssimf_host(ctx.handle if ctx is not None else None, n, params, data_range, window, out)
    return np.array(out[:n], np.float32)


def make_params3f(width, height, depth, a_ptr, a_strides, b_ptr, b_strides, map_ptr=None, map_strides=None):
    """rmgr_ssim_hip_Params3F; a_strides, b_strides, map_strides: (step, stride, sliceStride) in floats (map_strides None: a dense
    depth x height x width map)."""
    p = Params3F()
    p.width, p.height, p.depth = width, height, depth
    p.imgA = Img3F(a_ptr, *a_strides)
    p.imgB = Img3F(b_ptr, *b_strides)
    p.ssimMap = map_ptr
    p.ssimStep, p.ssimStride, p.ssimSliceStride = (1, width, width * height) if map_strides is None else map_strides
    return p


def _f32_volume(x):
    """A native float32 D x H x W array whose strides are whole floats: x itself when it already is one (negative strides kept)."""
    assert x.ndim == 3 and x.dtype.kind == "f" and x.dtype.itemsize == 4, "D x H x W float32 expected"
    if not x.dtype.isnative:
        x = x.astype(np.float32)
    if any(s % 4 for s in x.strides) or x.ctypes.data % 4:
        x = np.ascontiguousarray(x)
    return x


def _params3f_of(a, b, map_ptr=None):
    d, h, w = a.shape
    return make_params3f(w, h, d, a.ctypes.data, (a.strides[2] // 4, a.strides[1] // 4, a.strides[0] // 4),
                         b.ctypes.data, (b.strides[2] // 4, b.strides[1] // 4, b.strides[0] // 4), map_ptr)


def _ssim3f_host(handle, count, params, data_range, window, out):
    """rmgr_ssim_hip_compute_ssim3f_host, or -- a window given -- rmgr_ssim_hip_compute_ssim3f_win_host."""
    lib = load_library()
    if window is None:
        _check("rmgr_ssim_hip_compute_ssim3f_host", lib.rmgr_ssim_hip_compute_ssim3f_host(handle, count, params, data_range, out))
    else:
        _check("rmgr_ssim_hip_compute_ssim3f_win_host", lib.rmgr_ssim_hip_compute_ssim3f_win_host(handle, count, params, data_range, _window_ref(window), out))


def compute_ssim3f(a, b, data_range, want_map=False, ctx=None, window=None):
    """SSIM of two D x H x W float32 host volumes at `data_range` under the three-dimensional 11-tap window (any strides numpy can
    express, negative ones included) through rmgr_ssim_hip_compute_ssim3f_host; window (a Window, make_window): through
    rmgr_ssim_hip_compute_ssim3f_win_host under that window on all three axes.  Returns (float32 value, D x H x W float32 map or None)."""
    a, b = _f32_volume(a), _f32_volume(b)
    assert a.shape == b.shape
    m = np.empty(a.shape, np.float32) if want_map else None
    params = (Params3F * 1)()
    params[0] = _params3f_of(a, b, m.ctypes.data if want_map else None)
    out = (ctypes.c_float * 1)()
    _ssim3f_host(ctx.handle if ctx is not None else None, 1, params, data_range, window, out)
    return np.float32(out[0]), m


def compute_ssim3f_batch(pairs, data_range, ctx=None, window=None):
    """compute_ssim3f() of many host pairs of one size in one call (no maps): a float32 array."""
    pairs = [(_f32_volume(a), _f32_volume(b)) for a, b in pairs]
    n = len(pairs)
    params = (Params3F * max(n, 1))()
    for i, (a, b) in enumerate(pairs):
        params[i] = _params3f_of(a, b)
    out = (ctypes.c_float * max(n, 1))()
    _ssim3f_host(ctx.handle if ctx is not None else None, n, params, data_range, window, out)
    return np.array(out[:n], np.float32)


def sample_type_code(sample_type):
    """RMGR_SSIM_HIP_SAMPLE_F16 / _BF16 of "float16" / "bfloat16" (or of the code itself).  ValueError: anything else."""
    if isinstance(sample_type, str) and sample_type in _SAMPLE_TYPES:
        return _SAMPLE_TYPES[sample_type]
    if not isinstance(sample_type, (str, bool)) and sample_type in (SAMPLE_F16, SAMPLE_BF16):
        return int(sample_type)
    raise ValueError("sample_type must be 'float16' or 'bfloat16', got %r" % (sample_type,))


def _h_view(x, sample_type):
    """(host-byte-order uint16 view of an H x W array of 16-bit float samples, sample type code).  np.float16 arrays are float16;
    np.uint16 arrays hold the bit patterns of the encoding `sample_type` names (numpy has no bfloat16).  TypeError: another dtype, or a
    float16 array declared bfloat16; ValueError: a uint16 array without a sample_type, or an unknown one."""
    if not isinstance(x, np.ndarray) or x.ndim != 2:
        raise TypeError("H x W numpy array of float16 or uint16 expected")
    if x.dtype.kind == "f" and x.dtype.itemsize == 2:
        code = SAMPLE_F16 if sample_type is None else sample_type_code(sample_type)
        if code != SAMPLE_F16:
            raise TypeError("a float16 array cannot be read as bfloat16: pass the bit patterns as uint16")
        if not x.dtype.isnative:
            x = x.astype(np.float16)
        return _u16_view(x.view(np.uint16)), code
    if x.dtype.kind == "u" and x.dtype.itemsize == 2:
        if sample_type is None:
            raise ValueError("uint16 arrays need sample_type='bfloat16' or 'float16'")
        return _u16_view(x), sample_type_code(sample_type)
    raise TypeError("float16 or uint16 arrays expected, got %s" % x.dtype)


def _h_pair(a, b, sample_type):
    (a, ta), (b, tb) = _h_view(a, sample_type), _h_view(b, sample_type)
    if ta != tb:
        raise TypeError("the two images differ in sample type")
    if a.shape != b.shape:
        raise ValueError("shapes differ: %s and %s" % (a.shape, b.shape))
    return a, b, ta


def _ssimh_host(handle, count, params, code, data_range, window, out):
    """rmgr_ssim_hip_compute_ssimh_host, or -- a window given -- rmgr_ssim_hip_compute_ssimh_win_host."""
    lib = load_library()
    if window is None:
        _check("rmgr_ssim_hip_compute_ssimh_host", lib.rmgr_ssim_hip_compute_ssimh_host(handle, count, params, code, data_range, out))
    else:
        _check("rmgr_ssim_hip_compute_ssimh_win_host", lib.rmgr_ssim_hip_compute_ssimh_win_host(
            handle, count, params, code, data_range, _window_ref(window), out))


def compute_ssimh(a, b, data_range, sample_type=None, want_map=False, ctx=None, window=None):
    """SSIM of two H x W host arrays of float16 or bfloat16 samples at `data_range` (any strides numpy can express, negative ones
    included) through rmgr_ssim_hip_compute_ssimh_host; window (a Window, make_window): through rmgr_ssim_hip_compute_ssimh_win_host
    under that window.  np.float16 arrays select float16; np.uint16 arrays carry bit patterns and need sample_type="bfloat16" or
    "float16".  Returns (float32 value, H x W float32 map or None)."""
    if window is not None:
        _window_ref(window)
    a, b, code = _h_pair(a, b, sample_type)
    h, w = a.shape
    m = np.empty((h, w), np.float32) if want_map else None
    params = (Params16 * 1)()
    params[0] = _params16_of(a, b, m.ctypes.data if want_map else None)
    out = (ctypes.c_float * 1)()
    _ssimh_host(ctx.handle if ctx is not None else None, 1, params, code, data_range, window, out)
    return np.float32(out[0]), m


def compute_ssimh_batch(pairs, data_range, sample_type=None, ctx=None, window=None):
    """compute_ssimh() of many host pairs of one size and one sample type in one call (no maps): a float32 array."""
    if window is not None:
        _window_ref(window)
    pairs = [_h_pair(a, b, sample_type) for a, b in pairs]
    n = len(pairs)
    codes = set(t for _, _, t in pairs)
    if len(codes) > 1:
        raise TypeError("the pairs differ in sample type")
    code = codes.pop() if codes else sample_type_code("float16" if sample_type is None else sample_type)
    params = (Params16 * max(n, 1))()
    for i, (a, b, _) in enumerate(pairs):
        params[i] = _params16_of(a, b)
    out = (ctypes.c_float * max(n, 1))()
    _ssimh_host(ctx.handle if ctx is not None else None, n, params, code, data_range, window, out)
    return np.array(out[:n], np.float32)


def make_params3h(width, height, depth, a_ptr, a_strides, b_ptr, b_strides, map_ptr=None, map_strides=None):
    """rmgr_ssim_hip_Params3H; a_strides, b_strides: (step, stride, sliceStride) in 16-bit samples; map_strides: the same in floats
    (None: a dense depth x height x width map)."""
    p = Params3H()
    p.width, p.height, p.depth = width, height, depth
    p.imgA = Img3H(a_ptr, *a_strides)
    p.imgB = Img3H(b_ptr, *b_strides)
    p.ssimMap = map_ptr
    p.ssimStep, p.ssimStride, p.ssimSliceStride = (1, width, width * height) if map_strides is None else map_strides
    return p


def _h_volume(x, sample_type):
    """_h_view() of a D x H x W array: (host-byte-order uint16 view whose strides are whole samples, sample type code)."""
    if not isinstance(x, np.ndarray) or x.ndim != 3:
        raise TypeError("D x H x W numpy array of float16 or uint16 expected")
    if x.dtype.kind == "f" and x.dtype.itemsize == 2:
        code = SAMPLE_F16 if sample_type is None else sample_type_code(sample_type)
        if code != SAMPLE_F16:
            raise TypeError("a float16 array cannot be read as bfloat16: pass the bit patterns as uint16")
        x = (x if x.dtype.isnative else x.astype(np.float16)).view(np.uint16)
    elif x.dtype.kind == "u" and x.dtype.itemsize == 2:
        if sample_type is None:
            raise ValueError("uint16 arrays need sample_type='bfloat16' or 'float16'")
        code = sample_type_code(sample_type)
        if not x.dtype.isnative:
            x = x.astype(np.uint16)
    else:
        raise TypeError("float16 or uint16 arrays expected, got %s" % x.dtype)
    if any(s % 2 for s in x.strides) or x.ctypes.data % 2:
        x = np.ascontiguousarray(x)
    return x, code


def _h_volume_pair(a, b, sample_type):
    (a, ta), (b, tb) = _h_volume(a, sample_type), _h_volume(b, sample_type)
    if ta != tb:
        raise TypeError("the two volumes differ in sample type")
    if a.shape != b.shape:
        raise ValueError("shapes differ: %s and %s" % (a.shape, b.shape))
    return a, b, ta


def _params3h_of(a, b, map_ptr=None):
    d, h, w = a.shape
    return make_params3h(w, h, d, a.ctypes.data, (a.strides[2] // 2, a.strides[1] // 2, a.strides[0] // 2),
                         b.ctypes.data, (b.strides[2] // 2, b.strides[1] // 2, b.strides[0] // 2), map_ptr)


def _ssim3h_host(handle, count, params, code, data_range, window, out):
    """rmgr_ssim_hip_compute_ssim3h_host, or -- a window given -- rmgr_ssim_hip_compute_ssim3h_win_host."""
    lib = load_library()
    if window is None:
        _check("rmgr_ssim_hip_compute_ssim3h_host", lib.rmgr_ssim_hip_compute_ssim3h_host(handle, count, params, code, data_range, out))
    else:
        _check("rmgr_ssim_hip_compute_ssim3h_win_host", lib.rmgr_ssim_hip_compute_ssim3h_win_host(
            handle, count, params, code, data_range, _window_ref(window), out))


def compute_ssim3h(a, b, data_range, sample_type=None, want_map=False, ctx=None, window=None):
    """SSIM of two D x H x W host volumes of float16 or bfloat16 samples at `data_range` under the three-dimensional 11-tap window (any
    strides numpy can express, negative ones included) through rmgr_ssim_hip_compute_ssim3h_host; window (a Window, make_window): through
    rmgr_ssim_hip_compute_ssim3h_win_host under that window on all three axes.  Arrays and sample_type: as
    compute_ssimh (np.float16 arrays select float16; np.uint16 arrays carry bit patterns and need sample_type="bfloat16" or "float16").
    Returns (float32 value, D x H x W float32 map or None)."""
    a, b, code = _h_volume_pair(a, b, sample_type)
    m = np.empty(a.shape, np.float32) if want_map else None
    params = (Params3H * 1)()
    params[0] = _params3h_of(a, b, m.ctypes.data if want_map else None)
    out = (ctypes.c_float * 1)()
    _ssim3h_host(ctx.handle if ctx is not None else None, 1, params, code, data_range, window, out)
    return np.float32(out[0]), m


def compute_ssim3h_batch(pairs, data_range, sample_type=None, ctx=None, window=None):
    """compute_ssim3h() of many host pairs of one size and one sample type in one call (no maps): a float32 array."""
    pairs = [_h_volume_pair(a, b, sample_type) for a, b in pairs]
    n = len(pairs)
    codes = set(t for _, _, t in pairs)
    if len(codes) > 1:
        raise TypeError("the pairs differ in sample type")
    code = codes.pop() if codes else sample_type_code("float16" if sample_type is None else sample_type)
    params = (Params3H * max(n, 1))()
    for i, (a, b, _) in enumerate(pairs):
        params[i] = _params3h_of(a, b)
    out = (ctypes.c_float * max(n, 1))()
    _ssim3h_host(ctx.handle if ctx is not None else None, n, params, code, data_range, window, out)
    return np.array(out[:n], np.float32)


def _weights_array(weights):
    """The `weights` argument of the multi-scale entry points: NULL (Wang's five) or a double array."""
    if weights is None:
        return None
    return (ctypes.c_double * max(len(weights), 1))(*[float(x) for x in weights])


def _win_name(fn_name):
    """The name of the _win sibling of a multi-scale entry: rmgr_ssim_hip_compute_msssimf_host -> rmgr_ssim_hip_compute_msssimf_win_host."""
    for tail in ("_device", "_host", "_grad"):
        if fn_name.endswith(tail):
            return fn_name[:-len(tail)] + "_win" + tail
    return fn_name + "_win"


def _msssimf_call(fn_name, handle, params, count, data_range, scales, weights, per_scale, window=None):
    """window None: the entry fn_name; a Window: its _win sibling."""
    ref = _window_ref(window)
    out = (ctypes.c_float * max(count, 1))()
    means = (ctypes.c_double * max(count * scales * 2, 1))() if per_scale else None
    if ref is None:
        _check(fn_name, getattr(load_library(), fn_name)(handle, count, params, data_range, scales, _weights_array(weights), out, means))
    else:
        fn_name = _win_name(fn_name)
        _check(fn_name, getattr(load_library(), fn_name)(handle, count, params, data_range, ref, scales, _weights_array(weights), out, means))
    vals = np.array(out[:count], np.float32)
    if not per_scale:
        return vals
    return vals, np.array(means[:count * scales * 2], np.float64).reshape(count, scales, 2)


def compute_msssimf(a, b, data_range, scales=5, weights=None, per_scale=False, ctx=None, window=None):
    """Multi-scale SSIM of two H x W float32 host arrays at `data_range` (any strides numpy can express, negative ones included)
    through rmgr_ssim_hip_compute_msssimf_host; window (a Window, make_window): through rmgr_ssim_hip_compute_msssimf_win_host under that
    window at every scale.  weights None: Wang's five (scales must be 5).  Returns a float32, and with per_scale=True also a (scales, 2)
    float64 array of [scale]{mcs, mssim}.  TypeError: a window that is neither None nor a Window."""
    a, b = _f32_view(a), _f32_view(b)
    assert a.shape == b.shape
    params = (ParamsF * 1)()
    params[0] = _params_f_of(a, b)
    r = _msssimf_call("rmgr_ssim_hip_compute_msssimf_host", ctx.handle if ctx is not None else None, params, 1, data_range, scales, weights, per_scale,
                      window)
    return (r[0][0], r[1][0]) if per_scale else r[0]


def compute_msssimf_batch(pairs, data_range, scales=5, weights=None, per_scale=False, ctx=None, window=None):
    """compute_msssimf() of many host pairs of one size in one call: a float32 array (and a (count, scales, 2) array with per_scale)."""
    pairs = [(_f32_view(a), _f32_view(b)) for a, b in pairs]
    n = len(pairs)
    params = (ParamsF * max(n, 1))()
    for i, (a, b) in enumerate(pairs):
        params[i] = _params_f_of(a, b)
    return _msssimf_call("rmgr_ssim_hip_compute_msssimf_host", ctx.handle if ctx is not None else None, params, n, data_range, scales, weights, per_scale,
                         window)


def compute_msssim3f(a, b, data_range, scales=5, weights=None, per_scale=False, ctx=None, window=None):
    """Multi-scale SSIM of two D x H x W float32 host volumes at `data_range` (any strides numpy can express, negative ones included)
    through rmgr_ssim_hip_compute_msssim3f_host: the 11-tap window on all three axes, all three axes halved from scale to scale; window (a
    Window, make_window): through rmgr_ssim_hip_compute_msssim3f_win_host under that window on all three axes at every scale.  weights
    None: Wang's five (scales must be 5).  Returns a float32, and with per_scale=True also a (scales, 2) float64 array of
    [scale]{mcs, mssim}.  TypeError: a window that is neither None nor a Window."""
    a, b = _f32_volume(a), _f32_volume(b)
    assert a.shape == b.shape
    params = (Params3F * 1)()
    params[0] = _params3f_of(a, b)
    r = _msssimf_call("rmgr_ssim_hip_compute_msssim3f_host", ctx.handle if ctx is not None else None, params, 1, data_range, scales, weights, per_scale,
                      window)
    return (r[0][0], r[1][0]) if per_scale else r[0]


def compute_msssim3f_batch(pairs, data_range, scales=5, weights=None, per_scale=False, ctx=None, window=None):
    """compute_msssim3f() of many host pairs of one size in one call: a float32 array (and a (count, scales, 2) array with per_scale)."""
    pairs = [(_f32_volume(a), _f32_volume(b)) for a, b in pairs]
    n = len(pairs)
    params = (Params3F * max(n, 1))()
    for i, (a, b) in enumerate(pairs):
        params[i] = _params3f_of(a, b)
    return _msssimf_call("rmgr_ssim_hip_compute_msssim3f_host", ctx.handle if ctx is not None else None, params, n, data_range, scales, weights, per_scale,
                         window)


def _msssimh_call(fn_name, handle, params, count, code, data_range, scales, weights, per_scale, window=None):
    """window None: the entry fn_name; a Window: its _win sibling."""
    ref = _window_ref(window)
    out = (ctypes.c_float * max(count, 1))()
    means = (ctypes.c_double * max(count * scales * 2, 1))() if per_scale else None
    if ref is None:
        _check(fn_name, getattr(load_library(), fn_name)(handle, count, params, code, data_range, scales, _weights_array(weights), out, means))
    else:
        fn_name = _win_name(fn_name)
        _check(fn_name, getattr(load_library(), fn_name)(handle, count, params, code, data_range, ref, scales, _weights_array(weights), out, means))
    vals = np.array(out[:count], np.float32)
    if not per_scale:
        return vals
    return vals, np.array(means[:count * scales * 2], np.float64).reshape(count, scales, 2)


def compute_msssimh(a, b, data_range, sample_type=None, scales=5, weights=None, per_scale=False, ctx=None, window=None):
    """Multi-scale SSIM of two H x W host arrays of float16 or bfloat16 samples at `data_range` (any strides numpy can express, negative
    ones included) through rmgr_ssim_hip_compute_msssimh_host; window (a Window, make_window): through
    rmgr_ssim_hip_compute_msssimh_win_host under that window at every scale.  Arrays and sample_type: as compute_ssimh (np.float16 arrays select
    float16; np.uint16 arrays carry bit patterns and need sample_type), with its errors.  weights None: Wang's five (scales must be 5).
    Returns a float32, and with per_scale=True also a (scales, 2) float64 array of [scale]{mcs, mssim}."""
    a, b, code = _h_pair(a, b, sample_type)
    params = (Params16 * 1)()
    params[0] = _params16_of(a, b)
    r = _msssimh_call("rmgr_ssim_hip_compute_msssimh_host", ctx.handle if ctx is not None else None, params, 1, code, data_range, scales, weights, per_scale,
                      window)
    return (r[0][0], r[1][0]) if per_scale else r[0]


def compute_msssimh_batch(pairs, data_range, sample_type=None, scales=5, weights=None, per_scale=False, ctx=None, window=None):
    """compute_msssimh() of many host pairs of one size and one sample type in one call: a float32 array (and a (count, scales, 2) array
    with per_scale)."""
    pairs = [_h_pair(a, b, sample_type) for a, b in pairs]
    n = len(pairs)
    codes = set(t for _, _, t in pairs)
    if len(codes) > 1:
        raise TypeError("the pairs differ in sample type")
    code = codes.pop() if codes else sample_type_code("float16" if sample_type is None else sample_type)
    params = (Params16 * max(n, 1))()
    for i, (a, b, _) in enumerate(pairs):
        params[i] = _params16_of(a, b)
    return _msssimh_call("rmgr_ssim_hip_compute_msssimh_host", ctx.handle if ctx is not None else None, params, n, code, data_range, scales, weights, per_scale,
                         window)


def compute_msssim3h(a, b, data_range, sample_type=None, scales=5, weights=None, per_scale=False, ctx=None, window=None):
    """Multi-scale SSIM of two D x H x W host volumes of float16 or bfloat16 samples at `data_range` (any strides numpy can express,
    negative ones included) through rmgr_ssim_hip_compute_msssim3h_host; window (a Window, make_window): through
    rmgr_ssim_hip_compute_msssim3h_win_host under that window at every scale.  Arrays and sample_type: as compute_ssim3h (np.float16 arrays
    select float16; np.uint16 arrays carry bit patterns and need sample_type), with its errors.  weights None: Wang's five (scales must be
    5).  Returns a float32, and with per_scale=True also a (scales, 2) float64 array of [scale]{mcs, mssim}."""
    a, b, code = _h_volume_pair(a, b, sample_type)
    params = (Params3H * 1)()
    params[0] = _params3h_of(a, b)
    r = _msssimh_call("rmgr_ssim_hip_compute_msssim3h_host", ctx.handle if ctx is not None else None, params, 1, code, data_range, scales, weights, per_scale,
                      window)
    return (r[0][0], r[1][0]) if per_scale else r[0]


def compute_msssim3h_batch(pairs, data_range, sample_type=None, scales=5, weights=None, per_scale=False, ctx=None, window=None):
    """compute_msssim3h() of many host pairs of one size and one sample type in one call: a float32 array (and a (count, scales, 2) array
    with per_scale)."""
    pairs = [_h_volume_pair(a, b, sample_type) for a, b in pairs]
    n = len(pairs)
    codes = set(t for _, _, t in pairs)
    if len(codes) > 1:
        raise TypeError("the pairs differ in sample type")
    code = codes.pop() if codes else sample_type_code("float16" if sample_type is None else sample_type)
    params = (Params3H * max(n, 1))()
    for i, (a, b, _) in enumerate(pairs):
        params[i] = _params3h_of(a, b)
    return _msssimh_call("rmgr_ssim_hip_compute_msssim3h_host", ctx.handle if ctx is not None else None, params, n, code, data_range, scales, weights, per_scale,
                         window)


class DeviceBuffer(object):
    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        p = ctypes.c_void_p()
        _check("rmgr_ssim_hip_malloc", ctx.lib.rmgr_ssim_hip_malloc(ctx.handle, ctypes.byref(p), nbytes))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _check("rmgr_ssim_hip_memcpy_h2d", self.ctx.lib.rmgr_ssim_hip_memcpy_h2d(self.ctx.handle, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        _check("rmgr_ssim_hip_memcpy_d2h", self.ctx.lib.rmgr_ssim_hip_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.rmgr_ssim_hip_free(self.ctx.handle, self.ptr)
            self.ptr = None


class Context(object):
    """rmgr_ssim_hip_Context: one engine bound to one device and one stream."""

    def __init__(self, device=0, stream=None, mode=MODE_EXACT):
        self.lib = load_library()
        h = ctypes.c_void_p()
        _check("rmgr_ssim_hip_create", self.lib.rmgr_ssim_hip_create(ctypes.byref(h), device, stream))
        self.handle = h
        self.set_mode(mode)

    def close(self):
        if self.handle:
            self.lib.rmgr_ssim_hip_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def describe(self):
        return self.lib.rmgr_ssim_hip_describe(self.handle).decode()

    def set_mode(self, mode):
        _check("rmgr_ssim_hip_set_mode", self.lib.rmgr_ssim_hip_set_mode(self.handle, mode))

    def tune(self, width, height, count, with_map=False):
        """Times the candidate plans of this launch shape on the device and keeps the winner for this context (rmgr_ssim_hip_tune).
        Returns {"default_ms", "best_ms", "best": (variant, strip_rows), "candidates": [(variant, strip_rows, ms), ...]} (candidates[0]: the default)."""
        r = TuneResult()
        r.structSize = ctypes.sizeof(TuneResult)
        _check("rmgr_ssim_hip_tune", self.lib.rmgr_ssim_hip_tune(self.handle, width, height, count, 1 if with_map else 0, ctypes.byref(r)))
        return {"default_ms": r.defaultMs, "best_ms": r.bestMs, "best": (r.bestVariant, r.bestStripRows),
                "candidates": [(r.candidateVariant[i], r.candidateStripRows[i], r.candidateMs[i]) for i in range(min(r.candidates, 8))]}

    def clear_tuned(self):
        _check("rmgr_ssim_hip_clear_tuned", self.lib.rmgr_ssim_hip_clear_tuned(self.handle))

    def tuned(self):
        """The measured choices the context holds: [(width, height, count, with_map, mode, variant, strip_rows), ...] (rmgr_ssim_hip_get_tuned)."""
        out, e = [], TunedEntry()
        while True:
            rc = self.lib.rmgr_ssim_hip_get_tuned(self.handle, len(out), ctypes.byref(e))
            if rc == errno.ENOENT:
                return out
            _check("rmgr_ssim_hip_get_tuned", rc)
            out.append((e.width, e.height, e.count, bool(e.withMap), e.mode, e.variant, e.stripRows))

    def set_tuned(self, width, height, count, with_map, variant, strip_rows):
        """Installs a choice for a launch shape under the context's current mode without measuring (rmgr_ssim_hip_set_tuned)."""
        _check("rmgr_ssim_hip_set_tuned", self.lib.rmgr_ssim_hip_set_tuned(self.handle, width, height, count, 1 if with_map else 0, variant, strip_rows))

    def trim(self):
        """Gives the context's grow-only staging back to the system (rmgr_ssim_hip_trim)."""
        _check("rmgr_ssim_hip_trim", self.lib.rmgr_ssim_hip_trim(self.handle))

    def set_tuning(self, strip_rows=0, variant=0):
        _check("rmgr_ssim_hip_set_tuning", self.lib.rmgr_ssim_hip_set_tuning(self.handle, strip_rows, variant))

    def alloc(self, nbytes):
        return DeviceBuffer(self, max(int(nbytes), 1))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        return self.alloc(arr.nbytes).upload(arr)

    def download(self, ptr, dtype, shape):
        """Copy device memory at `ptr` into a new numpy array (blocking)."""
        out = np.empty(shape, dtype)
        _check("rmgr_ssim_hip_memcpy_d2h", self.lib.rmgr_ssim_hip_memcpy_d2h(self.handle, out.ctypes.data, ptr, out.nbytes))
        return out

    def synchronize(self):
        _check("rmgr_ssim_hip_synchronize", self.lib.rmgr_ssim_hip_synchronize(self.handle))

    def compute_host(self, params, want_global=True, thread_pool=None):
        out = ctypes.c_float()
        rc = self.lib.rmgr_ssim_hip_compute_ssim_host(self.handle, ctypes.byref(out) if want_global else None,
                                                      ctypes.byref(params), thread_pool)
        _check("rmgr_ssim_hip_compute_ssim_host", rc)
        return np.float32(out.value)

    def compute_device(self, params, want_global=True):
        out = ctypes.c_float()
        rc = self.lib.rmgr_ssim_hip_compute_ssim_device(self.handle, ctypes.byref(out) if want_global else None, ctypes.byref(params))
        _check("rmgr_ssim_hip_compute_ssim_device", rc)
        return np.float32(out.value)

    def msssim_device(self, params_array, count, scales=5, weights=None, per_scale=False):
        """MS-SSIM of `count` device-resident pairs (a Params array) through rmgr_ssim_hip_compute_msssim_device: a float32 array,
        and with per_scale=True also a (count, scales, 2) float64 array of [image][scale]{mcs, mssim}."""
        return _msssim_call("rmgr_ssim_hip_compute_msssim_device", self.handle, params_array, count, scales, weights, per_scale)

    def ssim16_device(self, params_array, count, bit_depth):
        """SSIM of `count` device-resident uint16 pairs (a Params16 array) through rmgr_ssim_hip_compute_ssim16_device: a float32 array."""
        out = (ctypes.c_float * max(count, 1))()
        _check("rmgr_ssim_hip_compute_ssim16_device", self.lib.rmgr_ssim_hip_compute_ssim16_device(self.handle, count, params_array, bit_depth, out))
        return np.array(out[:count], np.float32)

    def enqueue_ssim16(self, params_array, count, bit_depth, sums_dev_ptr):
        """rmgr_ssim_hip_enqueue_ssim16: per-pair fp64 sums into device memory, asynchronously on the context's stream."""
        _check("rmgr_ssim_hip_enqueue_ssim16", self.lib.rmgr_ssim_hip_enqueue_ssim16(self.handle, count, params_array, bit_depth, sums_dev_ptr))

    # The float32 family takes window=None (the engine's 11-tap Gaussian of sigma 1.5: the entry without _win) or a Window
    # (make_window): the _win entry under that window.

    def ssimf_device(self, params_array, count, data_range, window=None):
        """SSIM of `count` device-resident float32 pairs (a ParamsF array) through rmgr_ssim_hip_compute_ssimf_device (window: _win_device):
        a float32 array."""
        out = (ctypes.c_float * max(count, 1))()
        if window is None:
            _check("rmgr_ssim_hip_compute_ssimf_device", self.lib.rmgr_ssim_hip_compute_ssimf_device(self.handle, count, params_array, data_range, out))
        else:
            _check("rmgr_ssim_hip_compute_ssimf_win_device", self.lib.rmgr_ssim_hip_compute_ssimf_win_device(
                self.handle, count, params_array, data_range, _window_ref(window), out))
        return np.array(out[:count], np.float32)

    def enqueue_ssimf(self, params_array, count, data_range, sums_dev_ptr, window=None):
        """rmgr_ssim_hip_enqueue_ssimf (window: _ssimf_win): per-pair fp64 sums into device memory, asynchronously on the context's stream."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssimf", self.lib.rmgr_ssim_hip_enqueue_ssimf(self.handle, count, params_array, data_range, sums_dev_ptr))
        else:
            _check("rmgr_ssim_hip_enqueue_ssimf_win", self.lib.rmgr_ssim_hip_enqueue_ssimf_win(
                self.handle, count, params_array, data_range, _window_ref(window), sums_dev_ptr))

    def enqueue_ssimf_grad(self, params_array, count, data_range, grad_out_dev_ptr, grad_a=None, grad_b=None, window=None):
        """rmgr_ssim_hip_enqueue_ssimf_grad (window: _ssimf_win_grad): dLoss/dA and / or dLoss/dB of `count` device-resident pairs into the
        planes the GradF arrays grad_a / grad_b describe (None: not wanted), from `count` floats dLoss/dS_i in device memory; asynchronous,
        written not accumulated."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssimf_grad", self.lib.rmgr_ssim_hip_enqueue_ssimf_grad(self.handle, count, params_array, data_range, grad_out_dev_ptr, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_ssimf_win_grad", self.lib.rmgr_ssim_hip_enqueue_ssimf_win_grad(
                self.handle, count, params_array, data_range, _window_ref(window), grad_out_dev_ptr, grad_a, grad_b))

    # The float32 volume family takes window=None (the engine's 11-tap Gaussian of sigma 1.5: the entry without _win) or a Window
    # (make_window): the _win entry under that window on all three axes.

    def ssim3f_device(self, params_array, count, data_range, window=None):
        """SSIM of `count` device-resident pairs of float32 volumes (a Params3F array) under the three-dimensional window through
        rmgr_ssim_hip_compute_ssim3f_device (window: _ssim3f_win_device): a float32 array."""
        out = (ctypes.c_float * max(count, 1))()
        if window is None:
            _check("rmgr_ssim_hip_compute_ssim3f_device", self.lib.rmgr_ssim_hip_compute_ssim3f_device(self.handle, count, params_array, data_range, out))
        else:
            _check("rmgr_ssim_hip_compute_ssim3f_win_device", self.lib.rmgr_ssim_hip_compute_ssim3f_win_device(
                self.handle, count, params_array, data_range, _window_ref(window), out))
        return np.array(out[:count], np.float32)

    def enqueue_ssim3f(self, params_array, count, data_range, sums_dev_ptr, window=None):
        """rmgr_ssim_hip_enqueue_ssim3f (window: _ssim3f_win): per-pair fp64 sums into device memory, asynchronously on the context's stream."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssim3f", self.lib.rmgr_ssim_hip_enqueue_ssim3f(self.handle, count, params_array, data_range, sums_dev_ptr))
        else:
            _check("rmgr_ssim_hip_enqueue_ssim3f_win", self.lib.rmgr_ssim_hip_enqueue_ssim3f_win(
                self.handle, count, params_array, data_range, _window_ref(window), sums_dev_ptr))

    def enqueue_ssim3f_grad(self, params_array, count, data_range, grad_out_dev_ptr, grad_a=None, grad_b=None, window=None):
        """rmgr_ssim_hip_enqueue_ssim3f_grad (window: _ssim3f_win_grad): dLoss/dA and / or dLoss/dB of `count` device-resident pairs of volumes into the volumes the
        Grad3F arrays grad_a / grad_b describe (None: not wanted), from `count` floats dLoss/dS_i in device memory; asynchronous, written
        not accumulated."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssim3f_grad", self.lib.rmgr_ssim_hip_enqueue_ssim3f_grad(self.handle, count, params_array, data_range, grad_out_dev_ptr, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_ssim3f_win_grad", self.lib.rmgr_ssim_hip_enqueue_ssim3f_win_grad(
                self.handle, count, params_array, data_range, _window_ref(window), grad_out_dev_ptr, grad_a, grad_b))

    # The 16-bit family takes window=None (the engine's 11-tap Gaussian of sigma 1.5: the entry without _win) or a Window (make_window):
    # the _win entry under that window.

    def ssimh_device(self, params_array, count, data_range, sample_type, window=None):
        """SSIM of `count` device-resident float16 / bfloat16 pairs (a Params16 array) through rmgr_ssim_hip_compute_ssimh_device
        (window: _ssimh_win_device): a float32 array."""
        out = (ctypes.c_float * max(count, 1))()
        if window is None:
            _check("rmgr_ssim_hip_compute_ssimh_device", self.lib.rmgr_ssim_hip_compute_ssimh_device(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, out))
        else:
            _check("rmgr_ssim_hip_compute_ssimh_win_device", self.lib.rmgr_ssim_hip_compute_ssimh_win_device(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), out))
        return np.array(out[:count], np.float32)

    def enqueue_ssim3f_map_grad(self, params_array, count, data_range, grad_out_maps, grad_a=None, grad_b=None, window=None):
        """rmgr_ssim_hip_enqueue_ssim3f_map_grad (window: _ssim3f_win_map_grad): dLoss/dA and / or dLoss/dB of `count` device-resident pairs of volumes for a per-voxel
        upstream gradient: grad_out_maps is a GradOut3F array of `count` float32 volumes dLoss/dssim_i(p) in device memory (any step /
        stride / sliceStride, 0 included); asynchronous, written not accumulated."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssim3f_map_grad", self.lib.rmgr_ssim_hip_enqueue_ssim3f_map_grad(
                self.handle, count, params_array, data_range, grad_out_maps, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_ssim3f_win_map_grad", self.lib.rmgr_ssim_hip_enqueue_ssim3f_win_map_grad(
                self.handle, count, params_array, data_range, _window_ref(window), grad_out_maps, grad_a, grad_b))

    # The 16-bit volume family takes window=None (the engine's 11-tap Gaussian of sigma 1.5: the entry without _win) or a Window
    # (make_window): the _win entry under that window on all three axes.

    def ssim3h_device(self, params_array, count, data_range, sample_type, window=None):
        """SSIM of `count` device-resident pairs of float16 / bfloat16 volumes (a Params3H array) under the three-dimensional window
        through rmgr_ssim_hip_compute_ssim3h_device (window: _ssim3h_win_device): a float32 array."""
        out = (ctypes.c_float * count)()
        if window is None:
            _check("rmgr_ssim_hip_compute_ssim3h_device", self.lib.rmgr_ssim_hip_compute_ssim3h_device(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, out))
        else:
            _check("rmgr_ssim_hip_compute_ssim3h_win_device", self.lib.rmgr_ssim_hip_compute_ssim3h_win_device(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), out))
        return np.array(out[:], np.float32)

    def enqueue_ssim3h(self, params_array, count, data_range, sample_type, sums_dev_ptr, window=None):
        """rmgr_ssim_hip_enqueue_ssim3h (window: _ssim3h_win): per-pair fp64 sums into device memory, asynchronously on the context's stream."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssim3h", self.lib.rmgr_ssim_hip_enqueue_ssim3h(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, sums_dev_ptr))
        else:
            _check("rmgr_ssim_hip_enqueue_ssim3h_win", self.lib.rmgr_ssim_hip_enqueue_ssim3h_win(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), sums_dev_ptr))

    def enqueue_ssim3h_grad(self, params_array, count, data_range, sample_type, grad_out_dev_ptr, grad_a=None, grad_b=None, window=None):
        """rmgr_ssim_hip_enqueue_ssim3h_grad (window: _ssim3h_win_grad): dLoss/dA and / or dLoss/dB of `count` device-resident pairs of
        volumes into the 16-bit volumes the Grad3H arrays describe, in the inputs' encoding; grad_out_dev_ptr: count float32 values;
        asynchronous, written not accumulated."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssim3h_grad", self.lib.rmgr_ssim_hip_enqueue_ssim3h_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, grad_out_dev_ptr, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_ssim3h_win_grad", self.lib.rmgr_ssim_hip_enqueue_ssim3h_win_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), grad_out_dev_ptr, grad_a, grad_b))

    def enqueue_ssim3h_map_grad(self, params_array, count, data_range, sample_type, grad_out_maps, grad_a=None, grad_b=None, window=None):
        """rmgr_ssim_hip_enqueue_ssim3h_map_grad (window: _ssim3h_win_map_grad): the same for a per-voxel upstream gradient: grad_out_maps
        is a GradOut3F array of `count` float32 volumes dLoss/dssim_i(p) in device memory (any step / stride / sliceStride in floats, 0
        allowed)."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssim3h_map_grad", self.lib.rmgr_ssim_hip_enqueue_ssim3h_map_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, grad_out_maps, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_ssim3h_win_map_grad", self.lib.rmgr_ssim_hip_enqueue_ssim3h_win_map_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), grad_out_maps, grad_a, grad_b))

    def enqueue_ssimh(self, params_array, count, data_range, sample_type, sums_dev_ptr, window=None):
        """rmgr_ssim_hip_enqueue_ssimh (window: _ssimh_win): per-pair fp64 sums into device memory, asynchronously on the context's stream."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssimh", self.lib.rmgr_ssim_hip_enqueue_ssimh(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, sums_dev_ptr))
        else:
            _check("rmgr_ssim_hip_enqueue_ssimh_win", self.lib.rmgr_ssim_hip_enqueue_ssimh_win(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), sums_dev_ptr))

    def enqueue_ssimh_grad(self, params_array, count, data_range, sample_type, grad_out_dev_ptr, grad_a=None, grad_b=None, window=None):
        """rmgr_ssim_hip_enqueue_ssimh_grad (window: _ssimh_win_grad): dLoss/dA and / or dLoss/dB of `count` device-resident pairs into the
        16-bit planes the GradH arrays describe, in the inputs' encoding; grad_out_dev_ptr: count float32 values; asynchronous, no host
        synchronisation."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssimh_grad", self.lib.rmgr_ssim_hip_enqueue_ssimh_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, grad_out_dev_ptr, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_ssimh_win_grad", self.lib.rmgr_ssim_hip_enqueue_ssimh_win_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), grad_out_dev_ptr, grad_a, grad_b))

    def enqueue_ssimf_map_grad(self, params_array, count, data_range, grad_out_maps, grad_a=None, grad_b=None, window=None):
        """rmgr_ssim_hip_enqueue_ssimf_map_grad (window: _ssimf_win_map_grad): dLoss/dA and / or dLoss/dB of `count` device-resident pairs for a per-pixel upstream
        gradient: grad_out_maps is a GradOutF array of `count` float32 planes dLoss/dssim_i(p) in device memory (any step / stride, 0
        included); asynchronous, written not accumulated."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssimf_map_grad", self.lib.rmgr_ssim_hip_enqueue_ssimf_map_grad(
                self.handle, count, params_array, data_range, grad_out_maps, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_ssimf_win_map_grad", self.lib.rmgr_ssim_hip_enqueue_ssimf_win_map_grad(
                self.handle, count, params_array, data_range, _window_ref(window), grad_out_maps, grad_a, grad_b))

    def enqueue_ssimh_map_grad(self, params_array, count, data_range, sample_type, grad_out_maps, grad_a=None, grad_b=None, window=None):
        """rmgr_ssim_hip_enqueue_ssimh_map_grad (window: _ssimh_win_map_grad): the same for float16 / bfloat16 pairs (a Params16 array); the
        GradH planes receive the float32 value rounded once into the inputs' encoding; the GradOutF planes stay float32."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_ssimh_map_grad", self.lib.rmgr_ssim_hip_enqueue_ssimh_map_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, grad_out_maps, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_ssimh_win_map_grad", self.lib.rmgr_ssim_hip_enqueue_ssimh_win_map_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), grad_out_maps, grad_a, grad_b))

    def msssimf_device(self, params_array, count, data_range, scales=5, weights=None, per_scale=False, window=None):
        """MS-SSIM of `count` device-resident float32 pairs (a ParamsF array) through rmgr_ssim_hip_compute_msssimf_device (window:
        _msssimf_win_device): a float32 array, and with per_scale=True also a (count, scales, 2) float64 array of
        [pair][scale]{mcs, mssim}."""
        return _msssimf_call("rmgr_ssim_hip_compute_msssimf_device", self.handle, params_array, count, data_range, scales, weights, per_scale, window)

    def enqueue_msssimf(self, params_array, count, data_range, values_dev_ptr, means_dev_ptr, scales=5, weights=None, window=None):
        """rmgr_ssim_hip_enqueue_msssimf (window: _msssimf_win): per-pair fp64 values and count x scales x 2 fp64 means into device memory,
        asynchronously on the context's stream."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_msssimf", self.lib.rmgr_ssim_hip_enqueue_msssimf(
                self.handle, count, params_array, data_range, scales, _weights_array(weights), values_dev_ptr, means_dev_ptr))
        else:
            _check("rmgr_ssim_hip_enqueue_msssimf_win", self.lib.rmgr_ssim_hip_enqueue_msssimf_win(
                self.handle, count, params_array, data_range, _window_ref(window), scales, _weights_array(weights), values_dev_ptr, means_dev_ptr))

    def enqueue_msssimf_grad(self, params_array, count, data_range, means_dev_ptr, grad_out_dev_ptr, grad_a=None, grad_b=None, scales=5, weights=None,
                             window=None):
        """rmgr_ssim_hip_enqueue_msssimf_grad (window: _msssimf_win_grad): dLoss/dA and / or dLoss/dB of `count` device-resident pairs, from the forward's means
        (device memory), into the planes the GradF arrays describe; asynchronous on the context's stream, no host synchronisation."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_msssimf_grad", self.lib.rmgr_ssim_hip_enqueue_msssimf_grad(
                self.handle, count, params_array, data_range, scales, _weights_array(weights), means_dev_ptr, grad_out_dev_ptr, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_msssimf_win_grad", self.lib.rmgr_ssim_hip_enqueue_msssimf_win_grad(
                self.handle, count, params_array, data_range, _window_ref(window), scales, _weights_array(weights), means_dev_ptr, grad_out_dev_ptr,
                grad_a, grad_b))

    def msssim3f_device(self, params_array, count, data_range, scales=5, weights=None, per_scale=False, window=None):
        """MS-SSIM of `count` device-resident pairs of float32 volumes (a Params3F array) through rmgr_ssim_hip_compute_msssim3f_device
        (window: _msssim3f_win_device): a float32 array, and with per_scale=True also a (count, scales, 2) float64 array of
        [pair][scale]{mcs, mssim}."""
        return _msssimf_call("rmgr_ssim_hip_compute_msssim3f_device", self.handle, params_array, count, data_range, scales, weights, per_scale, window)

    def enqueue_msssim3f(self, params_array, count, data_range, values_dev_ptr, means_dev_ptr, scales=5, weights=None, window=None):
        """rmgr_ssim_hip_enqueue_msssim3f (window: _msssim3f_win): per-pair fp64 values and count x scales x 2 fp64 means into device memory,
        asynchronously on the context's stream."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_msssim3f", self.lib.rmgr_ssim_hip_enqueue_msssim3f(
                self.handle, count, params_array, data_range, scales, _weights_array(weights), values_dev_ptr, means_dev_ptr))
        else:
            _check("rmgr_ssim_hip_enqueue_msssim3f_win", self.lib.rmgr_ssim_hip_enqueue_msssim3f_win(
                self.handle, count, params_array, data_range, _window_ref(window), scales, _weights_array(weights), values_dev_ptr, means_dev_ptr))

    def enqueue_msssim3f_grad(self, params_array, count, data_range, means_dev_ptr, grad_out_dev_ptr, grad_a=None, grad_b=None, scales=5, weights=None,
                              window=None):
        """rmgr_ssim_hip_enqueue_msssim3f_grad (window: _msssim3f_win_grad): dLoss/dA and / or dLoss/dB of `count` device-resident pairs of
        volumes, from the forward's means (device memory), into the volumes the Grad3F arrays describe; asynchronous on the context's
        stream, no host synchronisation."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_msssim3f_grad", self.lib.rmgr_ssim_hip_enqueue_msssim3f_grad(
                self.handle, count, params_array, data_range, scales, _weights_array(weights), means_dev_ptr, grad_out_dev_ptr, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_msssim3f_win_grad", self.lib.rmgr_ssim_hip_enqueue_msssim3f_win_grad(
                self.handle, count, params_array, data_range, _window_ref(window), scales, _weights_array(weights), means_dev_ptr, grad_out_dev_ptr,
                grad_a, grad_b))

    def msssimh_device(self, params_array, count, data_range, sample_type, scales=5, weights=None, per_scale=False, window=None):
        """MS-SSIM of `count` device-resident float16 / bfloat16 pairs (a Params16 array) through rmgr_ssim_hip_compute_msssimh_device
        (window: _msssimh_win_device): a float32 array, and with per_scale=True also a (count, scales, 2) float64 array of
        [pair][scale]{mcs, mssim}."""
        return _msssimh_call("rmgr_ssim_hip_compute_msssimh_device", self.handle, params_array, count, sample_type_code(sample_type), data_range,
                             scales, weights, per_scale, window)

    def enqueue_msssimh(self, params_array, count, data_range, sample_type, values_dev_ptr, means_dev_ptr, scales=5, weights=None, window=None):
        """rmgr_ssim_hip_enqueue_msssimh (window: _msssimh_win): per-pair fp64 values and count x scales x 2 fp64 means into device memory,
        asynchronously on the context's stream."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_msssimh", self.lib.rmgr_ssim_hip_enqueue_msssimh(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, scales, _weights_array(weights), values_dev_ptr, means_dev_ptr))
        else:
            _check("rmgr_ssim_hip_enqueue_msssimh_win", self.lib.rmgr_ssim_hip_enqueue_msssimh_win(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), scales, _weights_array(weights),
                values_dev_ptr, means_dev_ptr))

    def enqueue_msssimh_grad(self, params_array, count, data_range, sample_type, means_dev_ptr, grad_out_dev_ptr, grad_a=None, grad_b=None, scales=5,
                             weights=None, window=None):
        """rmgr_ssim_hip_enqueue_msssimh_grad (window: _msssimh_win_grad): dLoss/dA and / or dLoss/dB of `count` device-resident pairs, from the forward's means (device
        memory), into the 16-bit planes the GradH arrays describe, in the inputs' encoding; grad_out_dev_ptr: count float32 values;
        asynchronous on the context's stream, no host synchronisation."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_msssimh_grad", self.lib.rmgr_ssim_hip_enqueue_msssimh_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, scales, _weights_array(weights), means_dev_ptr,
                grad_out_dev_ptr, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_msssimh_win_grad", self.lib.rmgr_ssim_hip_enqueue_msssimh_win_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), scales, _weights_array(weights),
                means_dev_ptr, grad_out_dev_ptr, grad_a, grad_b))

    def msssim3h_device(self, params_array, count, data_range, sample_type, scales=5, weights=None, per_scale=False, window=None):
        """MS-SSIM of `count` device-resident pairs of float16 / bfloat16 volumes (a Params3H array) through
        rmgr_ssim_hip_compute_msssim3h_device (window: _msssim3h_win_device): a float32 array, and with per_scale=True also a
        (count, scales, 2) float64 array."""
        return _msssimh_call("rmgr_ssim_hip_compute_msssim3h_device", self.handle, params_array, count, sample_type_code(sample_type), data_range,
                             scales, weights, per_scale, window)

    def enqueue_msssim3h(self, params_array, count, data_range, sample_type, values_dev_ptr, means_dev_ptr, scales=5, weights=None, window=None):
        """rmgr_ssim_hip_enqueue_msssim3h (window: _msssim3h_win): per-pair fp64 values and count x scales x 2 fp64 means into device memory,
        asynchronously on the context's stream."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_msssim3h", self.lib.rmgr_ssim_hip_enqueue_msssim3h(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, scales, _weights_array(weights), values_dev_ptr, means_dev_ptr))
        else:
            _check("rmgr_ssim_hip_enqueue_msssim3h_win", self.lib.rmgr_ssim_hip_enqueue_msssim3h_win(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), scales, _weights_array(weights),
                values_dev_ptr, means_dev_ptr))

    def enqueue_msssim3h_grad(self, params_array, count, data_range, sample_type, means_dev_ptr, grad_out_dev_ptr, grad_a=None, grad_b=None, scales=5,
                              weights=None, window=None):
        """rmgr_ssim_hip_enqueue_msssim3h_grad (window: _msssim3h_win_grad): dLoss/dA and / or dLoss/dB of `count` device-resident pairs of
        volumes, from the forward's means (device memory), into the 16-bit volumes the Grad3H arrays describe, in the inputs' encoding;
        grad_out_dev_ptr: count float32 values; asynchronous on the context's stream, no host synchronisation."""
        if window is None:
            _check("rmgr_ssim_hip_enqueue_msssim3h_grad", self.lib.rmgr_ssim_hip_enqueue_msssim3h_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, scales, _weights_array(weights), means_dev_ptr,
                grad_out_dev_ptr, grad_a, grad_b))
        else:
            _check("rmgr_ssim_hip_enqueue_msssim3h_win_grad", self.lib.rmgr_ssim_hip_enqueue_msssim3h_win_grad(
                self.handle, count, params_array, sample_type_code(sample_type), data_range, _window_ref(window), scales, _weights_array(weights),
                means_dev_ptr, grad_out_dev_ptr, grad_a, grad_b))

    def enqueue_batch(self, params_array, count, sums_dev_ptr):
        _check("rmgr_ssim_hip_enqueue_batch", self.lib.rmgr_ssim_hip_enqueue_batch(self.handle, count, params_array, sums_dev_ptr))

    def enqueue_rows(self, params, y_begin, y_rows, cells_dev_ptr):
        """Rows [y_begin, y_begin + y_rows) of one device-resident pair: map rows + cell partials into a zeroed cell array."""
        _check("rmgr_ssim_hip_enqueue_rows", self.lib.rmgr_ssim_hip_enqueue_rows(self.handle, ctypes.byref(params), y_begin, y_rows, cells_dev_ptr))

    def reduce_cells(self, width, height, count, cells_dev_ptr, sums_dev_ptr):
        _check("rmgr_ssim_hip_reduce_cells", self.lib.rmgr_ssim_hip_reduce_cells(self.handle, width, height, count, cells_dev_ptr, sums_dev_ptr))

    # ---- native RCCL exchange (rmgr_ssim_hip_comm_*) ----
    @staticmethod
    def comm_unique_id():
        buf = ctypes.create_string_buffer(128)
        _check("rmgr_ssim_hip_comm_get_unique_id", load_library().rmgr_ssim_hip_comm_get_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, rank_count, rank):
        _check("rmgr_ssim_hip_comm_init", self.lib.rmgr_ssim_hip_comm_init(self.handle, unique_id, rank_count, rank))

    def comm_allreduce_sums(self, sums_dev_ptr, count):
        _check("rmgr_ssim_hip_comm_allreduce_sums", self.lib.rmgr_ssim_hip_comm_allreduce_sums(self.handle, sums_dev_ptr, count))

    def comm_destroy(self):
        _check("rmgr_ssim_hip_comm_destroy", self.lib.rmgr_ssim_hip_comm_destroy(self.handle))

    def comm_rank_count(self):
        """Ranks RCCL counts in this context's communicator (ncclCommCount); 0 without one."""
        n = ctypes.c_int32(0)
        _check("rmgr_ssim_hip_comm_rank_count", self.lib.rmgr_ssim_hip_comm_rank_count(self.handle, ctypes.byref(n)))
        return n.value

    @staticmethod
    def comm_describe():
        return load_library().rmgr_ssim_hip_comm_describe().decode()

    def synth_pair(self, a_ptr, a_stride, b_ptr, b_stride, width, height, seed):
        """Fill two device planes with the synthetic pair of SURVEY.md 8(d) (asynchronous on the context's stream)."""
        _check("rmgr_ssim_hip_synth_pair_device", self.lib.rmgr_ssim_hip_synth_pair_device(
            self.handle, a_ptr, a_stride, b_ptr, b_stride, width, height, seed))

    def probe_valu(self, waves_per_simd, stream_kind=0, launches=5, with_clock=False):
        """T lane-ops/s a pure packed-fp32 stream sustains on this device right now at a forced occupancy (rmgr_ssim_hip_probe_valu);
        with_clock: (T lane-ops/s, mean shader MHz over the XCDs, slowest XCD's MHz) of the timed launches."""
        t, mhz, lo = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _check("rmgr_ssim_hip_probe_valu", self.lib.rmgr_ssim_hip_probe_valu(self.handle, waves_per_simd, stream_kind, launches, ctypes.byref(t),
                                                                             ctypes.byref(mhz) if with_clock else None, ctypes.byref(lo) if with_clock else None))
        return (t.value, mhz.value, lo.value) if with_clock else t.value

    def get_profile_clock(self):
        """(mean shader MHz over the XCDs, slowest XCD's MHz, launches) of the profiled strip-kernel launches since the last call (rmgr_ssim_hip_get_profile_clock)."""
        mhz, lo, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
        _check("rmgr_ssim_hip_get_profile_clock", self.lib.rmgr_ssim_hip_get_profile_clock(self.handle, ctypes.byref(mhz), ctypes.byref(lo), ctypes.byref(n)))
        return mhz.value, lo.value, n.value

    def set_profiling(self, on):
        _check("rmgr_ssim_hip_set_profiling", self.lib.rmgr_ssim_hip_set_profiling(self.handle, 1 if on else 0))

    def get_profile(self):
        n = ctypes.c_uint64()
        ms = ctypes.c_double()
        _check("rmgr_ssim_hip_get_profile", self.lib.rmgr_ssim_hip_get_profile(self.handle, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    # ---- convenience used by the tests: planes given as numpy arrays, staged explicitly ----
    def ssim_planes(self, a, b, want_map=False):
        """Upload two H x W uint8 planes, run the device path, return (ssim, map or None)."""
        a = np.ascontiguousarray(a)
        b = np.ascontiguousarray(b)
        h, w = a.shape
        da, db = self.upload(a), self.upload(b)
        dm = self.alloc(4 * w * h) if want_map else None
        try:
            p = make_params(w, h, da.ptr, 1, w, db.ptr, 1, w, dm.ptr if dm else None, 1, w)
            v = self.compute_device(p)
            m = dm.download(np.float32, (h, w)) if dm else None
        finally:
            da.free()
            db.free()
            if dm:
                dm.free()
        return v, m
