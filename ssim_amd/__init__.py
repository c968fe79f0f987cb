"""ssim_amd -- MI355X-native SSIM engine, drop-in for rmgr::ssim::compute_ssim (romigrou/ssim 2.1.0).

The product is the C/C++ library ssim_amd/lib/librmgr-ssim-hip.so (sources in ssim_amd/csrc,
public headers in include/rmgr).  This Python package only binds its C ABI for tests and bench.py.
"""
from .api import (  # noqa: F401
    C_SYMBOLS, CXX_SYMBOLS, LIB_PATH, MODE_DOUBLE, MODE_EXACT, MODE_FAST, MODE_SEPARABLE, MODE_UNFUSED,
    ABI_VERSION, Context, DeviceBuffer, ImgParams, Params, Plan, SsimError, ThreadPool, Version,
    TuneResult, TunedEntry, compute_ssim, compute_ssim_batch, compute_ssim_batch_devices, compute_ssim_channels, compute_ssim_luminance, default_pool,
    MSSSIM_MAX_SCALES, MSSSIM_WANG_WEIGHTS, compute_msssim, compute_msssim_batch, default_pool_memory, device_count, finalize,
    get_plan, get_version, kernel_source_id, load_library, make_params, memory_info, trim_default_pool,
    Img16, Params16, compute_ssim16, compute_ssim16_batch, make_params16,
    ImgF, ParamsF, GradF, compute_ssimf, compute_ssimf_batch, make_params_f,
    Img3F, Params3F, Grad3F, GradOut3F, compute_ssim3f, compute_ssim3f_batch, make_params3f,
    Img3H, Params3H, Grad3H, compute_ssim3h, compute_ssim3h_batch, make_params3h,
    compute_msssimf, compute_msssimf_batch, compute_msssimh, compute_msssimh_batch, compute_msssim3f, compute_msssim3f_batch, compute_msssim3h, compute_msssim3h_batch,
    Window, WINDOW_GAUSSIAN, WINDOW_UNIFORM, WINDOW_SIZES, make_window,
    GradH, GradOutF, SAMPLE_F16, SAMPLE_BF16, compute_ssimh, compute_ssimh_batch, sample_type_code,
)
