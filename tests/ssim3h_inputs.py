"""Inputs shared by tests/test_ssim3h_cpu.py and tests/test_gpu_ssim3h.py, in plain numpy: no GPU, no library call.  Sizes are W x H x D;
arrays are (D, H, W); 16-bit samples travel as uint16 bit patterns (tests/halfmodel.py).

golden_cases(): the golden-derived volumes the GPU module holds to the float64 model as stored -- cut as tests/test_gpu_ssim3f.py cuts
them (ssim3f_model.fixture_forms), rounded into each encoding with halfmodel.round_to, then widened.  The CPU module checks the input
condition of that comparison on these very volumes: the fp32 emulation of the kernels stays within half of ssim3f_model.tolerances() of
the float64 model, per voxel and globally.
"""
import numpy as np

import halfmodel as HM
import ssim3f_model as S

# Not every golden volume qualifies: in the unit form as float16 the two q00 pairs leave 5.6e-6 and 6.2e-6 globally in the emulation, above
# half the global bound (4.8e-6); these three forms stay within it in both encodings.
GOLDEN = (("bbb255x63_q50_ch1", ("unit", "raw")), ("bbb257x65_q50_ch1", ("unit",)))

_cache = {}


def golden_cases(manifest):
    """[(what, encoding, uint16 a, uint16 b, data range)]: every form of GOLDEN in both encodings."""
    if "golden" not in _cache:
        out = []
        for name, forms in GOLDEN:
            for form, fa, fb, r in S.fixture_forms(manifest, name, forms):
                for enc in HM.ENCODINGS:
                    out.append(("%s %s %s" % (name, form, enc), enc, HM.round_to(fa, enc), HM.round_to(fb, enc), r))
        _cache["golden"] = out
    return _cache["golden"]


def golden_model(manifest, i):
    """(value, float64 map) of the float64 model on the widened volumes of case i; computed once."""
    key = ("model", i)
    if key not in _cache:
        _, enc, ua, ub, r = golden_cases(manifest)[i]
        _cache[key] = S.ssim(HM.widen(ua, enc), HM.widen(ub, enc), r)
    return _cache[key]


def random_pair(size, seed, enc, r=1.0):
    """A seeded pair of W x H x D in [0, r] as bit patterns of the encoding: random samples and a noisy copy."""
    w, h, d = size
    rng = np.random.default_rng(seed)
    a = rng.random((d, h, w), dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal((d, h, w)).astype(np.float32), 0, 1).astype(np.float32)
    return HM.round_to(a * np.float32(r), enc), HM.round_to(b * np.float32(r), enc)
