"""Inputs of the tests of multi-scale SSIM of volumes under a caller-chosen window (tests/test_msssim3k_cpu.py, test_gpu_msssim3k.py,
test_gpu_msssim3hk.py): the seeded odd-size pairs, on which ODD_EMU of tests/msssim3k_model.py is measured.  Sizes are W x H x D; arrays
are (D, H, W)."""
import numpy as np

# One voxel; thinner than every window; smaller than the 9-tap window on every axis; one more voxel than the 9-tap window reads; thin
# and deep; odd at several scales and across a tile; exactly one tile and one cell; more than one tile, cell and chunk, eight scales down
# to 1 x 1 x 1.
ODD_SIZES = ((1, 1, 1), (2, 1, 3), (7, 5, 3), (9, 9, 9), (17, 3, 33), (33, 20, 13), (16, 16, 8), (37, 21, 44))
ODD_WINDOWS = ((3, 0.0, "uniform"), (9, 1.5, "gaussian"))        # R = 1; R = 4, whose window exceeds most coarse volumes
ODD_SCALES = 8


def odd_pair(index):
    """The pair of ODD_SIZES[index]: a = float32(0.2 + 0.6 (x + 2y + 3z) / (W + 2H + 3D) + 0.05 N(0,1)), b = float32(a + 0.02 N(0,1)),
    a's noise drawn first from default_rng(0x3D00 + index); data range 1."""
    w, h, d = ODD_SIZES[index]
    rng = np.random.default_rng(0x3D00 + index)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    a = (0.2 + 0.6 * (x + 2 * y + 3 * z) / (w + 2 * h + 3 * d) + 0.05 * rng.standard_normal((d, h, w))).astype(np.float32)
    b = (a + 0.02 * rng.standard_normal((d, h, w))).astype(np.float32)
    return a, b


def odd_cases():
    """[(size, a, b, data range)] over ODD_SIZES."""
    return [(size,) + odd_pair(i) + (1.0,) for i, size in enumerate(ODD_SIZES)]
