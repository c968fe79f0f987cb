"""The planner of the volume family for a window of radius R (ssim3k_kernels.h: plan3k = plan3f with 2R warm-up slices), restated in plain
Python.  No GPU, no library call.  Sizes are W x H x D.

It is tests/ssim3f_plan.py's plan3f with one change: a workgroup costs its slices plus 2R warm-up slices (10 for the 11-tap window: R = 5
gives ssim3f_plan.plan3f itself).  Tiles, cells, the launch limit and the sub-batches do not depend on the window: they are
ssim3f_plan's.  tests/test_ssim3k_cpu.py holds plan3k to the C++; tests/test_gpu_ssim3k.py uses it to assert, before it launches, that a
launch really runs the chunk depth it is there for.
"""
import ssim3f_plan as P
from ssim3f_plan import Geometry, grid, max_count, smallest_count  # noqa: F401  (re-exported for the tests)


def plan3k(radius, width, height, depth, count, cus):
    warmup = 2 * radius
    tx, ty = P.tiles_of(width, height)
    slots = (cus if cus > 0 else P.DEFAULT_CUS) * P.WORKGROUPS_PER_CU
    cols = tx * ty * max(count, 1)
    best, best_slices = None, 0
    slices = P.CELL_Z
    while True:
        chunks = (depth + slices - 1) // slices
        if cols * chunks <= P.MAX_BLOCKS:
            cost = (cols * chunks + slots - 1) // slots * (min(slices, depth) + warmup)
            if best is None or cost <= best:
                best, best_slices = cost, slices
        if slices >= depth:
            if best_slices == 0:
                best_slices = slices
            break
        slices *= 2
    return Geometry(tx, ty, (depth + P.CELL_Z - 1) // P.CELL_Z, best_slices, (depth + best_slices - 1) // best_slices)


def depth_counts(radius, shape, cus, cap=200):
    """[(count, Geometry)]: the smallest count (at most `cap`) that gives each chunk depth plan3k chooses for this shape and radius."""
    w, h, d = shape
    out, seen = [], set()
    for n in range(1, cap + 1):
        g = plan3k(radius, w, h, d, n, cus)
        if g.chunk_slices not in seen:
            seen.add(g.chunk_slices)
            out.append((n, g))
    return out
