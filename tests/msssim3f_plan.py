"""The scratch and sub-batch rule of multi-scale SSIM of float32 volumes (msssim3f_kernels.hip: msssim3f_max_count,
msssim3f_scratch_bytes, msssim3f_per_sub_batch; ssim_volumes_abi.cpp passes them to take3f), restated in plain Python.  No GPU, no library
call.  Sizes are W x H x D.

Per pair: the pyramid of both volumes (scales >= 1, float32), in the backward one or two coarse gradient pyramids, the coefficient volumes
of the LARGEST scale (3 floats per voxel for one gradient, 4 for both; every scale reuses them) and `scales` floats of k_s; in the forward
two fp64 partials per 16 x 16 x 8 cell of every scale.  A sub-batch takes as many pairs as 1 GiB of that holds, at most the launch limit,
at least one.  tests/test_msssim3f_cpu.py holds every function here to the C++ through tests/src/msssim3f_plan_probe.cpp.
"""
import ssim3f_plan as P

SCRATCH_CAP = P.SCRATCH_CAP


def dim(n, s):
    """ms3_dim: ceil(n / 2^s)."""
    return (n + (1 << s) - 1) >> s


def dims(width, height, depth, s):
    return dim(width, s), dim(height, s), dim(depth, s)


def voxels(width, height, depth, s):
    w, h, d = dims(width, height, depth, s)
    return w * h * d


def pyramid_floats(width, height, depth, scales):
    return sum(voxels(width, height, depth, s) for s in range(1, scales))


def cells(width, height, depth, s):
    w, h, d = dims(width, height, depth, s)
    tx, ty = P.tiles_of(w, h)
    return tx * ty * ((d + P.CELL_Z - 1) // P.CELL_Z)


def max_count(width, height, depth):
    """msssim3f_max_count: the walk's limit and the pyramid step into scale 1 (one work-item per voxel, 256 per workgroup)."""
    walk = P.max_count(width, height, depth)
    if walk == 0:
        return 0
    return min(walk, P.MAX_BLOCKS // ((voxels(width, height, depth, 1) + 255) // 256))


def scratch_bytes(width, height, depth, scales, grad_planes):
    """msssim3f_scratch_bytes: grad_planes 0 the forward, 1 or 2 the backward for one gradient or both."""
    pyr = pyramid_floats(width, height, depth, scales)
    if grad_planes == 0:
        return 2 * pyr * 4 + sum(cells(width, height, depth, s) for s in range(scales)) * 2 * 8
    return (2 + grad_planes) * pyr * 4 + (4 if grad_planes == 2 else 3) * width * height * depth * 4 + scales * 4


def per_sub_batch(width, height, depth, scales, grad_planes, cap=SCRATCH_CAP):
    """msssim3f_per_sub_batch: the pairs of every sub-batch but the last."""
    return max(1, min(cap // scratch_bytes(width, height, depth, scales, grad_planes), max_count(width, height, depth)))


def sub_batches(width, height, depth, scales, grad_planes, count):
    """[(first pair, pairs)] of one call on device-resident volumes."""
    per, out, i0 = per_sub_batch(width, height, depth, scales, grad_planes), [], 0
    while i0 < count:
        n = min(per, count - i0)
        out.append((i0, n))
        i0 += n
    return out
