"""The planner of the volume family (ssim3f_kernels.hip: plan3f, ssim3f_max_count) and the sub-batches of its host flow (ssim_volumes_abi.cpp:
take3f for device-resident volumes), restated in plain Python.  No GPU, no library call.  Sizes are W x H x D.

The walk cuts every 16 x 16 (x, y) tile of every volume into z-chunks, one workgroup each; the fp64 reduction cells are 16 x 16 x 8 voxels
at absolute positions.  A chunk is 8, 16, 32, ... slices deep (whole cells, doubling, up to the first depth that covers the volume); among
the depths whose grid stays below 2^24 workgroups the planner takes the one that finishes the launch's tiles x count x ceil(D / depth)
workgroups in the fewest slice-times, a round being CUs x 4 workgroups and a workgroup costing its slices plus 10 warm-up slices; of
equally cheap depths the deepest.  Chunk depth is scheduling only: results do not depend on it.

tests/test_ssim3f_plan_cpu.py holds every function here to the C++ it restates; tests/test_gpu_ssim3f_chunks.py uses them to assert, before
it launches, that a launch really runs the chunk depth it is there for.
"""
from collections import namedtuple

TILE, CELL_Z = 16, 8                 # kS3Tile, kS3CellZ
MAX_DIM = 0x7FFF0000                 # kS3MaxDim
MAX_BLOCKS = (1 << 24) - 1           # kMaxBlocks: x 256 work-items stays below 2^32
MAX_LAUNCH = 65535                   # volumes of one launch, whatever their size
WORKGROUPS_PER_CU, DEFAULT_CUS = 4, 256
WARMUP = 10                          # slices a chunk walks before and after its own
SCRATCH_CAP = 1 << 30                # kScratchCap: device scratch of one sub-batch, bytes

Geometry = namedtuple("Geometry", "tiles_x tiles_y cells_z chunk_slices chunks")


def tiles_of(width, height):
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def max_count(width, height, depth):
    """ssim3f_max_count: most volumes of this size one launch may take; 0 when a dimension is 0 or above the limit."""
    if min(width, height, depth) == 0 or max(width, height, depth) > MAX_DIM:
        return 0
    tx, ty = tiles_of(width, height)
    return min(MAX_BLOCKS // (tx * ty), MAX_LAUNCH)


def plan3f(width, height, depth, count, cus):
    tx, ty = tiles_of(width, height)
    slots = (cus if cus > 0 else DEFAULT_CUS) * WORKGROUPS_PER_CU
    cols = tx * ty * max(count, 1)
    best, best_slices = None, 0
    slices = CELL_Z
    while True:
        chunks = (depth + slices - 1) // slices
        if cols * chunks <= MAX_BLOCKS:
            cost = (cols * chunks + slots - 1) // slots * (min(slices, depth) + WARMUP)
            if best is None or cost <= best:
                best, best_slices = cost, slices
        if slices >= depth:
            if best_slices == 0:
                best_slices = slices
            break
        slices *= 2
    return Geometry(tx, ty, (depth + CELL_Z - 1) // CELL_Z, best_slices, (depth + best_slices - 1) // best_slices)


def grid(geo, count):
    """Workgroups of the walk of `count` volumes."""
    return geo.tiles_x * geo.tiles_y * geo.chunks * count


def cells_per_workgroup(geo, depth):
    """Reduction cells a full chunk flushes (a volume's only chunk: the cells of the volume)."""
    return (min(geo.chunk_slices, depth) + CELL_Z - 1) // CELL_Z


def last_chunk_slices(geo, depth):
    return depth - (geo.chunks - 1) * geo.chunk_slices


def describe(geo, width, height, depth, count):
    return ("%d x %d x %d, %d volumes: %d x %d tiles, chunks of %d slices = %d cells per workgroup, %d chunk(s) per tile, the last %d slices; "
            "%d workgroups" % (width, height, depth, count, geo.tiles_x, geo.tiles_y, geo.chunk_slices, cells_per_workgroup(geo, depth), geo.chunks,
                               last_chunk_slices(geo, depth), grid(geo, count)))


# ---- the sub-batches of a call on device-resident volumes ---------------------------------------------------------------------------

def forward_scratch(width, height, depth):
    """Bytes of cell partials per volume (enqueue_all, blocking)."""
    tx, ty = tiles_of(width, height)
    return tx * ty * ((depth + CELL_Z - 1) // CELL_Z) * 8


def grad_scratch(width, height, depth, which):
    """Bytes of coefficient volumes per volume (grad_entry): three float planes for one gradient, four for both."""
    return (4 if which == 3 else 3) * width * height * depth * 4


def per_sub_batch(width, height, depth, scratch):
    """take3f without staging: the volumes of every sub-batch but the last -- at most the launch limit and SCRATCH_CAP bytes of scratch,
    at least one."""
    return max(1, min(max_count(width, height, depth), SCRATCH_CAP // scratch))


def sub_batches(width, height, depth, count, scratch):
    """[(first volume, volumes)] of one call."""
    per, out, i0 = per_sub_batch(width, height, depth, scratch), [], 0
    while i0 < count:
        n = min(per, count - i0)
        out.append((i0, n))
        i0 += n
    return out


def smallest_count(width, height, depth, cus, want, limit=70000):
    """The smallest count whose plan satisfies want(geometry), or None."""
    for n in range(1, limit + 1):
        if want(plan3f(width, height, depth, n, cus)):
            return n
    return None
