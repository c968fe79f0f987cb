"""The strip planner of the five sample families, restated in plain Python: plan16 (ssim16_kernels.hip), planf (ssimf_kernels.hip), planh
(ssimh_kernels.hip), plank (ssimk_kernels.hip) and strip_rows_of (msssimf_kernels.hip); the last four are one-line calls of one planner,
plan_strips of ssim2_walk.h, with the warm-up rows as a parameter.  No GPU, no library call.

All five use one rule.  The reduction cells are 64 columns x cell_rows rows at absolute positions (32 rows for images of 2048 rows or
more, else 8).  A strip is STRIP_W columns wide and a whole number of cells tall, at most 2048 rows; among those heights the planner takes
the one that finishes the launch's strips_x * count * ceil(H / rows) strips in the fewest row-times, a round being CUs * 4 SIMDs * 3 waves
strips and a strip costing its rows plus its warm-up rows (10 for the 11-tap kernels, 2 R for a window of radius R); of equally cheap
heights the tallest.  Strip height is scheduling only: results do not depend on it.

tests/test_sample_plan_cpu.py holds every function here to the C++ it restates; tests/test_gpu_tall_strips.py uses them to assert, before
it launches, that a launch really runs the multi-cell strips it is there for.
"""
from collections import namedtuple

CELL_BATCH = 8          # cells a strip parks before it flushes them (enum CELL_BATCH of every strip kernel)
MAX_STRIP_ROWS = 2048
WAVES_PER_SIMD, SIMDS_PER_CU, DEFAULT_CUS = 3, 4, 256
# columns of a strip: kS16StripW, kSFStripW (ssimf, ssimk and msssimf share it), kSHStripW
STRIP_W = {"ssim16": 128, "ssimf": 128, "ssimh": 128, "ssimk": 128, "msssimf": 128}
FAMILIES = tuple(sorted(STRIP_W))

Geometry = namedtuple("Geometry", "cell_rows strip_rows strips_x strips_y")


def cell_rows_of(height):
    return 32 if height >= 2048 else 8


def _plan(width, height, count, cus, warmup, strip_w):
    cell_rows = cell_rows_of(height)
    slots = (cus if cus > 0 else DEFAULT_CUS) * SIMDS_PER_CU * WAVES_PER_SIMD
    strips_x = (width + strip_w - 1) // strip_w
    cols = strips_x * count
    best, best_rows = None, cell_rows
    rows = cell_rows
    while rows <= max(cell_rows, MAX_STRIP_ROWS):
        per_col = (height + rows - 1) // rows
        rounds = (cols * per_col + slots - 1) // slots
        cost = rounds * (min(rows, height) + warmup)
        if best is None or cost <= best:
            best, best_rows = cost, rows
        if rows >= height:
            break
        rows += cell_rows
    return Geometry(cell_rows, best_rows, strips_x, (height + best_rows - 1) // best_rows)


def plan16(width, height, count, cus):
    return _plan(width, height, count, cus, 10, STRIP_W["ssim16"])


def planf(width, height, count, cus):
    return _plan(width, height, count, cus, 10, STRIP_W["ssimf"])


def planh(width, height, count, cus):
    return _plan(width, height, count, cus, 10, STRIP_W["ssimh"])


def plank(radius, width, height, count, cus):
    """A window of radius 1 .. 4 (ssimk_kernels.hip); radius 5, the 11-tap windows, runs the ssimf kernels under planf."""
    if radius == 5:
        return planf(width, height, count, cus)
    assert 1 <= radius <= 4, radius
    return _plan(width, height, count, cus, 2 * radius, STRIP_W["ssimk"])


def msf_dim(n, scale):
    """Width or height of scale s of the pyramid: ceil(n / 2^s)."""
    return (n + (1 << scale) - 1) >> scale


def planms(width, height, count, cus, scale=0):
    """The strip launch of one scale of msssimf: strip_rows_of() on that scale's size."""
    return _plan(msf_dim(width, scale), msf_dim(height, scale), count, cus, 10, STRIP_W["msssimf"])


def plan(family, width, height, count, cus, radius=0):
    """By name, as the probe of tests/test_sample_plan_cpu.py takes its rows; radius only for ssimk."""
    if family == "ssimk":
        return plank(radius, width, height, count, cus)
    return {"ssim16": plan16, "ssimf": planf, "ssimh": planh, "msssimf": planms}[family](width, height, count, cus)


# ---- what a geometry means for a strip ----------------------------------------------------------------------------------------------

def cells_per_strip(geo, height):
    """Reduction cells a full strip walks (the image's only strip: the cells of the image)."""
    return (min(geo.strip_rows, height) + geo.cell_rows - 1) // geo.cell_rows


def last_strip_rows(geo, height):
    """Rows of the last strip of a column."""
    return height - (geo.strips_y - 1) * geo.strip_rows


def last_strip_cells(geo, height):
    return (last_strip_rows(geo, height) + geo.cell_rows - 1) // geo.cell_rows


def last_cell_rows(geo, height):
    """Rows of the image's last cell: cell_rows, or fewer when the height is no multiple of it."""
    return height - (height - 1) // geo.cell_rows * geo.cell_rows


def full_flushes(cells):
    """(flushes of a full batch, cells of the last, partial one) of a strip of `cells` cells."""
    return cells // CELL_BATCH, cells % CELL_BATCH


def describe(geo, width, height, count):
    n, last = cells_per_strip(geo, height), last_strip_cells(geo, height)
    return ("%d x %d, %d pairs: %d-row cells, strips of %d rows = %d cells (%d full flushes + %d), %d strip column(s) of %d strips; "
            "the last strip %d rows = %d cells, the last of them %d rows" % (
                width, height, count, geo.cell_rows, geo.strip_rows, n, full_flushes(n)[0], full_flushes(n)[1], geo.strips_x, geo.strips_y,
                last_strip_rows(geo, height), last, last_cell_rows(geo, height)))
