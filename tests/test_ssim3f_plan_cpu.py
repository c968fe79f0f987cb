"""CPU: what tests/test_gpu_ssim3f_chunks.py rests on, checked without a device.  Sizes are W x H x D.

  * tests/ssim3f_plan.py restates plan3f and ssim3f_max_count (ssim3f_kernels.hip).  A small host program (tests/src/plan3f_probe.cpp, its
    own main, no HIP call) is linked against the project's built ssim3f_kernels object and prints what the C++ chooses; the restatement
    must agree on the launches of the GPU module, on a few hundred seeded launches with depths on both sides of every power of two from 8
    to 1024 and counts from 1 to 70000, and for 32, 64, 128, 256 and 304 CUs and 0 (no CU count known: 256).
  * What the kernels rely on: a chunk is 8 slices times a power of two, the chunks cover the depth with none to spare, the grid stays
    below 2^24 workgroups, and a count within ssim3f_max_count always has a plan.
  * On a 256-CU device, the smallest count that gives each chunk depth on the two shapes of the GPU module.
  * The sub-batches of the host flow (take3f for device-resident volumes) as the GPU module expects them.
  * The fp32 emulation of the model stays inside ssim3f_model.tolerances() on the exact pairs the GPU module uses
    (tests/ssim3f_chunks_inputs.py), so that a miss on the GPU means the kernel and not the inputs.
"""
import os
import subprocess

import numpy as np
import pytest

import ssim3f_chunks_inputs as IN
import ssim3f_model as S
import ssim3f_plan as P
from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
KERNEL_OBJECT = "build/obj/ssim3f_kernels.o"
CUS = (32, 64, 128, 256, 304, 0)


# ---- 1. the restatement against the C++ ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """The probe, linked against the kernel object of the library under test (the Makefile's own rule brings it up to date: nothing to
    do after a build)."""
    r = subprocess.run(["make", "-C", ROOT, KERNEL_OBJECT], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path_factory.mktemp("plan3f_probe")
    obj, exe = str(out / "plan3f_probe.o"), str(out / "plan3f_probe")
    src = os.path.join(ROOT, "tests", "src", "plan3f_probe.cpp")
    for cmd in ([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                 "-I" + os.path.join(ROOT, "ssim_amd", "csrc"), "-c", src, "-o", obj],
                [HIPCC, "--offload-arch=gfx950", obj, os.path.join(ROOT, KERNEL_OBJECT), "-o", exe]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]

    def run(rows):
        """rows: (W, H, D, count, CUs) -> [(Geometry, max_count)]."""
        text = "".join("%d %d %d %d %d\n" % row for row in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        assert len(got) == len(rows) and all(len(g) == 6 for g in got)
        return [(P.Geometry(*g[:5]), g[5]) for g in got]
    return run


def gpu_module_launches(cus):
    """(W, H, D, count) of every launch of the GPU module on a device of `cus` CUs."""
    out = []
    for shape in IN.SHAPES:
        out += [shape + (n,) for n, _ in IN.depth_counts(shape, cus)] + [shape + (1,)]
    for i0, n in P.sub_batches(*IN.LIMIT_SHAPE, IN.LIMIT_COUNT, P.forward_scratch(*IN.LIMIT_SHAPE)):
        out.append(IN.LIMIT_SHAPE + (n,))
    return out + [IN.LIMIT_SHAPE + (1,), IN.RING_SHAPE + (1,)]


def seeded_launches():
    """(W, H, D, count): depths on both sides of every power of two from 8 to 1024 at counts from 1 to 70000, shapes of many tiles
    (whose launch limit is below 65535) at and beyond that limit, and depths no grid of shallow chunks fits."""
    rng = np.random.default_rng(IN.SEED)
    out = []
    for p in (8, 16, 32, 64, 128, 256, 512, 1024):
        for d in (p - 1, p, p + 1):
            for _ in range(4):
                w, h = int(rng.integers(1, 70)), int(rng.integers(1, 70))
                n = int(rng.choice([1, 2, 3, 7, 16, 61, 154, 449, 1000, 5000, 65535, 65536, 70000])) if rng.random() < 0.5 else int(rng.integers(1, 70001))
                out.append((w, h, d, n))
    for _ in range(200):
        w, h, d = int(rng.integers(1, 400)), int(rng.integers(1, 400)), int(rng.integers(1, 1300))
        out.append((w, h, d, int(np.exp(rng.uniform(0, np.log(70000.0))))))
    for w, h in ((300, 300), (1000, 17), (4096, 4096), (16, 16), (17, 16)):
        m = P.max_count(w, h, 50)
        out += [(w, h, d, n) for d in (50, 1100) for n in (m, m + 1, max(m - 1, 1))]
    out += [(1, 1, 8 * (1 << 24) + 5, 1), (33, 1, 1 << 27, 2), (1, 1, P.MAX_DIM, 1), (P.MAX_DIM, 1, 9, 1)]
    return out


def test_the_restatement_agrees_with_the_planner(probe):
    rows = []
    for cus in CUS:
        rows += [launch + (cus,) for launch in gpu_module_launches(cus) + seeded_launches()]
    got = probe(rows)
    depths, within = set(), 0
    for row, (geo, most) in zip(rows, got):
        w, h, d, n, cus = row
        mine = P.plan3f(w, h, d, n, cus)
        assert geo == mine, (row, geo, mine)
        assert most == P.max_count(w, h, d), (row, most)
        # what the kernels rely on
        k = geo.chunk_slices // P.CELL_Z
        assert geo.chunk_slices == k * P.CELL_Z and k >= 1 and k & (k - 1) == 0, (row, geo)
        assert geo.chunks * geo.chunk_slices >= d > (geo.chunks - 1) * geo.chunk_slices, (row, geo)
        assert (geo.tiles_x, geo.tiles_y, geo.cells_z) == ((w + 15) // 16, (h + 15) // 16, (d + 7) // 8), (row, geo)
        if 1 <= n <= most:
            assert P.grid(geo, n) <= P.MAX_BLOCKS < 1 << 24, (row, geo)
            within += 1
        depths.add(geo.chunk_slices)
    assert within > len(rows) // 2
    assert depths >= set(8 << i for i in range(8)), sorted(depths)         # 8 .. 1024: every depth takes part
    print("\n%d launches agree, %d of them within the launch limit; chunk depths %s" % (len(rows), within, sorted(depths)))


def test_max_count_refuses_what_the_entry_points_refuse(probe):
    rows = [(0, 5, 5, 1, 0), (5, 0, 5, 1, 0), (5, 5, 0, 1, 0), (P.MAX_DIM + 1, 5, 5, 1, 0), (5, P.MAX_DIM + 1, 5, 1, 0), (5, 5, P.MAX_DIM + 1, 1, 0)]
    for row, (_, most) in zip(rows, probe(rows)):
        assert most == 0 == P.max_count(*row[:3]), row


# ---- 2. the launches of the GPU module on 256 CUs -----------------------------------------------------------------------------------

WHOLE = "one chunk"


def smallest(shape, cus, depth):
    w, h, d = shape
    if depth == WHOLE:
        return P.smallest_count(w, h, d, cus, lambda g: g.chunks == 1)
    return P.smallest_count(w, h, d, cus, lambda g: g.chunk_slices == depth)


def test_the_smallest_count_of_every_chunk_depth_on_256_cus(probe):
    a, b = IN.SHAPES
    table = [(a, 8, 1), (a, 16, 16), (a, 32, 31), (a, 64, 61), (a, WHOLE, 154), (b, 128, 97), (b, 256, 193), (b, 512, 449)]
    for shape, depth, count in table:
        assert smallest(shape, 256, depth) == count, (shape, depth, count, smallest(shape, 256, depth))
    # the C++ on both sides of every entry
    rows = [shape + (n, 256) for shape, _, count in table for n in (count - 1, count) if n > 0]
    got = dict(zip(rows, probe(rows)))
    for shape, depth, count in table:
        here, before = got[shape + (count, 256)][0], got.get(shape + (count - 1, 256), (None,))[0]
        if depth == WHOLE:
            assert here.chunks == 1 and here.chunk_slices >= shape[2] and before.chunks > 1, (shape, here, before)
        else:
            assert here.chunk_slices == depth and (before is None or before.chunk_slices < depth), (shape, depth, here, before)
    # what the GPU module launches there: the counts above, and for the second shape the shallower depths as well
    assert [(n, g.chunk_slices) for n, g in IN.depth_counts(a, 256)] == [(1, 8), (16, 16), (31, 32), (61, 64), (154, 256)]
    assert [(n, g.chunk_slices) for n, g in IN.depth_counts(b, 256)] == [(1, 8), (9, 16), (17, 32), (33, 64), (97, 128), (193, 256), (449, 512)]
    ga = dict((g.chunk_slices, g) for _, g in IN.depth_counts(a, 256))
    assert P.last_chunk_slices(ga[64], 131) == 3 and ga[64].chunks == 3 and P.cells_per_workgroup(ga[64], 131) == 8
    assert ga[256].chunks == 1 and P.cells_per_workgroup(ga[256], 131) == 17 and ga[8].cells_z == 17
    gb = IN.depth_counts(b, 256)[-1][1]
    assert gb.chunks == 2 and P.cells_per_workgroup(gb, 1000) == 64 and P.last_chunk_slices(gb, 1000) == 488


@pytest.mark.parametrize("cus", [c for c in CUS if c])
def test_every_cu_count_covers_the_depths_the_gpu_module_demands(cus):
    """What the GPU module fails on, never skips: with at most COUNT_CAP volumes the first shape reaches depths 8, 16, 32, 64 and the
    single chunk of the whole depth, the second at least two depths of 128 or more; one volume alone runs at depth 8."""
    a, b = IN.SHAPES
    got = IN.depth_counts(a, cus)
    assert set(g.chunk_slices for _, g in got) >= {8, 16, 32, 64} and any(g.chunks == 1 for _, g in got), got
    assert len([g for _, g in IN.depth_counts(b, cus) if g.chunk_slices >= 128]) >= 2
    for shape in IN.SHAPES + (IN.LIMIT_SHAPE, IN.RING_SHAPE):
        assert P.plan3f(*shape, 1, cus).chunk_slices == 8, shape
    assert max(n for s in IN.SHAPES for n, _ in IN.depth_counts(s, cus)) <= IN.COUNT_CAP


# ---- 3. the sub-batches ----------------------------------------------------------------------------------------------------------------

def test_sub_batches_of_the_launch_limit_and_of_the_scratch():
    w, h, d = IN.LIMIT_SHAPE
    assert P.max_count(w, h, d) == 65535
    for scratch in (P.forward_scratch(w, h, d), P.grad_scratch(w, h, d, 3), P.grad_scratch(w, h, d, 1)):
        assert P.sub_batches(w, h, d, IN.LIMIT_COUNT, scratch) == [(0, 65535), (65535, 2)]
    # tests/test_gpu_ssim3f.py: 17 volumes of 160^3, both gradients, run in two sub-batches of the 1 GiB scratch
    assert P.sub_batches(160, 160, 160, 17, P.grad_scratch(160, 160, 160, 3)) == [(0, 16), (16, 1)]
    assert P.sub_batches(160, 160, 160, 17, P.forward_scratch(160, 160, 160)) == [(0, 17)]
    assert P.per_sub_batch(2048, 2048, 100, P.grad_scratch(2048, 2048, 100, 3)) == 1          # more than the cap each: one at a time
    # no launch of the chunk tests is split
    for shape in IN.SHAPES:
        assert P.per_sub_batch(*shape, P.grad_scratch(*shape, 3)) >= IN.COUNT_CAP and P.per_sub_batch(*shape, P.forward_scratch(*shape)) >= IN.COUNT_CAP


# ---- 4. the emulation on the pairs of the GPU module --------------------------------------------------------------------------------

def test_the_draws_name_every_pair_and_every_g_out():
    for shape in IN.SHAPES:
        ps = IN.pairs(shape)
        assert len(set(a.tobytes() for a, _ in ps)) == IN.PAIRS and all(a.shape == shape[::-1] for a, _ in ps)
    for n in (1, 9, 16, 31, 61, 154, 449):
        for salt in (0, 1):
            pick, gpick = IN.picks(n, salt)
            assert len(pick) == len(gpick) == n and len(set(pick.tolist())) == min(n, IN.PAIRS)
            assert len(set(zip(pick.tolist(), gpick.tolist()))) == min(n, 35)
            assert np.count_nonzero(np.diff(gpick)) >= n // 2 and np.count_nonzero(np.diff(pick)) >= n // 2
        assert np.any(IN.picks(n, 0)[0] != IN.picks(n, 1)[0])
    pick, gpick = IN.picks(IN.LIMIT_COUNT, IN.LIMIT_SALT)
    assert len(set(zip(pick.tolist(), gpick.tolist()))) == 35
    # the second sub-batch starts at volume 65535: neither its pairs nor its gOut values are those of volumes 0 and 1
    assert gpick[65535] != gpick[0] and gpick[65536] != gpick[1] and pick[65535] != pick[0] and pick[65536] != pick[1]


@pytest.mark.parametrize("shape", IN.SHAPES + (IN.LIMIT_SHAPE, IN.RING_SHAPE), ids=IN.shape_id)
def test_emulation_is_inside_the_gpu_bounds(shape):
    px_tol, g_tol, grad_tol, _ = S.tolerances()
    worst = [0.0, 0.0, 0.0]
    for k, (a, b) in enumerate(IN.pairs(shape)):
        g = IN.held_g(k)
        v, m, ea, eb = S.emulate_fp32(a, b, IN.RANGE, g_out=IN.G_OUTS[g])
        (gv, gm), (wa, wb) = IN.model(shape, k), IN.model_grad(shape, k, g)
        assert np.abs(wa).max() > 0 and np.abs(wb).max() > 0
        errs = (float(np.abs(m - gm).max()), abs(v - gv), max(float(np.abs(e - w).max() / np.abs(w).max()) for e, w in ((ea, wa), (eb, wb))))
        worst = [max(x, y) for x, y in zip(worst, errs)]
    print("%s: per voxel %.3g (%.3g), global %.3g (%.3g), gradient %.3g (%.3g)" % (IN.shape_id(shape), worst[0], px_tol, worst[1], g_tol, worst[2], grad_tol))
    assert worst[0] <= px_tol and worst[1] <= g_tol and worst[2] <= grad_tol
