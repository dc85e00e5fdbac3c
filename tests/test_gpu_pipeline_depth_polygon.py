"""k_bounds_polygon_pipe<2> (pcq_scan_dev_count_batch_polygon) beyond its pipeline's second step, on step-coded data, against the
rule of include/pcq.h restated in numpy int64 (tests/_polygon_rule.py).

The plan, the schedule report and the step-coded data are those of tests/_pipeline_plan.py.  The kernel has K1's step of 512
points but its own number of workgroups per CU (scan_polygon.hip: POLYGON_WAVES_PER_CU; the grid is capped at steps + segments as
K1's), so the Family is declared here.  The deep run is the batch of seventeen segments sized from the device's compute units: at
least 5g + g // 3 steps (depth 5 at least, both exits out of the steady state), in which workgroups change segment when either
cursor seeks and jump over segments with steps, without a whole step and without points.  The shallow run has 4g - 1 steps (depths
4 and 3).  Segment k: its box `q.box` shifted by 10 000 k along x and an outline of its own, a hexagon around (10 000 k - 500, 0)
scaled by k — a cursor that keeps a neighbour's box, or the place or the number of a neighbour's edges, counts differently.
EMPTY_BOX_SEGMENT carries an empty box.
"""
import importlib
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402
import _polygon_rule as rule  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

POLYGON_WAVES_PER_CU = 16  # adhoc-queries-pointclouds_amd/csrc/scan_polygon.hip
FAM = pp.Family("K1 polygon", POLYGON_WAVES_PER_CU, pp.K1.step)
EMPTY = ([5, 5, 5], [4, 4, 4])
SENTINEL = 12345


def hexagon(k):
    r = 500 + 25 * k
    return [(10_000 * k - 500 + int(round(r * math.cos(0.2 + math.pi * i / 3))), int(round(r * math.sin(0.2 + math.pi * i / 3)))) for i in range(6)]


class Run:
    """Segments (steps, leftover points) in HBM, step-coded; `empty`: the segment whose box is empty."""

    def __init__(self, ctx, cus, seg_steps, seg_rest, empty, seed):
        self.ctx, self.empty = ctx, empty
        g = self.g = pp.full_grid(FAM, cus)
        assert all(r < FAM.step for r in seg_rest)
        ns = self.ns = [FAM.step * s + r for s, r in zip(seg_steps, seg_rest)]
        self.report = pp.depth_report(pp.schedule(pp.batch_grid(FAM, cus, sum(seg_steps), len(ns)), sum(seg_steps), seg_steps, ns))
        poff, psize = pp.carve(ns, [0] * len(ns), 12)
        self.blocks = [ctx.alloc(psize + 64), ctx.alloc(64)]
        d_pos, self.d_total = self.blocks
        assert d_pos % 16 == 0 and all(o % 16 == 0 for o in poff)
        begin = pp.tile_begin(seg_steps)
        rng = np.random.default_rng(seed)
        pos_img = np.zeros(psize, dtype=np.uint8)
        self.cols, self.q, self.xyz = [], [], []
        for k, (steps, rest) in enumerate(zip(seg_steps, seg_rest)):
            q = pp.PointQueries(10_000 * k)
            xyz, _, _ = pp.points_file(rng, g, steps, 0, rest, q, int(begin[k]))
            pos_img[poff[k]:poff[k] + 12 * ns[k]] = xyz.view(np.uint8).reshape(-1)
            self.cols.append(binding.make_columns(xyz=d_pos + poff[k], n=ns[k]))
            self.q.append(q), self.xyz.append(xyz)
        ctx.to_device(d_pos, pos_img)

    def check(self):
        """One call with q.box and the hexagon of every live segment; the rule over the live segments.  Returns (inside, passing the box)."""
        boxes = [EMPTY if k == self.empty else q.box for k, q in enumerate(self.q)]
        outlines = [hexagon(k) for k in range(len(boxes))]
        want = in_box = 0
        per = []
        for k, (lo, hi) in enumerate(boxes):
            if k != self.empty:
                per.append(int(rule.counted(self.xyz[k], lo, hi, outlines[k]).sum()))
                want += per[-1]
                in_box += int(rule.in_box(self.xyz[k], lo, hi).sum())
        assert len(set(per)) > len(per) // 2  # (the segments' counts differ)
        self.ctx.to_device(self.d_total, np.asarray([SENTINEL], dtype=np.uint64))
        self.ctx.scan_dev_count_batch_polygon(self.cols, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], outlines, self.d_total)
        got = np.zeros(1, dtype=np.uint64)
        self.ctx.to_host(got, self.d_total)  # (waits for the context's stream)
        assert int(got[0]) - SENTINEL == want, f"g={self.g}: got {int(got[0]) - SENTINEL}, want {want}"
        return want, in_box

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


@pytest.fixture(scope="module")
def cus(gpu_ctx):
    return gpu_ctx.device_info()["compute_units"]


@pytest.fixture(scope="module")
def deep(gpu_ctx, cus):
    g = pp.full_grid(FAM, cus)
    plan = pp.batch_plan(g)
    ns = [pp.point_segment_points(s) for s in plan]
    steps = [n // FAM.step for n in ns]
    assert steps == [s.steps for s in plan] and len(plan) == 17
    r = Run(gpu_ctx, cus, steps, [n % FAM.step for n in ns], pp.EMPTY_BOX_SEGMENT, 921)
    yield r
    r.free()


def test_the_constant_is_the_kernels():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adhoc-queries-pointclouds_amd", "csrc", "scan_polygon.hip")
    with open(path) as f:
        assert f"constexpr int POLYGON_WAVES_PER_CU = {POLYGON_WAVES_PER_CU};" in f.read()


def test_deep_plan_reaches_depths_five_and_six_through_both_cursors(deep):
    rep = deep.report
    assert sum(n // FAM.step for n in deep.ns) >= pp.deep_steps(deep.g)
    assert min(rep["depths"]) >= 5 and rep["both_exits_deep"], rep["depths"]
    assert rep["cross_into_a"] and rep["cross_into_b"] and rep["skips_stepped"] and rep["skips_zero_step"] and rep["skips_empty"], rep
    assert deep.empty in rep["skipped"] and deep.ns[deep.empty] // FAM.step > 0


def test_polygon_deep(deep):
    want, _ = deep.check()
    live = sum(n for k, n in enumerate(deep.ns) if k != deep.empty)
    assert live // 10 < want < 9 * live // 10, (want, live)  # between a tenth and nine tenths of the live points are inside


def test_polygon_shallow(gpu_ctx, cus):
    g = pp.full_grid(FAM, cus)
    steps = [g + g // 3 + 1, 3, 0]
    steps[2] = pp.shallow_steps(g) - steps[0] - steps[1]
    r = Run(gpu_ctx, cus, steps, [277, 77, 53], 1, 922)
    try:
        assert set(r.report["depths"]) == {3, 4} and r.report["cross_into_a"] and r.report["cross_into_b"], r.report
        want, in_box = r.check()
        live = sum(n for k, n in enumerate(r.ns) if k != r.empty)
        assert live // 10 < want < 9 * live // 10, (want, live)
    finally:
        r.free()
