"""k_bounds_count_multi_pipe<2, NQ> (pcq_scan_dev_count_batch_multi) beyond its pipeline's second step, on step-coded data,
against numpy.

The plan, the schedule report and the step-coded data are those of tests/_pipeline_plan.py.  The kernel has K1's step of 512
points but launches 12 workgroups per CU where K1 launches 3 (scan_count_multi.hip:24, MULTI_WAVES_PER_CU; the grid is capped at
steps + segments as K1's), so the Family is declared here.  The deep run
is the batch of seventeen segments sized from the device's compute units: at least 5g + g // 3 steps (depth 5 at least, both
exits out of the steady state), in which workgroups change segment when either cursor seeks.  The shallow run has 4g - 1 steps
(depths 4 and 3).  Segment k: its boxes shifted by 10 000 k along x, so a cursor that keeps the previous segment's boxes loses
the planted points.

One call asks eight boxes of every segment: its three `sub` boxes (the step-coded matches), `box`, `inside`, one `outside`, an
empty one and the full i32 range.  One segment between two large ones has all eight slots empty and one large segment only its
odd slots live: `live` changes at a seek of each cursor.  A second deep run asks two boxes (sub[0], sub[1]): another
instantiation at depth 5-6.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

FAM = pp.Family("K1 multi", 12, pp.K1.step)  # adhoc-queries-pointclouds_amd/csrc/scan_count_multi.hip:24
EMPTY = ([5, 5, 5], [4, 4, 4])
FULL = ([-2**40] * 3, [2**40] * 3)
PRESET = [3 + 11 * q for q in range(8)]


def slots(q):
    """The eight boxes of a segment."""
    return [q.sub[0], q.sub[1], q.sub[2], q.box, q.inside, q.outside[0], EMPTY, FULL]


class Run:
    """Segments (steps, leftover points) in HBM, step-coded; all_empty / odd_only: the segments whose live bits differ."""

    def __init__(self, ctx, cus, seg_steps, seg_rest, all_empty, odd_only, seed):
        self.ctx, self.all_empty, self.odd_only = ctx, all_empty, odd_only
        g = self.g = pp.full_grid(FAM, cus)
        assert all(r < FAM.step for r in seg_rest)
        ns = self.ns = [FAM.step * s + r for s, r in zip(seg_steps, seg_rest)]
        self.report = pp.depth_report(pp.schedule(pp.batch_grid(FAM, cus, sum(seg_steps), len(ns)), sum(seg_steps), seg_steps, ns))
        poff, psize = pp.carve(ns, [0] * len(ns), 12)
        self.blocks = [ctx.alloc(psize + 64), ctx.alloc(128)]
        d_pos, self.d_totals = self.blocks
        assert d_pos % 16 == 0 and all(o % 16 == 0 for o in poff)
        begin = pp.tile_begin(seg_steps)
        rng = np.random.default_rng(seed)
        img = np.zeros(psize, dtype=np.uint8)
        self.cols, self.q, self.xyz = [], [], []
        for k, (steps, rest) in enumerate(zip(seg_steps, seg_rest)):
            q = pp.PointQueries(10_000 * k)
            xyz, _, _ = pp.points_file(rng, g, steps, 0, rest, q, int(begin[k]))
            img[poff[k]:poff[k] + 12 * ns[k]] = xyz.view(np.uint8).reshape(-1)
            self.cols.append(binding.make_columns(xyz=d_pos + poff[k], n=ns[k]))
            self.q.append(q), self.xyz.append(xyz)
        ctx.to_device(d_pos, img)

    def boxes(self, k, pick):
        row = [slots(self.q[k])[s] for s in pick]
        if k == self.all_empty:
            return [EMPTY] * len(row)
        if k == self.odd_only:
            return [b if i % 2 else EMPTY for i, b in enumerate(row)]
        return row

    def check(self, pick):
        """One call with the boxes `pick` of every segment, from preset totals; every total from box_count over the live pairs."""
        nq = len(pick)
        rows, want = [], [0] * nq
        for k in range(len(self.ns)):
            row = self.boxes(k, pick)
            rows.append([pkg.Predicate.bounds(lo, hi) for lo, hi in row])
            for i, (lo, hi) in enumerate(row):
                if (lo, hi) != EMPTY:
                    want[i] += pp.box_count(self.xyz[k], lo, hi)
        self.ctx.to_device(self.d_totals, np.asarray(PRESET, dtype=np.uint64))
        self.ctx.scan_dev_count_batch_multi(self.cols, rows, self.d_totals)
        out = np.zeros(8, dtype=np.uint64)
        self.ctx.to_host(out, self.d_totals)  # (waits for the context's stream)
        got = [int(x) - p for x, p in zip(out, PRESET)]
        assert got[nq:] == [0] * (8 - nq), got
        assert got[:nq] == want, f"g={self.g} nq={nq}: got - want = {[a - b for a, b in zip(got, want)]}"
        return want

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
    assert steps == [s.steps for s in plan]
    r = Run(gpu_ctx, cus, steps, [n % FAM.step for n in ns], pp.EMPTY_BOX_SEGMENT, 6, 801)
    yield r
    r.free()


def test_deep_plan_reaches_depths_five_and_six_through_both_cursors(deep):
    rep = deep.report
    assert sum(n // FAM.step for n in deep.ns) >= pp.deep_steps(deep.g)
    # (batch_plan holds about 6.1 g steps, so the depths are 6 and 7 rather than 5 and 6: every workgroup has taken the loop-back
    # twice and both exits are left from the steady state, which is what the test is after)
    assert min(rep["depths"]) >= 5 and rep["both_exits_deep"], rep["depths"]
    assert rep["cross_into_a"] and rep["cross_into_b"] and rep["skips_stepped"] and rep["skips_zero_step"] and rep["skips_empty"], rep
    assert deep.ns[deep.odd_only] // FAM.step > deep.g // 2 and deep.all_empty in rep["skipped"]


def test_eight_boxes_deep(deep):
    want = deep.check(range(8))
    assert all(w > 0 for i, w in enumerate(want) if i != 6) and want[6] == 0
    live = sum(n for k, n in enumerate(deep.ns) if k != deep.all_empty)
    assert want[7] == live


def test_two_boxes_deep(deep):
    want = deep.check([0, 1])
    assert want[0] > 0 and want[1] > 0


def test_four_boxes_deep(deep):
    deep.check([2, 3, 7, 0])


def test_eight_boxes_shallow(gpu_ctx, cus):
    g = pp.full_grid(FAM, cus)
    steps = [g + g // 3 + 1, 3, 0]
    steps[2] = pp.shallow_steps(g) - steps[0] - steps[1]
    r = Run(gpu_ctx, cus, steps, [277, 77, 53], 1, 2, 802)
    try:
        assert set(r.report["depths"]) == {3, 4} and r.report["cross_into_a"] and r.report["cross_into_b"], r.report
        want = r.check(range(8))
        assert all(w > 0 for i, w in enumerate(want) if i != 6)
        r.check([0, 1])
    finally:
        r.free()
