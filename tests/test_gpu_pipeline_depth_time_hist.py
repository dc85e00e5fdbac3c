"""k_bounds_time_hist_pipe<2> (pcq_scan_dev_time_hist_batch) beyond its pipeline's second step, on step-coded data, against
numpy's compares per bin.

The plan, the schedule report and the step-coded data are those of tests/_pipeline_plan.py.  The kernel has K1's step of 512
points but its own number of workgroups per CU (scan_time_hist.hip: TIME_HIST_WAVES_PER_CU; the grid is capped at steps + segments
as K1's), so the Family is declared here.  The deep run is the batch of seventeen segments sized from the device's compute units:
at least 5g + g // 3 steps (depth 5 at least, both exits out of the steady state), in which workgroups change segment when either
cursor seeks and jump over segments with steps, without a whole step and without points.  The shallow run has 4g - 1 steps
(depths 4 and 3).  Segment k: positions 16-byte aligned, its time piece at byte phase 0 or 8 in turn, its box `q.box` shifted by
10 000 k along x — a cursor that keeps the previous segment's box or time block bins other points, or the same points under
their neighbours' times.  The data's three time ranges and the gaps between them are the bins: edges 100, 200, ..., 600.  The
planted points of step s lie in range s mod 3 (bins 0, 2, 4); the background inside the box carries times outside every range,
the ranges' ends among them (bins 1 and 3 take those at 200 and 400; 600 has no bin).  EMPTY_BOX_SEGMENT carries an empty box.
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

FAM = pp.Family("K1 time hist", 12, pp.K1.step)  # adhoc-queries-pointclouds_amd/csrc/scan_time_hist.hip: TIME_HIST_WAVES_PER_CU
EMPTY = ([5, 5, 5], [4, 4, 4])
EDGES = np.asarray([100.0, 200.0, 300.0, 400.0, 500.0, 600.0])
BINS = len(EDGES) - 1
WORDS = BINS + 8
PRESET = np.asarray([3 + 11 * c for c in range(WORDS)], dtype=np.uint64)


class Run:
    """Segments (steps, leftover points) in HBM, step-coded; `empty`: the segment whose box is empty."""

    def __init__(self, ctx, cus, seg_steps, seg_rest, empty, seed):
        self.ctx, self.empty = ctx, empty
        g = self.g = pp.full_grid(FAM, cus)
        assert all(r < FAM.step for r in seg_rest)
        ns = self.ns = [FAM.step * s + r for s, r in zip(seg_steps, seg_rest)]
        self.report = pp.depth_report(pp.schedule(pp.batch_grid(FAM, cus, sum(seg_steps), len(ns)), sum(seg_steps), seg_steps, ns))
        poff, psize = pp.carve(ns, [0] * len(ns), 12)
        toff, tsize = pp.carve(ns, [8 * (k % 2) for k in range(len(ns))], 8)
        self.blocks = [ctx.alloc(psize + 64), ctx.alloc(tsize + 64), ctx.alloc(8 * WORDS)]
        d_pos, d_t, self.d_hist = self.blocks
        assert d_pos % 16 == 0 and d_t % 16 == 0 and all(o % 16 == 0 for o in poff)
        assert {(d_t + o) % 16 for o, n in zip(toff, ns) if n} == {0, 8}
        begin = pp.tile_begin(seg_steps)
        rng = np.random.default_rng(seed)
        pos_img, t_img = np.zeros(psize, dtype=np.uint8), np.zeros(tsize, dtype=np.uint8)
        self.cols, self.q, self.xyz, self.t = [], [], [], []
        for k, (steps, rest) in enumerate(zip(seg_steps, seg_rest)):
            q = pp.PointQueries(10_000 * k)
            assert [e for r in q.ranges for e in r] == EDGES.tolist()
            xyz, _, t = pp.points_file(rng, g, steps, 0, rest, q, int(begin[k]))
            pos_img[poff[k]:poff[k] + 12 * ns[k]] = xyz.view(np.uint8).reshape(-1)
            t_img[toff[k]:toff[k] + 8 * ns[k]] = t.view(np.uint8).reshape(-1)
            self.cols.append(binding.make_columns(xyz=d_pos + poff[k], cls=d_t + toff[k], n=ns[k], cls_stride=8))
            self.q.append(q), self.xyz.append(xyz), self.t.append(t)
        ctx.to_device(d_pos, pos_img)
        ctx.to_device(d_t, t_img)

    def check(self):
        """One call with q.box of every live segment, from preset words; numpy's compares over the live segments"""
        boxes = [EMPTY if k == self.empty else q.box for k, q in enumerate(self.q)]
        want = np.zeros(BINS, dtype=np.int64)
        for k, (lo, hi) in enumerate(boxes):
            if k != self.empty:
                inside = pp.in_box(self.xyz[k], lo, hi)
                with np.errstate(invalid="ignore"):
                    want += np.asarray([int((inside & pp.in_range(self.t[k], EDGES[b], EDGES[b + 1])).sum()) for b in range(BINS)])
        self.ctx.to_device(self.d_hist, PRESET)
        self.ctx.scan_dev_time_hist_batch(self.cols, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], EDGES, self.d_hist)
        out = np.zeros(WORDS, dtype=np.uint64)
        self.ctx.to_host(out, self.d_hist)  # (waits for the context's stream)
        assert np.array_equal(out[BINS:], PRESET[BINS:])
        got = out[:BINS].astype(np.int64) - PRESET[:BINS].astype(np.int64)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, f"g={self.g}: (bin, got - want) = {[(int(c), int(got[c] - want[c])) for c in bad[:12]]}"
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
    r = Run(gpu_ctx, cus, steps, [n % FAM.step for n in ns], pp.EMPTY_BOX_SEGMENT, 821)
    yield r
    r.free()


def test_deep_plan_reaches_depth_five_through_both_cursors(deep):
    rep = deep.report
    assert sum(n // FAM.step for n in deep.ns) >= pp.deep_steps(deep.g)
    assert min(rep["depths"]) >= 5 and rep["both_exits_deep"], rep["depths"]
    assert rep["cross_into_a"] and rep["cross_into_b"] and rep["skips_stepped"] and rep["skips_zero_step"] and rep["skips_empty"], rep
    assert deep.empty in rep["skipped"] and deep.ns[deep.empty] // FAM.step > 0


def test_histogram_deep(deep):
    want = deep.check()
    assert all(w > 0 for w in want) and 0 < want.sum() < sum(deep.ns)


def test_histogram_shallow(gpu_ctx, cus):
    g = pp.full_grid(FAM, cus)
    steps = [g + g // 3 + 1, 3, 0]
    steps[2] = pp.shallow_steps(g) - steps[0] - steps[1]
    r = Run(gpu_ctx, cus, steps, [277, 77, 53], 1, 822)
    try:
        assert set(r.report["depths"]) == {3, 4} and r.report["cross_into_a"] and r.report["cross_into_b"], r.report
        want = r.check()
        assert want[0] > 0 and want[2] > 0 and want[4] > 0
    finally:
        r.free()
