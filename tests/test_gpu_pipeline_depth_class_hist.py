"""k_bounds_class_hist_pipe<2, R> (pcq_scan_dev_class_hist_batch) beyond its pipeline's second step, on step-coded data, against
numpy's full 256-bin histogram.

The plan, the schedule report and the step-coded data are those of tests/_pipeline_plan.py.  The kernel has K1's step of 512
points but its own number of workgroups per CU (scan_class_hist.hip:37, CLASS_HIST_WAVES_PER_CU = 4; the grid is capped at steps +
segments as K1's), so the Family is declared here.  The deep run is the batch of seventeen segments sized from the device's
compute units: at least 5g + g // 3 steps (depth 5 at least, both exits out of the steady state), in which workgroups change
segment when either cursor seeks and jump over segments with steps, without a whole step and without points.  The shallow run
has 4g - 1 steps (depths 4 and 3).  Segment k: positions 16-byte aligned, class bytes at the plan's byte phases 0..15, its box
`q.box` shifted by 10 000 k along x — a cursor that keeps the previous segment's box, class block or misalignment bins other
points, or the same points under their neighbours' bytes.  EMPTY_BOX_SEGMENT carries an empty box.
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

FAM = pp.Family("K1 class hist", 4, pp.K1.step)  # adhoc-queries-pointclouds_amd/csrc/scan_class_hist.hip:37
EMPTY = ([5, 5, 5], [4, 4, 4])
BINS = 256
PRESET = np.asarray([3 + 11 * c for c in range(BINS)], dtype=np.uint64)


class Run:
    """Segments (steps, leftover points, class byte phase) in HBM, step-coded; `empty`: the segment whose box is empty."""

    def __init__(self, ctx, cus, seg_steps, seg_rest, phases, empty, seed):
        self.ctx, self.empty = ctx, empty
        g = self.g = pp.full_grid(FAM, cus)
        assert all(r < FAM.step for r in seg_rest)
        ns = self.ns = [FAM.step * s + r for s, r in zip(seg_steps, seg_rest)]
        self.report = pp.depth_report(pp.schedule(pp.batch_grid(FAM, cus, sum(seg_steps), len(ns)), sum(seg_steps), seg_steps, ns))
        poff, psize = pp.carve(ns, [0] * len(ns), 12)
        coff, csize = pp.carve(ns, phases)
        self.blocks = [ctx.alloc(psize + 64), ctx.alloc(csize + 64), ctx.alloc(8 * BINS)]
        d_pos, d_cls, self.d_hist = self.blocks
        assert d_pos % 16 == 0 and d_cls % 16 == 0 and all(o % 16 == 0 for o in poff)
        begin = pp.tile_begin(seg_steps)
        rng = np.random.default_rng(seed)
        pos_img, cls_img = np.zeros(psize, dtype=np.uint8), np.full(csize, 255, dtype=np.uint8)
        self.cols, self.q, self.xyz, self.cls = [], [], [], []
        for k, (steps, rest) in enumerate(zip(seg_steps, seg_rest)):
            # the planted points carry class 20 + k, the background inside the box its neighbours' classes, the background outside
            # it the segment's own class: every bin a segment feeds is fed by another segment too
            q = pp.PointQueries(10_000 * k, classes=(20 + k,), other_classes=(19 + k, 21 + k))
            xyz, cls, _ = pp.points_file(rng, g, steps, 0, rest, q, int(begin[k]))
            pos_img[poff[k]:poff[k] + 12 * ns[k]] = xyz.view(np.uint8).reshape(-1)
            cls_img[coff[k]:coff[k] + ns[k]] = cls
            self.cols.append(binding.make_columns(xyz=d_pos + poff[k], cls=d_cls + coff[k], n=ns[k]))
            self.q.append(q), self.xyz.append(xyz), self.cls.append(cls)
        ctx.to_device(d_pos, pos_img)
        ctx.to_device(d_cls, cls_img)

    def check(self):
        """One call with q.box of every live segment, from preset words; numpy's histogram over the live segments"""
        boxes = [EMPTY if k == self.empty else q.box for k, q in enumerate(self.q)]
        want = np.zeros(BINS, dtype=np.int64)
        for k, (lo, hi) in enumerate(boxes):
            if k != self.empty:
                want += np.bincount(self.cls[k][pp.in_box(self.xyz[k], lo, hi)], minlength=BINS)
        self.ctx.to_device(self.d_hist, PRESET)
        self.ctx.scan_dev_class_hist_batch(self.cols, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], self.d_hist)
        out = np.zeros(BINS, dtype=np.uint64)
        self.ctx.to_host(out, self.d_hist)  # (waits for the context's stream)
        got = out.astype(np.int64) - PRESET.astype(np.int64)
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
    assert steps == [s.steps for s in plan] and sorted({s.phase for s in plan}) == list(range(16))
    r = Run(gpu_ctx, cus, steps, [n % FAM.step for n in ns], [s.phase for s in plan], pp.EMPTY_BOX_SEGMENT, 811)
    yield r
    r.free()


def test_deep_plan_reaches_depths_five_and_six_through_both_cursors(deep):
    rep = deep.report
    assert sum(n // FAM.step for n in deep.ns) >= pp.deep_steps(deep.g)
    # (batch_plan holds about 6.1 g steps, so the depths are 6 and 7 rather than 5 and 6: every workgroup has taken the loop-back
    # twice and both exits are left from the steady state, which is what the test is after)
    assert min(rep["depths"]) >= 5 and rep["both_exits_deep"], rep["depths"]
    assert rep["cross_into_a"] and rep["cross_into_b"] and rep["skips_stepped"] and rep["skips_zero_step"] and rep["skips_empty"], rep
    assert deep.empty in rep["skipped"] and deep.ns[deep.empty] // FAM.step > 0


def test_histogram_deep(deep):
    want = deep.check()
    live = [k for k in range(len(deep.ns)) if k != deep.empty and deep.ns[k]]
    assert all(want[20 + k] > 0 for k in live) and want[19 + live[0]] > 0 and want[21 + live[-1]] > 0
    assert 0 < want.sum() < sum(deep.ns) and not want[:19].any() and not want[22 + len(deep.ns):].any()


def test_histogram_shallow(gpu_ctx, cus):
    g = pp.full_grid(FAM, cus)
    steps = [g + g // 3 + 1, 3, 0]
    steps[2] = pp.shallow_steps(g) - steps[0] - steps[1]
    r = Run(gpu_ctx, cus, steps, [277, 77, 53], [5, 10, 15], 1, 812)
    try:
        assert set(r.report["depths"]) == {3, 4} and r.report["cross_into_a"] and r.report["cross_into_b"], r.report
        want = r.check()
        assert want[20] > 0 and want[22] > 0 and want.sum() > 0
    finally:
        r.free()
