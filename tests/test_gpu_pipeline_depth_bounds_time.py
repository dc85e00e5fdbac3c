"""k_bounds_count_batch_pipe<2, GpsTimes> (pcq_scan_dev_count_batch_bounds_time) beyond its pipeline's second step, on step-coded
data, against numpy.

The plan, the schedule report and the step-coded data are those of tests/_pipeline_plan.py, as test_gpu_pipeline_depth.py uses them: one
batch of seventeen segments sized from the device's compute units, at least 5g + g // 3 steps (depths 5 and 6, both exits out of
the steady state), in which workgroups change segment when either cursor seeks and jump over segments with a few steps, none,
and no point.  Segment k: its boxes shifted by 10 000 k along x and its range shifted by 1000 k; its planted points pass both
tests, half of its background passes the box alone (times outside every range), half the range alone (outside the box).  A
cursor that keeps the previous segment's range, or its time block, loses the planted points.  The time blocks are carved from
one buffer at 8-byte offsets of both residues modulo 16.
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


class Batch:
    """Segments in HBM with their predicates, numpy's answer for each, and the device total."""

    def __init__(self, ctx, name, g, run):
        self.ctx, self.name, self.g, self.run = ctx, name, g, run
        self.cols, self.preds, self.want, self.blocks = [], [], [], []
        self.d_total = self.alloc(64)

    def alloc(self, nbytes):
        p = self.ctx.alloc(nbytes + 64)
        assert p % 16 == 0
        self.blocks.append(p)
        return p

    def total(self):
        out = np.zeros(1, dtype=np.uint64)
        self.ctx.to_host(out, self.d_total)  # (waits for the context's stream)
        return int(out[0])

    def of(self, cols, preds):
        self.ctx.memset(self.d_total, 0, 8)
        self.run(cols, preds, self.d_total)
        return self.total()

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


def check_batch(b):
    """The whole batch and a second call that adds to it; every segment alone; prefixes; the reversed order."""
    n, want = len(b.cols), sum(b.want)
    got = b.of(b.cols, b.preds)
    assert got == want, f"{b.name} batch g={b.g}: got - want = {got - want}"
    b.run(b.cols, b.preds, b.d_total)
    assert b.total() == 2 * want, f"{b.name} batch g={b.g}, second call: got - want = {b.total() - 2 * want}"
    for k in range(n):
        got = b.of(b.cols[k:k + 1], b.preds[k:k + 1])
        assert got == b.want[k], f"{b.name} segment {k} alone g={b.g}: got - want = {got - b.want[k]}"
    for m in (2, 3, 5, 6, 9, 10, 12, 14, 16):
        got = b.of(b.cols[:m], b.preds[:m])
        assert got == sum(b.want[:m]), f"{b.name} first {m} segments g={b.g}: got - want = {got - sum(b.want[:m])}"
    got = b.of(b.cols[::-1], b.preds[::-1])
    assert got == want, f"{b.name} batch reversed g={b.g}: got - want = {got - want}"


def batch_reaches(fam, cus, plan, ns, steps):
    """Every crossing kind, with the real compute-unit count."""
    g = pp.full_grid(fam, cus)
    assert steps == [s.steps for s in plan]
    rep = pp.depth_report(pp.schedule(pp.batch_grid(fam, cus, sum(steps), len(plan)), sum(steps), steps, ns))
    assert sum(steps) >= pp.deep_steps(g) and min(rep["depths"]) >= 5 and rep["both_exits_deep"], rep["depths"]
    assert rep["cross_into_a"] and rep["cross_into_b"] and rep["skips_stepped"] and rep["skips_zero_step"] and rep["skips_empty"], rep
    s = np.arange(sum(steps))
    pp.check_counts(s, pp.planted(s, g), g, 1, fam.step)


def seg_range(k):
    return (1000.0 * k + 100.0, 1000.0 * k + 200.0)


class TimeSegments:
    def __init__(self, ctx, cus):
        g = self.g = pp.full_grid(pp.K1, cus)
        plan = pp.batch_plan(g)
        ns = [pp.point_segment_points(s) for s in plan]
        batch_reaches(pp.K1, cus, plan, ns, [n // pp.K1.step for n in ns])
        poff, psize = pp.carve(ns, [0] * len(ns), 12)
        toff, tsize = pp.carve(ns, [8 * (k % 2) for k in range(len(ns))], 8)
        self.keep = Batch(ctx, "", g, None)
        d_pos, d_t = self.keep.alloc(psize), self.keep.alloc(tsize)
        assert {(d_t + o) % 16 for o, n in zip(toff, ns) if n} == {0, 8}
        begin = pp.tile_begin([s.steps for s in plan])
        rng = np.random.default_rng(600)
        pos_img, t_img = np.zeros(psize, dtype=np.uint8), np.zeros(tsize, dtype=np.uint8)
        self.cols, self.q, self.xyz, self.t = [], [], [], []
        for k, seg in enumerate(plan):
            q = pp.PointQueries(10_000 * k, classes=(1,), other_classes=(2,), ranges=(seg_range(k),))
            xyz, _, t = pp.points_file(rng, g, seg.steps, 0, ns[k] - pp.K1.step * seg.steps, q, int(begin[k]))
            pos_img[poff[k]:poff[k] + 12 * ns[k]] = xyz.view(np.uint8).reshape(-1)
            t_img[toff[k]:toff[k] + 8 * ns[k]] = t.view(np.uint8).reshape(-1)
            self.cols.append(binding.make_columns(xyz=d_pos + poff[k], cls=d_t + toff[k], n=ns[k], cls_stride=8))
            self.q.append(q), self.xyz.append(xyz), self.t.append(t)
        ctx.to_device(d_pos, pos_img)
        ctx.to_device(d_t, t_img)

    def batch(self, ctx, boxes, ranges):
        b = Batch(ctx, "bounds_time", self.g, ctx.scan_dev_count_batch_bounds_time)
        b.cols = self.cols
        for k, ((lo, hi), (a, e)) in enumerate(zip(boxes, ranges)):
            b.preds.append(pkg.Predicate.bounds_time(lo, hi, a, e))
            with np.errstate(invalid="ignore"):
                b.want.append(int((pp.in_box(self.xyz[k], lo, hi) & pp.in_range(self.t[k], a, e)).sum()))
        return b


@pytest.fixture(scope="module")
def time_segments(gpu_ctx):
    p = TimeSegments(gpu_ctx, gpu_ctx.device_info()["compute_units"])
    yield p
    p.keep.free()


def test_bounds_time_batch(gpu_ctx, time_segments):
    """Every segment's large box and its own range; one box with lmin > lmax between two large segments."""
    p = time_segments
    boxes = [q.box for q in p.q]
    boxes[pp.EMPTY_BOX_SEGMENT] = ([5, 5, 5], [4, 4, 4])
    b = p.batch(gpu_ctx, boxes, [seg_range(k) for k in range(len(p.q))])
    try:
        assert b.want[pp.EMPTY_BOX_SEGMENT] == 0 and all(w > 0 for k, w in enumerate(b.want) if k != pp.EMPTY_BOX_SEGMENT and p.cols[k].n)
        # what a stale cursor would count is another number: the neighbour's range matches nothing here
        for k in range(1, len(p.q)):
            with np.errstate(invalid="ignore"):
                assert not pp.in_range(p.t[k], *seg_range(k - 1)).any()
        check_batch(b)
    finally:
        b.free()


def test_bounds_time_batch_small_boxes_and_the_whole_time_line(gpu_ctx, time_segments):
    """The planted points' small box with every time but NaN and +inf: the range passes the background too, the box decides."""
    p = time_segments
    b = p.batch(gpu_ctx, [q.sub[0] for q in p.q], [(-np.inf, np.inf)] * len(p.q))
    try:
        check_batch(b)
    finally:
        b.free()
