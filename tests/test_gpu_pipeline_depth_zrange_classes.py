"""k_bounds_zrange_classes_pipe<2> (pcq_scan_dev_zrange_raster_batch_classes) beyond its pipeline's second step, on step-coded data,
against numpy's minimum under the low set and maximum under the high set per cell.

The plan, the schedule report and the step-coded data are those of tests/_pipeline_plan.py, as in
test_gpu_pipeline_depth_zsum_classes.py: at 64 x 64 cells scan_zrange_classes.hip launches 4 workgroups per CU (160 KiB / (256 + 8 x
4096) bytes), the deep run of seventeen segments sized from the device's compute units (depth 5 at least, both exits out of the steady
state, both cursors seek, segments jumped over), the shallow run of 4g - 1 steps.  The class bytes of points_file travel too, class
piece k at the plan's byte phase: in step s the m(s) planted points carry class classes[s mod 3], the rest of the box a class of
other_classes, and the points outside the box a class of `classes`.  With low = `classes` and high = other_classes the minima come
from the planted points alone and the maxima from the background alone, so a class byte from the other register set, the
neighbouring tile or another segment, or a verdict of the other set, moves a word; the reverse pair and (one class, all 256) are
asked as well.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402
from _zsum_classes import in_set  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

NX, NY = 64, 64
LDS_LIMIT = 160 * 1024 // (256 + 8 * NX * NY)
FAM = pp.Family("K1 zrange classes", min(16, LDS_LIMIT) if LDS_LIMIT <= 4 else min(16, LDS_LIMIT) & ~3, pp.K1.step)  # scan_zrange_classes.hip
EMPTY = ([5, 5, 5], [4, 4, 4])
assert FAM.waves_per_cu == 4 and NX * NY == 4096
I32_MIN, I32_MAX = -2**31, 2**31 - 1
WORDS = NX * NY + 16
PRE_MIN = np.asarray([(I32_MAX, 0, -10**9)[c % 3] for c in range(WORDS)], dtype=np.int32)
PRE_MAX = np.asarray([(I32_MIN, 0, 10**9, 7)[c % 4] for c in range(WORDS)], dtype=np.int32)
ALL = tuple(range(256))


def widths(k):
    return 32 + k, 33 + 2 * k  # 64 cells of either cover the box's 2001 lattice steps


class Run:
    """Segments (steps, leftover points) in HBM, step-coded; `empty`: the segment whose box is empty."""

    def __init__(self, ctx, cus, seg_steps, seg_rest, phases, empty, seed):
        self.ctx, self.empty = ctx, empty
        g = self.g = pp.full_grid(FAM, cus)
        assert all(r < FAM.step for r in seg_rest)
        ns = self.ns = [FAM.step * s + r for s, r in zip(seg_steps, seg_rest)]
        self.report = pp.depth_report(pp.schedule(pp.batch_grid(FAM, cus, sum(seg_steps), len(ns)), sum(seg_steps), seg_steps, ns))
        poff, psize = pp.carve(ns, [0] * len(ns), 12)
        coff, csize = pp.carve(ns, phases, 1)
        self.blocks = [ctx.alloc(psize + 64), ctx.alloc(csize + 64), ctx.alloc(4 * WORDS), ctx.alloc(4 * WORDS)]
        d_pos, d_cls, self.d_min, self.d_max = self.blocks
        assert d_pos % 16 == 0 and d_cls % 16 == 0 and all(o % 16 == 0 for o in poff)
        begin = pp.tile_begin(seg_steps)
        rng = np.random.default_rng(seed)
        pos_img, cls_img = np.zeros(psize, dtype=np.uint8), np.full(csize + 64, 2, dtype=np.uint8)  # (between the pieces: a class of the set)
        self.cols, self.q, self.xyz, self.cls = [], [], [], []
        for k, (steps, rest) in enumerate(zip(seg_steps, seg_rest)):
            q = pp.PointQueries(10_000 * k)
            xyz, cls, _ = pp.points_file(rng, g, steps, 0, rest, q, int(begin[k]))
            pos_img[poff[k]:poff[k] + 12 * ns[k]] = xyz.view(np.uint8).reshape(-1)
            cls_img[coff[k]:coff[k] + ns[k]] = cls
            self.cols.append(binding.make_columns(xyz=d_pos + poff[k], cls=d_cls + coff[k], n=ns[k]))
            self.q.append(q), self.xyz.append(xyz), self.cls.append(cls)
        self.misalignments = {(d_cls + o) % 4 for o, n in zip(coff, ns) if n >= FAM.step}
        ctx.to_device(d_pos, pos_img)
        ctx.to_device(d_cls, cls_img)

    def check(self, low, high):
        """One call with q.box of every live segment, from preset words; numpy's folds over the live segments.  Returns the number of
        words of zmin and of zmax that the call changed."""
        boxes = [EMPTY if k == self.empty else q.box for k, q in enumerate(self.q)]
        cws = [widths(k) for k in range(len(boxes))]
        zmin, zmax = PRE_MIN.copy(), PRE_MAX.copy()
        for k, (lo, hi) in enumerate(boxes):
            if k != self.empty:
                box = pp.in_box(self.xyz[k], lo, hi)
                for out, fold, classes in ((zmin, np.minimum, low), (zmax, np.maximum, high)):
                    p = self.xyz[k][box & in_set(self.cls[k], classes)].astype(np.int64)
                    cell = ((p[:, 1] - lo[1]) // cws[k][1]) * NX + (p[:, 0] - lo[0]) // cws[k][0]
                    assert not len(cell) or (0 <= cell.min() and cell.max() < NX * NY)
                    fold.at(out, cell, p[:, 2].astype(np.int32))
        self.ctx.to_device(self.d_min, PRE_MIN)
        self.ctx.to_device(self.d_max, PRE_MAX)
        self.ctx.scan_dev_zrange_raster_batch_classes(self.cols, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], cws, NX, NY, low, high,
                                                      self.d_min, self.d_max)
        for name, d, want in (("zmin", self.d_min, zmin), ("zmax", self.d_max, zmax)):
            got = np.zeros(len(want), dtype=np.int32)
            self.ctx.to_host(got, d)  # (waits for the context's stream)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (f"g={self.g}, low {sorted(low)[:8]}, high {sorted(high)[:8]}: {name} (cell, got, want) = "
                                   f"{[(int(c), int(got[c]), int(want[c])) for c in bad[:12]]} ({len(bad)} words)")
        assert np.array_equal(zmin[NX * NY:], PRE_MIN[NX * NY:]) and np.array_equal(zmax[NX * NY:], PRE_MAX[NX * NY:])
        return int((zmin != PRE_MIN).sum()), int((zmax != PRE_MAX).sum()), zmin, zmax

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
    r = Run(gpu_ctx, cus, steps, [n % FAM.step for n in ns], [s.phase for s in plan], pp.EMPTY_BOX_SEGMENT, 1931)
    yield r
    r.free()


def test_deep_plan_reaches_depths_five_and_six_through_both_cursors(deep):
    rep = deep.report
    assert sum(n // FAM.step for n in deep.ns) >= pp.deep_steps(deep.g)
    assert min(rep["depths"]) >= 5 and rep["both_exits_deep"], rep["depths"]
    assert rep["cross_into_a"] and rep["cross_into_b"] and rep["skips_stepped"] and rep["skips_zero_step"] and rep["skips_empty"], rep
    assert deep.empty in rep["skipped"] and deep.ns[deep.empty] // FAM.step > 0
    assert deep.misalignments == {0, 1, 2, 3}  # of the class blocks that have whole steps


def pairs_differ(r):
    q = r.q[0]
    a = r.check(q.classes, q.other_classes)
    b = r.check(q.other_classes, q.classes)
    c = r.check(q.classes[:1], ALL)
    assert a[0] > 0 and a[1] > 0 and b[0] > 0 and b[1] > 0 and c[0] > 0 and c[1] > 0
    assert not np.array_equal(a[2], b[2]) and not np.array_equal(a[3], b[3])  # swapping the sets shows in both arrays
    return a, b, c


def test_zrange_classes_deep(deep):
    pairs_differ(deep)
    none = deep.check((), ())
    assert none[0] == 0 and none[1] == 0


def test_zrange_classes_shallow(gpu_ctx, cus):
    g = pp.full_grid(FAM, cus)
    steps = [g + g // 3 + 1, 3, 0]
    steps[2] = pp.shallow_steps(g) - steps[0] - steps[1]
    r = Run(gpu_ctx, cus, steps, [277, 77, 53], [1, 2, 3], 1, 1932)
    try:
        assert set(r.report["depths"]) == {3, 4} and r.report["cross_into_a"] and r.report["cross_into_b"], r.report
        pairs_differ(r)
    finally:
        r.free()
