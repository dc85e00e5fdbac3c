"""k_bounds_zmoments_pipe<2> (pcq_scan_dev_zmoments_raster_batch) beyond its pipeline's second step, on step-coded data, against
numpy's count, sum of z and the two halves of the sum of z squared per cell on int64.

The plan, the schedule report and the step-coded data are those of tests/_pipeline_plan.py.  The kernel has K1's step of 512
points but its own number of workgroups per CU (scan_zmoments.hip: the smaller of ZMOMENTS_WAVES_PER_CU and what a CU's LDS holds at
the 32 x 32 = PCQ_ZMOMENTS_CELLS_MAX cells used here, five, rounded down to a multiple of four: 4; the grid is capped at steps +
segments as K1's), so the Family is declared here.  The deep run is the batch of seventeen segments sized from the device's compute
units: at least 5g + g // 3 steps (depth 5 at least, both exits out of the steady state), in which workgroups change segment when
either cursor seeks and jump over segments with steps, without a whole step and without points.  The shallow run has 4g - 1 steps
(depths 4 and 3).  Segment k: its box `q.box` shifted by 10 000 k along x, the raster's origin at the box's lower corner, and cell
widths (63 + k, 64 + 2k) of its own — a cursor that keeps a neighbour's box, widths, magics or origin bins into other cells, and a z
from the other register set is another point's.  EMPTY_BOX_SEGMENT carries an empty box.

What turns it red: a register set evaluated before its loads have landed or after the next load has overwritten it, at any depth
from 3 to 6; a cursor that is not advanced with its set; the tail prefetch folded in a second time.
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

NX, NY = 32, 32
LDS_LIMIT = 160 * 1024 // (32 * NX * NY)
FAM = pp.Family("K1 zmoments", min(16, LDS_LIMIT) & ~3, pp.K1.step)  # adhoc-queries-pointclouds_amd/csrc/scan_zmoments.hip
EMPTY = ([5, 5, 5], [4, 4, 4])
assert FAM.waves_per_cu == 4 and NX * NY == 1024
WORDS = NX * NY + 16
NAMES = ("count", "sum", "zsq_lo", "zsq_hi")
PRE = [np.asarray([(0, 2**32 - 1, 2**40 + c)[c % 3] for c in range(WORDS)], dtype=np.int64),
       np.asarray([(0, -1, 2**62, -2**62 + c)[c % 4] for c in range(WORDS)], dtype=np.int64),
       np.asarray([(-1, 0, 2**32 - 1, 2**33 + c)[c % 4] for c in range(WORDS)], dtype=np.int64),
       np.asarray([(2**32 - 1, -1 - c, 0)[c % 3] for c in range(WORDS)], dtype=np.int64)]


def widths(k):
    return 63 + k, 64 + 2 * k  # 32 cells of either cover the box's 2001 lattice steps


class Run:
    """Segments (steps, leftover points) in HBM, step-coded; `empty`: the segment whose box is empty."""

    def __init__(self, ctx, cus, seg_steps, seg_rest, empty, seed):
        self.ctx, self.empty = ctx, empty
        g = self.g = pp.full_grid(FAM, cus)
        assert all(r < FAM.step for r in seg_rest)
        ns = self.ns = [FAM.step * s + r for s, r in zip(seg_steps, seg_rest)]
        self.report = pp.depth_report(pp.schedule(pp.batch_grid(FAM, cus, sum(seg_steps), len(ns)), sum(seg_steps), seg_steps, ns))
        poff, psize = pp.carve(ns, [0] * len(ns), 12)
        self.blocks = [ctx.alloc(psize + 64)] + [ctx.alloc(8 * WORDS) for _ in NAMES]
        d_pos, self.d_words = self.blocks[0], self.blocks[1:]
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
        """One call with q.box of every live segment, from preset words; numpy's adds (modulo 2^64, as int64 wraps) over the live
        segments.  Returns the points per cell."""
        boxes = [EMPTY if k == self.empty else q.box for k, q in enumerate(self.q)]
        cws = [widths(k) for k in range(len(boxes))]
        want = [p.copy() for p in PRE]
        for k, (lo, hi) in enumerate(boxes):
            if k != self.empty:
                p = self.xyz[k][pp.in_box(self.xyz[k], lo, hi)].astype(np.int64)
                cell = ((p[:, 1] - lo[1]) // cws[k][1]) * NX + (p[:, 0] - lo[0]) // cws[k][0]
                assert not len(cell) or (0 <= cell.min() and cell.max() < NX * NY)
                z = p[:, 2]
                for w, v in zip(want, (np.ones_like(z), z, (z * z) & 0xffffffff, (z * z) >> 32)):
                    np.add.at(w, cell, v)
        for d, pre in zip(self.d_words, PRE):
            self.ctx.to_device(d, pre)
        self.ctx.scan_dev_zmoments_raster_batch(self.cols, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], cws, NX, NY, *self.d_words)
        for name, d, w in zip(NAMES, self.d_words, want):
            got = np.zeros(WORDS, dtype=np.int64)
            self.ctx.to_host(got, d)  # (waits for the context's stream)
            bad = np.flatnonzero(got != w)
            assert len(bad) == 0, f"g={self.g}: {name} (cell, got, want) = {[(int(c), int(got[c]), int(w[c])) for c in bad[:12]]} ({len(bad)} words)"
        assert (want[1][:NX * NY] != PRE[1][:NX * NY]).sum() > NX * NY // 8 and (want[2][:NX * NY] != PRE[2][:NX * NY]).sum() > NX * NY // 8
        return (want[0] - PRE[0])[:NX * NY]

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
    r = Run(gpu_ctx, cus, steps, [n % FAM.step for n in ns], pp.EMPTY_BOX_SEGMENT, 841)
    yield r
    r.free()


def test_deep_plan_reaches_depths_five_and_six_through_both_cursors(deep):
    rep = deep.report
    assert sum(n // FAM.step for n in deep.ns) >= pp.deep_steps(deep.g)
    assert min(rep["depths"]) >= 5 and rep["both_exits_deep"], rep["depths"]
    assert rep["cross_into_a"] and rep["cross_into_b"] and rep["skips_stepped"] and rep["skips_zero_step"] and rep["skips_empty"], rep
    assert deep.empty in rep["skipped"] and deep.ns[deep.empty] // FAM.step > 0


def test_zmoments_deep(deep):
    cnt = deep.check()
    live = sum(n for k, n in enumerate(deep.ns) if k != deep.empty)
    # every point of a live segment passes the box or lies outside it: more than a third inside, spread over many cells
    assert live // 3 < cnt.sum() < live and (cnt > 0).sum() > NX * NY // 4


def test_zmoments_shallow(gpu_ctx, cus):
    g = pp.full_grid(FAM, cus)
    steps = [g + g // 3 + 1, 3, 0]
    steps[2] = pp.shallow_steps(g) - steps[0] - steps[1]
    r = Run(gpu_ctx, cus, steps, [277, 77, 53], 1, 842)
    try:
        assert set(r.report["depths"]) == {3, 4} and r.report["cross_into_a"] and r.report["cross_into_b"], r.report
        assert r.check().sum() > 0
    finally:
        r.free()
