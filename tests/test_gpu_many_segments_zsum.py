"""pcq_scan_dev_zsum_raster_batch with more segments than workgroups: the set of _many_segments.py (S = 2 * 16 * CUs + 37 segments,
sized from the device's compute units), so that the leftover loop at the end of k_bounds_zsum_pipe (`for (i = blockIdx.x; i < nseg;
i += gridDim.x)`) makes a second pass in every workgroup and a third in 37 of them.  It does for the mean-height raster what the
zrange case of test_gpu_many_segments.py does for the height raster: at 16 x 8 cells of 16 bytes the kernel runs the widest grid,
16 workgroups per CU (scan_zsum.hip: ZSUM_WAVES_PER_CU, far below the LDS limit), the density raster's.

Only the positions are uploaded.  The call adds into u64 / i64 words preset to distinct values, twice the raster's length: the
difference is numpy's answer on int64 — the counts are _many_segments.shares(.., "raster"), the sums np.add.at over the same
points — and the words behind the raster stay.  A launch over the segments below the grid alone (the others n = 0) says, when only
the full launch fails, that a later pass of the leftover loop is wrong.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _many_segments as ms  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

KIND = ms.Kind("zsum", ms.raster_waves(ms.CELLS, 16), ms.K1_STEP, ms.CELLS)
assert KIND.waves == ms.WIDEST
CELLS = ms.CELLS


def sum_shares(d):
    """[S, CELLS]: what each segment adds to each cell's z sum"""
    sel = ms.in_box(d)
    s, cell = ms.cells_of(d, sel)
    out = np.zeros((d.plan.S, CELLS), dtype=np.int64)
    np.add.at(out, (s, cell), d.xyz[sel, 2].astype(np.int64))
    return out


class Dev:
    def __init__(self, ctx):
        self.ctx = ctx
        self.cus = ctx.device_info()["compute_units"]
        p, d = self.plan, self.data = ms.plan(self.cus), ms.data(self.cus)
        self.blocks = [ctx.alloc(p.psize + 64), ctx.alloc(8 * 2 * CELLS), ctx.alloc(8 * 2 * CELLS)]
        d_pos, self.d_cnt, self.d_sum = self.blocks
        assert all(b % 16 == 0 for b in self.blocks)
        img = np.zeros(p.psize + 64, dtype=np.uint8)
        raw = np.ascontiguousarray(d.xyz).view(np.uint8).reshape(-1)
        for o, a, n in zip(p.poff, d.pstart, p.n):
            img[o:o + 12 * n] = raw[12 * a:12 * (a + n)]
        ctx.to_device(d_pos, img)
        self.pos = [d_pos + int(o) for o in p.poff]
        self.preds = [pkg.Predicate.bounds(a, b) for a, b in zip(d.lo.tolist(), d.hi.tolist())]
        self.pre_cnt = (2**32 - 64 + 5 * np.arange(2 * CELLS)).astype(np.int64)   # (some carry out of the low half)
        self.pre_sum = (-3000 + 11 * np.arange(2 * CELLS)).astype(np.int64)       # (some change sign)
        self.cnt_shares, self.sum_shares = ms.shares(d, "raster"), sum_shares(d)

    def wrong(self, keep=None):
        """What is wrong with a launch over the segments in `keep` (the others n = 0; None: all), or None"""
        n = self.plan.n if keep is None else np.where(keep, self.plan.n, 0)
        cols = [binding.make_columns(xyz=x, n=int(m)) for x, m in zip(self.pos, n)]
        self.ctx.to_device(self.d_cnt, self.pre_cnt), self.ctx.to_device(self.d_sum, self.pre_sum)
        self.ctx.scan_dev_zsum_raster_batch(cols, self.preds, self.data.cw.tolist(), ms.NX, ms.NY, self.d_cnt, self.d_sum)
        got_cnt, got_sum = np.zeros(2 * CELLS, dtype=np.int64), np.zeros(2 * CELLS, dtype=np.int64)
        self.ctx.to_host(got_cnt, self.d_cnt), self.ctx.to_host(got_sum, self.d_sum)  # (waits for the context's stream)
        for name, got, pre, share in (("count", got_cnt, self.pre_cnt, self.cnt_shares), ("sum", got_sum, self.pre_sum, self.sum_shares)):
            diff, want = got - pre, ms.answer(share, keep)
            bad = np.flatnonzero(diff[:CELLS] != want)
            if len(bad):
                return f"{name}: (cell, got - want) {[(int(b), int(diff[b] - want[b])) for b in bad[:8]]} ({len(bad)} of {CELLS} words)"
            if diff[CELLS:].any():
                return f"{name}: the words behind the raster changed"
        return None

    def free(self):
        for b in self.blocks:
            self.ctx.free(b)


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    d = Dev(gpu_ctx)
    yield d
    d.free()


def test_mean_height_raster(dev):
    p = dev.plan
    g = p.grid(KIND)
    assert g == 16 * dev.cus and sorted(set(p.passes(KIND).tolist())) == [2, 3]
    below = np.arange(p.S) < g
    want_cnt, below_cnt = ms.answer(dev.cnt_shares), ms.answer(dev.cnt_shares, below)
    want_sum, below_sum = ms.answer(dev.sum_shares), ms.answer(dev.sum_shares, below)
    later = int(((want_cnt > below_cnt) & (want_sum != below_sum)).sum())
    assert later >= 3  # cells whose words only a later pass can deliver
    print(f"\nzsum: grid {g}, S {p.S}, {later} of {CELLS} cells need a segment beyond the grid", file=sys.stderr)
    full, first = dev.wrong(), dev.wrong(below)
    assert first is None, f"the segments below the grid alone (the others n = 0): {first}; all segments: {full}"
    assert full is None, f"all segments: {full}; the segments below the grid alone are right: a later pass of the leftover loop is wrong"


def test_a_segment_behind_an_empty_one_keeps_its_own_constants(dev):
    """The live segments a workgroup reaches behind an empty predicate give something to the answer, and a launch with segment k's
    box changed differs from the first in k's share alone"""
    p = dev.plan
    live = dev.cnt_shares.sum(axis=1) > 0
    reached = ms.behind_an_empty(p, KIND, live)
    assert reached, "no live segment behind an empty one"  # (test_many_segments_plan.py proves it for every grid of the set)
    k = reached[-1]
    d2 = dev.data.changed(k)
    cnt2, sum2 = ms.shares(d2, "raster"), sum_shares(d2)
    other = np.arange(p.S) != k
    assert np.array_equal(cnt2[other], dev.cnt_shares[other]) and not np.array_equal(cnt2[k], dev.cnt_shares[k])
    saved = dev.preds, dev.cnt_shares, dev.sum_shares
    try:
        dev.preds = [pkg.Predicate.bounds(a, b) for a, b in zip(d2.lo.tolist(), d2.hi.tolist())]
        dev.cnt_shares, dev.sum_shares = cnt2, sum2
        assert dev.wrong() is None
    finally:
        dev.preds, dev.cnt_shares, dev.sum_shares = saved
