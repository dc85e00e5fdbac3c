"""pcq_scan_dev_zsum_raster_batch_classes with more segments than workgroups: the set of _many_segments.py (S = 2 * 16 * CUs + 37
segments, sized from the device's compute units), so that the leftover loop at the end of k_bounds_zsum_classes_pipe (`for (i =
blockIdx.x; i < nseg; i += gridDim.x)`) makes a second pass in every workgroup and a third in 37 of them — at 16 x 8 cells the kernel
runs its widest grid, 16 workgroups per CU (scan_zsum_classes.hip: ZSUM_CLASSES_WAVES_PER_CU), as test_gpu_many_segments_zsum.py's.

The positions are the set's; the class bytes are coded here from the segment, the trip of the one-lane-per-point loop and the point —
(3 (i // 64) + i + 2 k) % 5 for point i of segment k — at the set's class offsets (every byte phase of a 16-byte line), under the set
{1, 3}: the class read for another point, another trip or another segment's block differs from the point's own.  The call adds into
u64 / i64 words preset to distinct values, twice the raster's length; the difference is numpy's answer on int64 and the words behind
the raster stay.  A launch over the segments below the grid alone (the others n = 0) says, when only the full launch fails, that a
later pass of the leftover loop is wrong.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _many_segments as ms  # noqa: E402
from _zsum_classes import in_set  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

KIND = ms.Kind("zsum_classes", ms.raster_waves(ms.CELLS, 16), ms.K1_STEP, ms.CELLS)
assert KIND.waves == ms.WIDEST
CELLS = ms.CELLS
SET = (1, 3)


def class_bytes(d):
    """per point, in the order of d.xyz"""
    within = np.arange(len(d.seg)) - d.pstart[d.seg]
    return ((3 * (within // 64) + within + 2 * d.seg) % 5).astype(np.uint8)


def shares(d, cls):
    """([S, CELLS], [S, CELLS]): what each segment adds to each cell's count and z sum under SET"""
    sel = ms.in_box(d) & in_set(cls, SET)
    s, cell = ms.cells_of(d, sel)
    cnt, zsum = np.zeros((d.plan.S, CELLS), dtype=np.int64), np.zeros((d.plan.S, CELLS), dtype=np.int64)
    np.add.at(cnt, (s, cell), 1)
    np.add.at(zsum, (s, cell), d.xyz[sel, 2].astype(np.int64))
    return cnt, zsum


class Dev:
    def __init__(self, ctx):
        self.ctx = ctx
        self.cus = ctx.device_info()["compute_units"]
        p, d = self.plan, self.data = ms.plan(self.cus), ms.data(self.cus)
        self.blocks = [ctx.alloc(p.psize + 64), ctx.alloc(p.csize + 64), ctx.alloc(8 * 2 * CELLS), ctx.alloc(8 * 2 * CELLS)]
        d_pos, d_cls, self.d_cnt, self.d_sum = self.blocks
        assert all(b % 16 == 0 for b in self.blocks)
        self.cls = class_bytes(d)
        img, cimg = np.zeros(p.psize + 64, dtype=np.uint8), np.full(p.csize + 64, 1, dtype=np.uint8)  # (between the pieces: a class of the set)
        raw = np.ascontiguousarray(d.xyz).view(np.uint8).reshape(-1)
        for o, c, a, n in zip(p.poff, p.coff, d.pstart, p.n):
            img[o:o + 12 * n] = raw[12 * a:12 * (a + n)]
            cimg[c:c + n] = self.cls[a:a + n]
        ctx.to_device(d_pos, img)
        ctx.to_device(d_cls, cimg)
        self.pos = [d_pos + int(o) for o in p.poff]
        self.cblk = [d_cls + int(c) for c in p.coff]
        self.preds = [pkg.Predicate.bounds(a, b) for a, b in zip(d.lo.tolist(), d.hi.tolist())]
        self.pre_cnt = (2**32 - 64 + 5 * np.arange(2 * CELLS)).astype(np.int64)   # (some carry out of the low half)
        self.pre_sum = (-3000 + 11 * np.arange(2 * CELLS)).astype(np.int64)       # (some change sign)
        self.cnt_shares, self.sum_shares = shares(d, self.cls)

    def wrong(self, keep=None):
        """What is wrong with a launch over the segments in `keep` (the others n = 0; None: all), or None"""
        n = self.plan.n if keep is None else np.where(keep, self.plan.n, 0)
        cols = [binding.make_columns(xyz=x, cls=c, n=int(m)) for x, c, m in zip(self.pos, self.cblk, n)]
        self.ctx.to_device(self.d_cnt, self.pre_cnt), self.ctx.to_device(self.d_sum, self.pre_sum)
        self.ctx.scan_dev_zsum_raster_batch_classes(cols, self.preds, self.data.cw.tolist(), ms.NX, ms.NY, SET, self.d_cnt, self.d_sum)
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


def test_mean_height_raster_of_classes(dev):
    p = dev.plan
    g = p.grid(KIND)
    assert g == 16 * dev.cus and sorted(set(p.passes(KIND).tolist())) == [2, 3]
    assert sorted(set((np.asarray(dev.cblk) % 4).tolist())) == [0, 1, 2, 3]
    below = np.arange(p.S) < g
    want_cnt, below_cnt = ms.answer(dev.cnt_shares), ms.answer(dev.cnt_shares, below)
    want_sum, below_sum = ms.answer(dev.sum_shares), ms.answer(dev.sum_shares, below)
    later = int(((want_cnt > below_cnt) & (want_sum != below_sum)).sum())
    assert later >= 3  # cells whose words only a later pass can deliver
    every = ms.answer(ms.shares(dev.data, "raster"))
    assert 0 < want_cnt.sum() < every.sum()  # the set keeps points and drops points
    full, first = dev.wrong(), dev.wrong(below)
    assert first is None, f"the segments below the grid alone (the others n = 0): {first}; all segments: {full}"
    assert full is None, f"all segments: {full}; the segments below the grid alone are right: a later pass of the leftover loop is wrong"
