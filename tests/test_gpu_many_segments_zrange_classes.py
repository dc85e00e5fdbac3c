"""pcq_scan_dev_zrange_raster_batch_classes with more segments than workgroups: the set of _many_segments.py (S = 2 * 16 * CUs + 37
segments, sized from the device's compute units), so that the leftover loop at the end of k_bounds_zrange_classes_pipe (`for (i =
blockIdx.x; i < nseg; i += gridDim.x)`) makes a second pass in every workgroup and a third in 37 of them — at 16 x 8 cells the kernel
runs its widest grid, 16 workgroups per CU (scan_zrange_classes.hip: ZRANGE_CLASSES_WAVES_PER_CU).

The positions are the set's; the class bytes are coded here from the segment, the trip of the one-lane-per-point loop and the point —
(3 (i // 64) + i + 2 k) % 5 for point i of segment k — at the set's class offsets (every byte phase of a 16-byte line), under the low
set {1, 3} and the high set {0, 3}: the class read for another point, another trip or another segment's block differs from the
point's own, and so does the verdict of the other set.  The call folds into i32 words preset to their sentinels, twice the raster's
length; the words behind the raster stay.  A launch over the segments below the grid alone (the others n = 0) says, when only the
full launch fails, that a later pass of the leftover loop is wrong.
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

CELLS = ms.CELLS
WAVES = min(16, ms.LDS_PER_CU // (256 + 8 * CELLS)) & ~3  # scan_zrange_classes.hip: the class table in front of the raster's words
KIND = ms.Kind("zrange_classes", WAVES, ms.K1_STEP, CELLS)
assert KIND.waves == ms.WIDEST
LOW, HIGH = (1, 3), (0, 3)
I32_MAX, I32_MIN = ms.I32_MAX, ms.I32_MIN


def class_bytes(d):
    """per point, in the order of d.xyz"""
    within = np.arange(len(d.seg)) - d.pstart[d.seg]
    return ((3 * (within // 64) + within + 2 * d.seg) % 5).astype(np.uint8)


def shares(d, cls):
    """([S, CELLS], [S, CELLS]): each segment's minimum under LOW and maximum under HIGH per cell, the sentinels where it has none"""
    zmin, zmax = np.full((d.plan.S, CELLS), I32_MAX, dtype=np.int64), np.full((d.plan.S, CELLS), I32_MIN, dtype=np.int64)
    box = ms.in_box(d)
    for out, fold, classes in ((zmin, np.minimum, LOW), (zmax, np.maximum, HIGH)):
        sel = box & in_set(cls, classes)
        s, cell = ms.cells_of(d, sel)
        fold.at(out, (s, cell), d.xyz[sel, 2].astype(np.int64))
    return zmin, zmax


class Dev:
    def __init__(self, ctx):
        self.ctx = ctx
        self.cus = ctx.device_info()["compute_units"]
        p, d = self.plan, self.data = ms.plan(self.cus), ms.data(self.cus)
        self.blocks = [ctx.alloc(p.psize + 64), ctx.alloc(p.csize + 64), ctx.alloc(4 * 2 * CELLS), ctx.alloc(4 * 2 * CELLS)]
        d_pos, d_cls, self.d_min, self.d_max = self.blocks
        assert all(b % 16 == 0 for b in self.blocks)
        self.cls = class_bytes(d)
        img, cimg = np.zeros(p.psize + 64, dtype=np.uint8), np.full(p.csize + 64, 3, dtype=np.uint8)  # (between the pieces: a class of both sets)
        raw = np.ascontiguousarray(d.xyz).view(np.uint8).reshape(-1)
        for o, c, a, n in zip(p.poff, p.coff, d.pstart, p.n):
            img[o:o + 12 * n] = raw[12 * a:12 * (a + n)]
            cimg[c:c + n] = self.cls[a:a + n]
        ctx.to_device(d_pos, img)
        ctx.to_device(d_cls, cimg)
        self.pos = [d_pos + int(o) for o in p.poff]
        self.cblk = [d_cls + int(c) for c in p.coff]
        self.preds = [pkg.Predicate.bounds(a, b) for a, b in zip(d.lo.tolist(), d.hi.tolist())]
        self.pre_min = np.full(2 * CELLS, I32_MAX, dtype=np.int32)
        self.pre_max = np.full(2 * CELLS, I32_MIN, dtype=np.int32)
        self.shares = shares(d, self.cls)

    def wrong(self, keep=None):
        """What is wrong with a launch over the segments in `keep` (the others n = 0; None: all), or None"""
        n = self.plan.n if keep is None else np.where(keep, self.plan.n, 0)
        cols = [binding.make_columns(xyz=x, cls=c, n=int(m)) for x, c, m in zip(self.pos, self.cblk, n)]
        self.ctx.to_device(self.d_min, self.pre_min), self.ctx.to_device(self.d_max, self.pre_max)
        self.ctx.scan_dev_zrange_raster_batch_classes(cols, self.preds, self.data.cw.tolist(), ms.NX, ms.NY, LOW, HIGH, self.d_min, self.d_max)
        got_min, got_max = np.zeros(2 * CELLS, dtype=np.int32), np.zeros(2 * CELLS, dtype=np.int32)
        self.ctx.to_host(got_min, self.d_min), self.ctx.to_host(got_max, self.d_max)  # (waits for the context's stream)
        want_min, want_max = ms.answer(self.shares, keep)
        for name, got, pre, want in (("zmin", got_min, self.pre_min, want_min), ("zmax", got_max, self.pre_max, want_max)):
            bad = np.flatnonzero(got[:CELLS].astype(np.int64) != want)
            if len(bad):
                return f"{name}: (cell, got, want) {[(int(b), int(got[b]), int(want[b])) for b in bad[:8]]} ({len(bad)} of {CELLS} words)"
            if not np.array_equal(got[CELLS:], pre[CELLS:]):
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


def test_canopy_raster(dev):
    p = dev.plan
    g = p.grid(KIND)
    assert g == 16 * dev.cus and sorted(set(p.passes(KIND).tolist())) == [2, 3]
    assert sorted(set((np.asarray(dev.cblk) % 4).tolist())) == [0, 1, 2, 3]
    below = np.arange(p.S) < g
    (want_min, want_max), (below_min, below_max) = ms.answer(dev.shares), ms.answer(dev.shares, below)
    later = int(((want_min < below_min) | (want_max > below_max)).sum())
    assert later >= 3  # cells whose words only a later pass can deliver
    plain_min, plain_max = ms.answer(ms.shares(dev.data, "zrange"))
    assert (want_min != plain_min).any() and (want_max != plain_max).any()  # the sets drop points that matter
    swapped_min = ms.answer((shares_swapped(dev)[0], dev.shares[1]))[0]
    assert (want_min != swapped_min).any()  # ... and the two sets differ where it shows
    full, first = dev.wrong(), dev.wrong(below)
    assert first is None, f"the segments below the grid alone (the others n = 0): {first}; all segments: {full}"
    assert full is None, f"all segments: {full}; the segments below the grid alone are right: a later pass of the leftover loop is wrong"


def shares_swapped(dev):
    """the minima under HIGH and the maxima under LOW: what a kernel that swaps the sets would fold"""
    d = dev.data
    zmin, zmax = np.full((d.plan.S, CELLS), I32_MAX, dtype=np.int64), np.full((d.plan.S, CELLS), I32_MIN, dtype=np.int64)
    box = ms.in_box(d)
    for out, fold, classes in ((zmin, np.minimum, HIGH), (zmax, np.maximum, LOW)):
        sel = box & in_set(dev.cls, classes)
        s, cell = ms.cells_of(d, sel)
        fold.at(out, (s, cell), d.xyz[sel, 2].astype(np.int64))
    return zmin, zmax
