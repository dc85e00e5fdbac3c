"""The ten batched entries with more segments than workgroups (_many_segments.py, proven on the CPU by test_many_segments_plan.py).

One upload of the set, sized from the device's compute units: S = 2 * 16 * CUs + 37 segments, so that the leftover loop at the
end of every batched kernel (`for (i = blockIdx.x; i < nseg; i += gridDim.x)`) makes a second pass in every workgroup of the
widest grid (16 * CUs: rasters, polygon) and a third in 37 of them; the narrower grids make up to eleven passes.  Every entry adds
into words preset to distinct non-zero values: the difference is numpy's answer, exactly, and the words behind it stay.

The smallest S at which an assertion can still fail.  A full launch differs from its first pass from S = grid + 1 on, if segment
`grid` has leftovers inside its predicate: 3 * CUs + 1 (box, box AND class, box AND time), 4 * CUs + 1 (class, class histogram),
12 * CUs + 1 (multi-box, time histogram), 16 * CUs + 1 (rasters, polygon).  A stride that is wrong only from its second
application on (a third pass) needs 2 * grid + 1, in the widest grid 32 * CUs + 1: this set's S, with 37 workgroups rather than
one on the third pass so that three LDS rasters of one workgroup hold something.  The below-the-grid launches keep S (the
segments from `grid` on have n = 0): they fail only where the first pass or the step loop is wrong.
"""
import importlib
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _many_segments as ms  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

REGION = 320      # u64 words per call: 256 of an answer at most, and what lies behind it
NCALLS = 40
BEGAN = time.perf_counter()


def image(size, offs, starts, counts, flat, unit):
    """Pieces of `counts` elements of `unit` bytes, piece k from element starts[k] of `flat`, at byte offsets offs"""
    img = np.zeros(size + 64, dtype=np.uint8)
    raw = np.ascontiguousarray(flat).view(np.uint8).reshape(-1)
    for o, a, n in zip(offs, starts, counts):
        if n:
            img[o:o + n * unit] = raw[a * unit:(a + n) * unit]
    return img


class Dev:
    def __init__(self, ctx):
        self.ctx = ctx
        self.cus = ctx.device_info()["compute_units"]
        p, d = self.plan, self.data = ms.plan(self.cus), ms.data(self.cus)
        S = self.S = p.S
        self.blocks = [ctx.alloc(size + 64) for size in (p.psize, p.csize, p.tsize, 8 * REGION * NCALLS)]
        d_pos, d_cls, d_t, self.d_out = self.blocks
        assert all(b % 16 == 0 for b in self.blocks)  # the plan's class steps assume it
        ctx.to_device(d_pos, image(p.psize, p.poff, d.pstart, p.n, d.xyz, 12))
        ctx.to_device(d_cls, image(p.csize, p.coff, d.cstart, p.nc, d.cls_c, 1))
        ctx.to_device(d_t, image(p.tsize, p.toff, d.pstart, p.n, d.t, 8))
        self.pos = [d_pos + int(o) for o in p.poff]
        self.clsp = [d_cls + int(o) for o in p.coff]
        self.tp = [d_t + int(o) for o in p.toff]
        assert {a % 16 for a, n in zip(self.clsp, p.nc) if n} == set(range(16)) and {a % 16 for a, n in zip(self.tp, p.n) if n} == {0, 8}
        self.preset = (1000 + 7 * np.arange(REGION * NCALLS)).astype(np.uint64)
        ctx.to_device(self.d_out, self.preset)
        self.call = 0
        self.entry = {"box": ctx.scan_dev_count_batch, "class": ctx.scan_dev_count_batch, "box_class": ctx.scan_dev_count_batch_combined,
                      "box_time": ctx.scan_dev_count_batch_bounds_time, "multi3": ctx.scan_dev_count_batch_multi,
                      "multi8": ctx.scan_dev_count_batch_multi, "class_hist": ctx.scan_dev_class_hist_batch,
                      "time_hist": ctx.scan_dev_time_hist_batch, "raster": ctx.scan_dev_raster_batch, "polygon": ctx.scan_dev_count_batch_polygon}
        self._shares = {}

    def shares(self, name, d=None):
        if d is not None:
            return ms.shares(d, name)
        if name not in self._shares:
            self._shares[name] = ms.shares(self.data, name)
        return self._shares[name]

    def below(self, name):
        """The segments of the first pass of the kind's leftover loop"""
        return np.arange(self.S) < self.plan.grid(ms.KIND[name])

    def cols(self, name, keep=None):
        """The kind's columns; the segments outside `keep` with n = 0"""
        p = self.plan
        n = p.seg_n(ms.KIND[name])
        n = [int(x) for x in (n if keep is None else np.where(keep, n, 0))]
        if name == "class":
            return [binding.make_columns(cls=c, n=m) for c, m in zip(self.clsp, n)]
        if name in ("box_class", "class_hist"):
            return [binding.make_columns(xyz=x, cls=c, n=m) for x, c, m in zip(self.pos, self.clsp, n)]
        if name in ("box_time", "time_hist"):
            return [binding.make_columns(xyz=x, cls=t, n=m, cls_stride=8) for x, t, m in zip(self.pos, self.tp, n)]
        return [binding.make_columns(xyz=x, n=m) for x, m in zip(self.pos, n)]

    def args(self, name, d=None):
        """The kind's predicates and what travels with them"""
        d = self.data if d is None else d
        lo, hi = d.lo.tolist(), d.hi.tolist()
        if name == "class":
            return ([pkg.Predicate.classification(int(c)) for c in d.qclass],)
        if name == "box_class":
            return ([pkg.Predicate.bounds_class(a, b, int(c)) for a, b, c in zip(lo, hi, d.qclass)],)
        if name == "box_time":
            return ([pkg.Predicate.bounds_time(a, b, float(t0), float(t1)) for a, b, t0, t1 in zip(lo, hi, d.t0, d.t1)],)
        if name in ("multi3", "multi8"):
            mlo, mhi = d.multi_boxes(ms.KIND[name].words)
            return ([[pkg.Predicate.bounds(a, b) for a, b in zip(ra, rb)] for ra, rb in zip(mlo.tolist(), mhi.tolist())],)
        preds = [pkg.Predicate.bounds(a, b) for a, b in zip(lo, hi)]
        if name == "time_hist":
            return preds, ms.EDGES
        if name in ("raster", "zrange"):
            return preds, d.cw.tolist(), ms.NX, ms.NY
        if name == "polygon":
            return preds, d.outline.tolist()
        return (preds,)

    def added(self, name, cols, args):
        """One launch into the next region; (the kind's words, whether the words behind them kept their preset)"""
        call, self.call = self.call, self.call + 1
        assert call < NCALLS
        self.entry[name](cols, *args, self.d_out + 8 * REGION * call)
        out = np.zeros(REGION, dtype=np.uint64)
        self.ctx.to_host(out, self.d_out + 8 * REGION * call)  # (waits for the context's stream)
        diff = out.astype(np.int64) - self.preset[REGION * call:REGION * (call + 1)].astype(np.int64)
        w = ms.KIND[name].words
        return diff[:w], not diff[w:].any()

    def wrong(self, name, keep=None, d=None):
        """(what is wrong with the launch or None, numpy's answer)"""
        got, behind = self.added(name, self.cols(name, keep), self.args(name, d))
        want = ms.answer(self.shares(name, d), keep)
        bad = np.flatnonzero(got != want)
        if len(bad):
            return f"(word, got - want) {[(int(b), int(got[b] - want[b])) for b in bad[:8]]} ({len(bad)} of {len(want)} words)", want
        return (None if behind else "the words behind the answer changed"), want

    def check(self, name, keep=None, d=None, what="all segments"):
        bad, want = self.wrong(name, keep, d)
        assert bad is None, f"{name}, {what}: {bad}"
        return want

    def free(self):
        for b in self.blocks:
            self.ctx.free(b)


@pytest.fixture(scope="module")
def dev():
    ctx = pkg.Context(0)
    try:
        d = Dev(ctx)
        print(f"\n{d.cus} CUs, S = {d.S}, {d.plan.points()} points; the upload took {time.perf_counter() - BEGAN:.2f} s since import", file=sys.stderr)
        try:
            yield d
        finally:
            d.free()
    finally:
        ctx.close()


def report(dev, name, want_all, want_below):
    k = ms.KIND[name]
    total, beyond = int(np.sum(want_all)), int(np.sum(want_all) - np.sum(want_below))
    print(f"\n{name}: grid {dev.plan.grid(k)}, S {dev.S}, passes {sorted(set(dev.plan.passes(k).tolist()))}, "
          f"answer {total}, from segments beyond the grid {beyond} ({100.0 * beyond / max(total, 1):.1f} %)", file=sys.stderr)


def full_and_below(dev, name):
    """The full launch, and the launch over the segments below the grid alone (the others n = 0): a failure of the first alone says
    that a later pass of the leftover loop is wrong"""
    below = dev.below(name)
    want_below = ms.answer(dev.shares(name), below)
    want_all = ms.answer(dev.shares(name))
    assert np.all(want_all > want_below)  # every word of the answer needs the later passes
    report(dev, name, want_all, want_below)
    full, _ = dev.wrong(name)
    first, _ = dev.wrong(name, keep=below)
    assert first is None, f"{name}, the segments below the grid alone (the others n = 0): {first}; all segments: {full}"
    assert full is None, f"{name}, all segments: {full}; the segments below the grid alone are right: a later pass of the leftover loop is wrong"


def test_box(dev):
    full_and_below(dev, "box")


def test_class(dev):
    full_and_below(dev, "class")


def test_box_and_class(dev):
    full_and_below(dev, "box_class")


def test_box_and_time(dev):
    full_and_below(dev, "box_time")


@pytest.mark.parametrize("name", ["multi3", "multi8"])
def test_multi_box(dev, name):
    """3 queries run the instantiation of 4 with a dead slot, 8 the full one; rows without a live box among the later passes"""
    lo, hi = dev.data.multi_boxes(ms.KIND[name].words)
    dead = (hi < lo).any(axis=2).all(axis=1)
    assert dead[dev.plan.grid(ms.KIND[name]):].any()
    full_and_below(dev, name)


def test_polygon(dev):
    full_and_below(dev, "polygon")


def test_class_histogram(dev):
    want = dev.check("class_hist")
    below = ms.answer(dev.shares("class_hist"), dev.below("class_hist"))
    assert (want > below).sum() >= 3 and (want == 0).sum() == 256 - len(ms.CLASSES)
    report(dev, "class_hist", want, below)


def test_time_histogram(dev):
    want = dev.check("time_hist")
    below = ms.answer(dev.shares("time_hist"), dev.below("time_hist"))
    assert np.all(want > below)
    report(dev, "time_hist", want, below)


def test_density_raster(dev):
    want = dev.check("raster")
    below = ms.answer(dev.shares("raster"), dev.below("raster"))
    assert (want > below).sum() >= 3
    report(dev, "raster", want, below)


def test_height_raster(dev):
    """Signed min and max into i32 words preset to distinct values inside the data's z range: a cell keeps its preset where no
    point beats it"""
    ctx, name = dev.ctx, "zrange"
    cells = ms.CELLS
    pre_min = (30 + np.arange(2 * cells) % 41).astype(np.int32)   # the words behind the raster too
    pre_max = (60 + np.arange(2 * cells) % 37).astype(np.int32)
    d_min, d_max = ctx.alloc(8 * cells), ctx.alloc(8 * cells)
    try:
        ctx.to_device(d_min, pre_min), ctx.to_device(d_max, pre_max)
        preds, cws, nx, ny = dev.args(name)
        ctx.scan_dev_zrange_raster_batch(dev.cols(name), preds, cws, nx, ny, d_min, d_max)
        got_min, got_max = np.zeros(2 * cells, dtype=np.int32), np.zeros(2 * cells, dtype=np.int32)
        ctx.to_host(got_min, d_min), ctx.to_host(got_max, d_max)
    finally:
        ctx.free(d_min), ctx.free(d_max)
    zmin, zmax = ms.answer(dev.shares(name))
    bmin, bmax = ms.answer(dev.shares(name), dev.below(name))
    want_min, want_max = np.minimum(pre_min[:cells], zmin), np.maximum(pre_max[:cells], zmax)
    first_min, first_max = np.minimum(pre_min[:cells], bmin), np.maximum(pre_max[:cells], bmax)
    later = int(((want_min < first_min) | (want_max > first_max)).sum())
    assert later >= 3  # cells whose words only a later pass can deliver
    print(f"\nzrange: grid {dev.plan.grid(ms.KIND[name])}, S {dev.S}, {later} of {cells} cells need a segment beyond the grid", file=sys.stderr)
    bad = np.flatnonzero((got_min[:cells] != want_min) | (got_max[:cells] != want_max))
    assert len(bad) == 0, [(int(c), int(got_min[c]), int(want_min[c]), int(got_max[c]), int(want_max[c])) for c in bad[:8]]
    assert np.array_equal(got_min[cells:], pre_min[cells:]) and np.array_equal(got_max[cells:], pre_max[cells:])


@pytest.mark.parametrize("name", ["box_time", "polygon"])
def test_a_change_in_the_tables_last_kilobyte(dev, name):
    """The same call again with the predicate (polygon: the box and one vertex) of segment S - 2 alone changed: the upload's byte
    compare has to see a change in the last kilobyte of a table of hundreds of kilobytes, and the polygon's edges lie behind
    nsegments x sizeof(Seg) at this S.  Then the first table again."""
    k = dev.S - 2
    first = dev.check(name, what="before the change")
    ch = dev.data.changed(k)
    if name == "polygon":
        share = dev.shares(name).copy()
        share[k, 0] = ms.polygon_segment(ch, k)
    else:
        share = ms.shares(ch, name)
    want = ms.answer(share)
    assert want[0] != first[0] and share[k, 0] > 0
    got, behind = dev.added(name, dev.cols(name), dev.args(name, ch))
    assert got[0] == want[0] and behind, (name, int(got[0]), int(want[0]), int(first[0]))
    dev.check(name, what="after the change, the first table again")
