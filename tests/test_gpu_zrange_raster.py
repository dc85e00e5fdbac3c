"""pcq_scan_dev_zrange_raster_batch: the lowest and the highest z per cell of a box over many resident segments in one pass, every
cell against numpy.

Segments of n = 0, 1, 511, 512, 513, 1535, 4133 points, the sizes of test_gpu_raster.py (a step of the pipeline is 512 points),
positions pieces 16-byte aligned in one buffer.  Every segment has its own origin, its own box and its own cell widths; x, y and z
are drawn independently, so a z taken from the wrong lane or load is another point's.  Every case uploads the positions it needs.
The call is a FOLD: every call starts from preset words, PCQ_ZRANGE_CELLS_MAX of each array and 64 more — "nothing yet" (INT32_MAX /
INT32_MIN), values inside the data's range, below it and above it, so that folding both ways is seen — and the test compares all of
them with np.minimum.at / np.maximum.at of the z of the points pp.in_box keeps into a copy of the presets: the raster's words
folded, the 64 behind them as they were.
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

NS = (0, 1, 511, 512, 513, 1535, 4133)
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
I32_MIN, I32_MAX = -2**31, 2**31 - 1
CELLS_MAX = 4096
WORDS = CELLS_MAX + 64
EMPTY = ([5, 5, 5], [4, 4, 4])
# z of the drawn data lies in 0 .. 99: per word nothing yet, a value inside the range, one below it, one above it
PRE_MIN = np.asarray([(I32_MAX, 50, -7 - c, 1000 + c)[c % 4] for c in range(WORDS)], dtype=np.int32)
PRE_MAX = np.asarray([(I32_MIN, 2000 + c, 50, I32_MIN, -1000 - c)[c % 5] for c in range(WORDS)], dtype=np.int32)
NOTHING = np.full(WORDS, I32_MAX, dtype=np.int32), np.full(WORDS, I32_MIN, dtype=np.int32)


def origin(k):
    return 1000 * k - 300, 77 - 500 * k


def box_of(k, nx, ny, cw, z=None):
    """Segment k's box: nx x ny full cells from its origin, and a slab of z that keeps about half of 0 .. 99"""
    ox, oy = origin(k)
    zlo, zhi = (25 + k, 74 - k) if z is None else z
    return [ox, oy, zlo], [ox + nx * cw[0] - 1, oy + ny * cw[1] - 1, zhi]


def draw(rng, nx, ny, cws, margin=2):
    """Positions of every segment: x and y independent over the segment's raster and `margin` lattice steps around it, z in 0..99"""
    out = []
    for k, n in enumerate(NS):
        ox, oy = origin(k)
        out.append(np.stack([ox + rng.integers(-margin, nx * cws[k][0] + margin, n), oy + rng.integers(-margin, ny * cws[k][1] + margin, n),
                             rng.integers(0, 100, n)], axis=1).astype(np.int32))
    return out


class Dev:
    def __init__(self, ctx):
        self.ctx = ctx
        self.poff, self.psize = pp.carve(NS, [0] * len(NS), 12)
        self.blocks = [ctx.alloc(self.psize + 64), ctx.alloc(4 * WORDS), ctx.alloc(4 * WORDS), ctx.alloc(8 * 8192)]
        self.d_pos, self.d_min, self.d_max, self.d_cnt = self.blocks
        assert all(p % 16 == 0 for p in self.blocks) and all(o % 16 == 0 for o in self.poff)
        self.cols = [binding.make_columns(xyz=self.d_pos + p, n=n) for p, n in zip(self.poff, NS)]
        self.xyz = None

    def upload(self, xyz):
        assert [len(a) for a in xyz] == list(NS)
        img = np.zeros(self.psize, dtype=np.uint8)
        for o, a in zip(self.poff, xyz):
            img[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.ctx.to_device(self.d_pos, img)
        self.xyz = xyz

    def want(self, boxes, cws, nx, ny, segments=None, pre=(PRE_MIN, PRE_MAX)):
        """(all words of the minima, all words of the maxima, points per cell): numpy's fold into a copy of `pre`"""
        wmin, wmax = pre[0].astype(np.int64), pre[1].astype(np.int64)
        cnt = np.zeros(nx * ny, dtype=np.int64)
        for k, (lo, hi), cw in zip(range(len(NS)) if segments is None else segments, boxes, cws):
            p = self.xyz[k][pp.in_box(self.xyz[k], lo, hi)].astype(np.int64)
            cell = ((p[:, 1] - int(lo[1])) // int(cw[1])) * nx + (p[:, 0] - int(lo[0])) // int(cw[0])
            assert not len(cell) or (0 <= cell.min() and cell.max() < nx * ny)
            np.minimum.at(wmin, cell, p[:, 2])
            np.maximum.at(wmax, cell, p[:, 2])
            np.add.at(cnt, cell, 1)
        return wmin, wmax, cnt

    def preset(self, pre):
        self.ctx.to_device(self.d_min, pre[0])
        self.ctx.to_device(self.d_max, pre[1])

    def words(self):
        lo, hi = np.zeros(WORDS, dtype=np.int32), np.zeros(WORDS, dtype=np.int32)
        self.ctx.to_host(lo, self.d_min)  # (waits for the context's stream)
        self.ctx.to_host(hi, self.d_max)
        return lo, hi

    def launch(self, boxes, cws, nx, ny, segments=None, cols=None, preds=None, d_zmin=None, d_zmax=None, stream=None):
        if cols is None:
            cols = self.cols if segments is None else [self.cols[k] for k in segments]
        if preds is None:
            preds = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
        self.ctx.scan_dev_zrange_raster_batch(cols, preds, cws, nx, ny, self.d_min if d_zmin is None else d_zmin,
                                              self.d_max if d_zmax is None else d_zmax, stream=stream)

    def compare(self, want, nx, ny):
        got = self.words()
        for name, g, w in (("min", got[0], want[0]), ("max", got[1], want[1])):
            bad = np.flatnonzero(g.astype(np.int64) != w)
            assert len(bad) == 0, (name, nx, ny, [(int(c), int(g[c]), int(w[c])) for c in bad[:12]], len(bad))

    def check(self, boxes, cws, nx, ny, segments=None, pre=(PRE_MIN, PRE_MAX), stream=None):
        """One call from the preset words: every word of both arrays is numpy's; returns the points per cell"""
        self.preset(pre)
        self.launch(boxes, cws, nx, ny, segments, stream=stream)
        want = self.want(boxes, cws, nx, ny, segments, pre)
        self.compare(want, nx, ny)
        return want[2]

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    d = Dev(gpu_ctx)
    yield d
    d.free()


@pytest.mark.parametrize("k", [3, 4, 5])
def test_one_point_per_cell(dev, k):
    """(a) 64 x 64 cells of width 1, a single segment of 512, 513 or 1535 points, point p in cell p with a z of its own over the
    whole i32 range: every position of a step, points 85 and 170 of both tiles, the leftover loop.  min == max == that z."""
    n, nx, ny = NS[k], 64, 64
    ox, oy = origin(k)
    rng = np.random.default_rng(700 + k)
    z = rng.integers(I32_MIN, I32_MAX + 1, n)
    z[85], z[170], z[256 + 85], z[256 + 170], z[n - 1] = I32_MIN, I32_MAX, I32_MAX - 1, I32_MIN + 1, I32_MIN + 2
    assert len(set(z.tolist())) == n
    xyz = [np.full((m, 3), -10**6, dtype=np.int32) for m in NS]
    p = np.arange(n)
    xyz[k] = np.stack([ox + p % 64, oy + p // 64, z], axis=1).astype(np.int32)
    dev.upload(xyz)
    box = ([ox, oy, -2**40], [ox + 63, oy + 63, 2**40])
    cnt = dev.check([box], [(1, 1)], nx, ny, [k], pre=NOTHING)
    assert cnt[:n].tolist() == [1] * n and not cnt[n:].any()
    lo, hi = dev.words()
    assert np.array_equal(lo[:n], z.astype(np.int32)) and np.array_equal(hi[:n], z.astype(np.int32))
    assert (lo[n:] == I32_MAX).all() and (hi[n:] == I32_MIN).all()
    # the i32 limits as the box's z faces: the same answer
    dev.check([([ox, oy, I32_MIN], [ox + 63, oy + 63, I32_MAX])], [(1, 1)], nx, ny, [k], pre=NOTHING)
    assert all(np.array_equal(a[:n], z.astype(np.int32)) for a in dev.words())


def test_all_segments_over_the_full_raster(dev):
    """(b) 64 x 64 = PCQ_ZRANGE_CELLS_MAX cells of one lattice value each; the z slab keeps about half the points, and those it
    rejects hold the extreme z"""
    nx, ny = 64, 64
    cws = [(1, 1)] * len(NS)
    dev.upload(draw(np.random.default_rng(41), nx, ny, cws))
    boxes = [box_of(k, nx, ny, (1, 1)) for k in range(len(NS))]
    cnt = dev.check(boxes, cws, nx, ny)
    assert sum(NS) // 4 < cnt.sum() < 2 * sum(NS) // 3 and 1000 < (cnt > 0).sum() < 3600 and (cnt > 1).sum() > 300
    every = [([lo[0], lo[1], -2**40], [hi[0], hi[1], 2**40]) for lo, hi in boxes]
    assert dev.check(every, cws, nx, ny).sum() > cnt.sum()
    # the rejected points hold the extremes: without the slab some cell's words differ
    a, b = dev.want(boxes, cws, nx, ny), dev.want(every, cws, nx, ny)
    assert (a[0] != b[0]).sum() > 500 and (a[1] != b[1]).sum() > 500


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 37), (37, 1), (3, 5)])
def test_small_dimensions(dev, nx, ny):
    cws = [(2 + k, 9 - k) for k in range(len(NS))]
    dev.upload(draw(np.random.default_rng(42 + nx + 100 * ny), nx, ny, cws))
    cnt = dev.check([box_of(k, nx, ny, cws[k]) for k in range(len(NS))], cws, nx, ny)
    assert 0 < cnt.sum() < sum(NS) // 2 + 400 and cnt.min() > 0


def test_hard_widths(dev):
    """(c) Widths 3, 7 and 641 with points planted at q cw - 1, q cw and q cw + 1 from the origin, on both axes"""
    nx, ny = 12, 9
    hard = (3, 7, 641)
    cws = [(hard[k % 3], hard[(k + 1) % 3]) for k in range(len(NS))]
    rng = np.random.default_rng(43)
    xyz = draw(rng, nx, ny, cws)
    for k, n in enumerate(NS):
        ox, oy = origin(k)
        for a, (o, dim) in enumerate(((ox, nx), (oy, ny))):
            edge = (o + np.repeat(np.arange(dim + 1), 3) * cws[k][a] + np.tile([-1, 0, 1], dim + 1)).astype(np.int32)
            at = rng.permutation(n)[:len(edge)]
            xyz[k][at, a] = edge[:len(at)]
    dev.upload(xyz)
    cnt = dev.check([box_of(k, nx, ny, cws[k]) for k in range(len(NS))], cws, nx, ny)
    assert 0 < cnt.sum() < sum(NS) and cnt.min() > 0


def test_two_calls_fold_into_the_same_words(dev):
    """(d) Two calls with different data into the same words equal one fold of both"""
    nx, ny = 16, 16
    n = len(NS)
    cws = [(3 + k, 4) for k in range(n)]
    boxes = [box_of(k, nx, ny, cws[k]) for k in range(n)]
    first, second = draw(np.random.default_rng(44), nx, ny, cws), draw(np.random.default_rng(45), nx, ny, cws)
    dev.preset((PRE_MIN, PRE_MAX))
    dev.upload(first)
    dev.launch(boxes, cws, nx, ny)
    one = dev.want(boxes, cws, nx, ny)
    dev.compare(one, nx, ny)
    dev.upload(second)  # (a synchronous copy behind the words' copy back: the first launch has ended)
    dev.launch(boxes, cws, nx, ny)
    both = dev.want(boxes, cws, nx, ny, pre=(one[0], one[1]))
    assert (both[0] != one[0]).sum() > 20 and (both[1] != one[1]).sum() > 20
    dev.compare(both, nx, ny)
    # ... and one launch over both halves of the data
    mixed = [np.concatenate([a[:len(a) // 2], b[len(b) // 2:]]) for a, b in zip(first, second)]
    dev.upload(mixed)
    dev.check(boxes, cws, nx, ny)


def test_on_a_callers_stream(dev):
    """(e) The same call on a caller's stream; the caller orders its outputs"""
    import torch
    nx, ny = 16, 16
    n = len(NS)
    cws = [(3 + k, 4) for k in range(n)]
    boxes = [box_of(k, nx, ny, cws[k]) for k in range(n)]
    dev.upload(draw(np.random.default_rng(46), nx, ny, cws))
    ts = torch.cuda.Stream()
    dev.preset((PRE_MIN, PRE_MAX))
    dev.launch(boxes, cws, nx, ny, stream=ts.cuda_stream)
    ts.synchronize()
    want = dev.want(boxes, cws, nx, ny)
    assert want[2].sum() > 1000
    dev.compare(want, nx, ny)
    dev.check(boxes, cws, nx, ny)  # (the last call of a test is on the context's own stream)


def test_empty_predicates_and_no_segments(dev):
    """(f) words unchanged"""
    nx, ny = 6, 7
    n = len(NS)
    cws = [(4 + k, 5) for k in range(n)]
    dev.upload(draw(np.random.default_rng(47), nx, ny, cws))
    boxes = [box_of(k, nx, ny, cws[k]) for k in range(n)]
    all_of = dev.check(boxes, cws, nx, ny).sum()
    odd = [EMPTY if k % 2 else boxes[k] for k in range(n)]
    assert 0 < dev.check(odd, cws, nx, ny).sum() < all_of  # (the odd segments would have matched: they are not evaluated)
    far_z = [([lo[0], lo[1], 2**31], [hi[0], hi[1], 2**40]) for lo, hi in boxes]  # outside the i32 range on z
    for none in ([EMPTY] * n, far_z):
        assert dev.check(none, cws, nx, ny).sum() == 0
        assert np.array_equal(dev.words()[0], PRE_MIN) and np.array_equal(dev.words()[1], PRE_MAX)
    assert dev.check([], [], nx, ny, []).sum() == 0  # nsegments == 0
    assert np.array_equal(dev.words()[0], PRE_MIN) and np.array_equal(dev.words()[1], PRE_MAX)


def test_refusals_leave_the_words_alone(dev):
    """(g) every refusal of the header comment"""
    nx, ny = 6, 7
    n = len(NS)
    cws = [(4 + k, 5) for k in range(n)]
    dev.upload(draw(np.random.default_rng(48), nx, ny, cws))
    boxes = [box_of(k, nx, ny, cws[k]) for k in range(n)]
    dev.check(boxes, cws, nx, ny)
    good = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
    dev.preset((PRE_MIN, PRE_MAX))

    def refused(cols=dev.cols, preds=good, cells=cws, nx=nx, ny=ny, d_zmin=None, d_zmax=None):
        with pytest.raises(binding.PcqError) as e:
            dev.launch(None, cells, nx, ny, cols=cols, preds=preds, d_zmin=d_zmin, d_zmax=d_zmax)
        assert e.value.code == PCQ_ERR_ARG, e.value
        lo, hi = dev.words()
        assert np.array_equal(lo, PRE_MIN) and np.array_equal(hi, PRE_MAX)

    def swapped(seq, k, v):
        out = list(seq)
        out[k] = v
        return out

    refused(d_zmin=0), refused(d_zmax=0)               # a null argument
    refused(nx=0), refused(ny=0), refused(nx=65, ny=64), refused(nx=CELLS_MAX + 1, ny=1), refused(nx=64, ny=128), refused(nx=2**31, ny=2**31)
    for bad in (pkg.Predicate.classification(2), pkg.Predicate.bounds_class(*boxes[3], 2)):  # any other predicate kind
        refused(preds=swapped(good, 3, bad))
    c = dev.cols[5]
    for bad in (binding.make_columns(xyz=c.xyz, n=100, xyz_stride=20), binding.make_columns(xyz=c.xyz + 4, n=c.n - 1),
                binding.make_columns(xyz=None, n=100)):                                      # stride, alignment, null positions with points
        refused(cols=swapped(dev.cols, 5, bad))
    refused(cells=swapped(cws, 4, (0, 5))), refused(cells=swapped(cws, 4, (8, 0)))           # a cell width of 0 in a non-empty segment
    lo, hi = boxes[2]
    for a in (0, 1):
        out = pkg.Predicate.bounds(swapped(lo, a, I32_MIN - 1), hi)                          # lmin outside the i32 range
        refused(preds=swapped(good, 2, out), cells=swapped(cws, 2, (2**30, 2**30)))
        reach = pkg.Predicate.bounds(lo, swapped(hi, a, hi[a] + 1))                          # one lattice step beyond the raster
        refused(preds=swapped(good, 2, reach))
        refused(preds=swapped(good, 2, pkg.Predicate.bounds(lo, swapped(hi, a, 2**40))))
    # a width of 0 in the segment without points is nothing to refuse, and the table stored before the refusals serves the next call
    dev.check(boxes, swapped(cws, 0, (0, 0)), nx, ny)
    dev.check(boxes, cws, nx, ny)


@pytest.mark.parametrize("nx,ny", [(64, 64), (3, 5)])
def test_reached_cells_are_the_density_rasters(dev, nx, ny):
    """(h) On case (b)'s data the cells with zmin <= zmax are exactly those where pcq_scan_dev_raster_batch counts more than 0"""
    full = (nx, ny) == (64, 64)
    cws = [(1, 1)] * len(NS) if full else [(2 + k, 9 - k) for k in range(len(NS))]
    dev.upload(draw(np.random.default_rng(41 if full else 42 + nx + 100 * ny), nx, ny, cws))
    boxes = [box_of(k, nx, ny, cws[k]) for k in range(len(NS))]
    cnt = dev.check(boxes, cws, nx, ny, pre=NOTHING)
    lo, hi = dev.words()
    dev.ctx.memset(dev.d_cnt, 0, 8 * nx * ny)
    dev.ctx.scan_dev_raster_batch(dev.cols, [pkg.Predicate.bounds(b[0], b[1]) for b in boxes], cws, nx, ny, dev.d_cnt)
    counts = np.zeros(nx * ny, dtype=np.uint64)
    dev.ctx.to_host(counts, dev.d_cnt)
    assert np.array_equal(counts.astype(np.int64), cnt)
    assert np.array_equal(lo[:nx * ny] <= hi[:nx * ny], counts > 0) and (not full or 0 < (counts == 0).sum())
