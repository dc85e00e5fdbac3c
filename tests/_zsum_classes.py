"""What the tests of pcq_scan_dev_zsum_raster_batch_classes share: segments of positions and class bytes carved from two buffers in
HBM — the positions pieces 16-byte aligned, class piece k at byte misalignment mis[k] of a dword — two arrays of preset words, and
numpy's answer on int64: into a copy of the presets, np.add.at of 1 and of z over the points that pp.in_box keeps and whose class
byte is in the set.  Nothing here is a test."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

CELLS_MAX = 2048
WORDS = CELLS_MAX + 64
PRE_CNT = np.asarray([(0, 2**32 - 1, 2**40 + c)[c % 3] for c in range(WORDS)], dtype=np.int64)
PRE_SUM = np.asarray([(0, -1, 2**62, -2**62 + c)[c % 4] for c in range(WORDS)], dtype=np.int64)
ZEROS = np.zeros(WORDS, dtype=np.int64), np.zeros(WORDS, dtype=np.int64)
ALL = tuple(range(256))


def origin(k):
    return 1000 * k - 300, 77 - 500 * k


def box_of(k, nx, ny, cw, z=None):
    """Segment k's box: nx x ny full cells from its origin, and a slab of z that keeps about half of -50 .. 49"""
    ox, oy = origin(k)
    zlo, zhi = (-25 + k, 24 - k) if z is None else z
    return [ox, oy, zlo], [ox + nx * cw[0] - 1, oy + ny * cw[1] - 1, zhi]


def draw(rng, ns, nx, ny, cws, classes=(0, 1, 2, 3, 9, 31, 32, 200, 255), margin=2):
    """(positions, class bytes) of every segment: x and y independent over the segment's raster and `margin` lattice steps around it,
    z in -50 .. 49, and a class byte drawn from `classes` independently of all three"""
    xyz, cls = [], []
    for k, n in enumerate(ns):
        ox, oy = origin(k)
        xyz.append(np.stack([ox + rng.integers(-margin, nx * cws[k][0] + margin, n), oy + rng.integers(-margin, ny * cws[k][1] + margin, n),
                             rng.integers(-50, 50, n)], axis=1).astype(np.int32))
        cls.append(rng.choice(np.asarray(classes, dtype=np.uint8), n))
    return xyz, cls


def in_set(cls, classes):
    """numpy's membership of class bytes in a set of classes"""
    table = np.zeros(256, dtype=bool)
    table[list(classes)] = True
    return table[np.asarray(cls, dtype=np.uint8)]


class Dev:
    """Segments of ns[k] points.  upload(xyz, cls, mis) lays the data out; launch / want / check / compare as in
    test_gpu_zsum_raster.py, with the set of classes."""

    def __init__(self, ctx, ns):
        self.ctx, self.ns = ctx, tuple(ns)
        self.poff, self.psize = pp.carve(self.ns, [0] * len(self.ns), 12)
        _, self.csize = pp.carve(self.ns, [15] * len(self.ns), 1)  # (room for every phase)
        self.blocks = [ctx.alloc(self.psize + 64), ctx.alloc(self.csize + 64), ctx.alloc(8 * WORDS), ctx.alloc(8 * WORDS)]
        self.d_pos, self.d_cls, self.d_cnt, self.d_sum = self.blocks
        assert all(p % 16 == 0 for p in self.blocks) and all(o % 16 == 0 for o in self.poff)
        self.xyz = self.cls = self.cols = self.mis = None

    def upload(self, xyz, cls, mis):
        assert [len(a) for a in xyz] == list(self.ns) == [len(c) for c in cls] and len(mis) == len(self.ns)
        img = np.zeros(self.psize, dtype=np.uint8)
        for o, a in zip(self.poff, xyz):
            img[o:o + a.nbytes] = np.ascontiguousarray(a, dtype=np.int32).view(np.uint8).reshape(-1)
        self.ctx.to_device(self.d_pos, img)
        coff, csize = pp.carve(self.ns, list(mis), 1)
        assert csize <= self.csize
        cimg = np.full(self.csize + 64, 0xa5, dtype=np.uint8)  # (a byte of no set used here is not assumed: the tests' sets decide)
        for o, c in zip(coff, cls):
            cimg[o:o + len(c)] = np.asarray(c, dtype=np.uint8)
        self.ctx.to_device(self.d_cls, cimg)
        self.xyz, self.cls, self.mis = list(xyz), [np.asarray(c, dtype=np.uint8) for c in cls], list(mis)
        self.cols = [binding.make_columns(xyz=self.d_pos + p, cls=self.d_cls + c, n=n) for p, c, n in zip(self.poff, coff, self.ns)]
        assert [(self.d_cls + c) % 4 for c in coff] == [m % 4 for m in mis]

    def want(self, boxes, cws, nx, ny, classes, segments=None, pre=(PRE_CNT, PRE_SUM)):
        cnt, zsum = pre[0].copy(), pre[1].copy()
        for k, (lo, hi), cw in zip(range(len(self.ns)) if segments is None else segments, boxes, cws):
            keep = pp.in_box(self.xyz[k], lo, hi) & in_set(self.cls[k], classes)
            p = self.xyz[k][keep].astype(np.int64)
            cell = ((p[:, 1] - int(lo[1])) // int(cw[1])) * nx + (p[:, 0] - int(lo[0])) // int(cw[0])
            assert not len(cell) or (0 <= cell.min() and cell.max() < nx * ny)
            np.add.at(cnt, cell, 1)
            np.add.at(zsum, cell, p[:, 2])
        return cnt, zsum

    def preset(self, pre=(PRE_CNT, PRE_SUM)):
        self.ctx.to_device(self.d_cnt, np.ascontiguousarray(pre[0], dtype=np.int64))
        self.ctx.to_device(self.d_sum, np.ascontiguousarray(pre[1], dtype=np.int64))

    def words(self):
        cnt, zsum = np.zeros(WORDS, dtype=np.int64), np.zeros(WORDS, dtype=np.int64)
        self.ctx.to_host(cnt, self.d_cnt)  # (waits for the context's stream)
        self.ctx.to_host(zsum, self.d_sum)
        return cnt, zsum

    def launch(self, boxes, cws, nx, ny, classes, segments=None, cols=None, preds=None, d_count=None, d_zsum=None, stream=None):
        if cols is None:
            cols = self.cols if segments is None else [self.cols[k] for k in segments]
        if preds is None:
            preds = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
        self.ctx.scan_dev_zsum_raster_batch_classes(cols, preds, cws, nx, ny, classes, self.d_cnt if d_count is None else d_count,
                                                    self.d_sum if d_zsum is None else d_zsum, stream=stream)

    def compare(self, want, what=""):
        got = self.words()
        for name, g, w in (("count", got[0], want[0]), ("sum", got[1], want[1])):
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (name, what, [(int(c), int(g[c]), int(w[c])) for c in bad[:12]], len(bad))

    def check(self, boxes, cws, nx, ny, classes, segments=None, pre=(PRE_CNT, PRE_SUM), stream=None):
        """One call from the preset words: every word of both arrays is numpy's; returns (points per cell, z sum per cell)"""
        self.preset(pre)
        self.launch(boxes, cws, nx, ny, classes, segments, stream=stream)
        want = self.want(boxes, cws, nx, ny, classes, segments, pre)
        self.compare(want, (nx, ny, sorted(classes)[:8], self.mis))
        return (want[0] - pre[0])[:nx * ny], (want[1] - pre[1])[:nx * ny]

    def unchanged(self):
        cnt, zsum = self.words()
        return np.array_equal(cnt, PRE_CNT) and np.array_equal(zsum, PRE_SUM)

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)
