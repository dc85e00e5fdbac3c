"""The batched entries share one segment table (pcq_upload_segment_table: d_segments / h_segments of the context): box,
class, box AND class and box AND time, and with them the height raster, the mean-height raster, its class-filtered twin and the
polygon count, on one context over the same seven small segments, called in an order that holds every ordered pair of kinds —
each kind twice in a row too, with one segment's predicate changed in between.  Every total, and every word of the rasters,
against numpy (the rasters' and the polygon's through the reference helpers of their own tests, as _batch_all_kinds.py does).

A table travels only when it differs from the one in HBM, and every kind here has as many segments as every other: an upload
that looked at the segment count alone would keep the previous call's table — the second call (box after box, one box wider)
already shows it, before any table of another layout could be read as this one's.

Segments of n = 0, 1, 511, 512, 513, 1535, 4133 points (a step of the pipeline is 512 points: none, one less, exactly one, one
more, one less than three, eight and a few), positions pieces 16-byte aligned, class blocks at byte offsets 0..3 of a dword,
time blocks at 0 and 8 modulo 16.
"""
import importlib
from types import SimpleNamespace

import numpy as np
import pytest

import _batch_all_kinds as ak
import _polygon_rule as polygon_ref
import _zsum_classes as zsum_classes_ref
import test_gpu_zrange_raster as zrange_ref
import test_gpu_zsum_raster as zsum_ref

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

NS = (0, 1, 511, 512, 513, 1535, 4133)
KINDS = BOX, CLASS, BOX_CLASS, BOX_TIME, ZRANGE, ZSUM, ZSUM_CLASSES, POLYGON = range(8)
COUNTS = KINDS[:4]
# every ordered pair of the eight kinds, the equal ones included, in 65 calls: a de Bruijn sequence with its first symbol again at the end
ORDER = tuple(ak._de_bruijn(8)) + (0,)
# the launch-level parameters of the four later kinds cycle by the visit
ZRANGE_SHAPES = ((8, 8), (64, 64), (1, 1), (3, 5), (1, 37))
ZSUM_SHAPES = ((8, 8), (64, 32), (1, 1), (3, 5))
CLASS_SETS = ((1,), tuple(range(256)), (1, 3), tuple(c for c in range(256) if c != 2), (2, 3))
NVERTS = (3, 4, 5, 256, 255, 8)
VARIED = 6  # the segment whose predicate changes from one call of a kind to its next


def carve(sizes, residues, modulo):
    """offsets of blocks of `sizes` bytes, block k at residues[k] modulo `modulo`, 64 bytes apart at least; the whole size"""
    offs, at = [], 0
    for size, r in zip(sizes, residues):
        at += (r - at) % modulo
        offs.append(at)
        at += size + 64
    return offs, at


class Segments:
    def __init__(self, ctx):
        self.ctx = ctx
        rng = np.random.default_rng(1812)
        self.xyz = [rng.integers(0, 100, size=(n, 3), dtype=np.int32) for n in NS]
        self.cls = [rng.integers(1, 4, size=n, dtype=np.uint8) for n in NS]
        self.t = [rng.integers(0, 1000, size=n).astype(np.float64) for n in NS]
        poff, psize = carve([12 * n for n in NS], [0] * len(NS), 16)
        coff, csize = carve(list(NS), [k % 4 for k in range(len(NS))], 4)
        toff, tsize = carve([8 * n for n in NS], [8 * (k % 2) for k in range(len(NS))], 16)
        self.blocks = [ctx.alloc(size + 64) for size in (psize, csize, tsize, 64, 8 * zrange_ref.WORDS, 8 * zrange_ref.WORDS)]
        d_pos, d_cls, d_t, self.d_total, self.d_a, self.d_b = self.blocks
        assert all(p % 16 == 0 for p in self.blocks)
        assert {(d_cls + o) % 4 for o in coff} == {0, 1, 2, 3} and {(d_t + o) % 16 for o in toff} == {0, 8}
        for base, size, offs, parts in ((d_pos, psize, poff, self.xyz), (d_cls, csize, coff, self.cls), (d_t, tsize, toff, self.t)):
            img = np.zeros(size, dtype=np.uint8)
            for o, a in zip(offs, parts):
                img[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
            ctx.to_device(base, img)
        self.cols = {
            BOX: [binding.make_columns(xyz=d_pos + p, n=n) for p, n in zip(poff, NS)],
            CLASS: [binding.make_columns(cls=d_cls + c, n=n) for c, n in zip(coff, NS)],
            BOX_CLASS: [binding.make_columns(xyz=d_pos + p, cls=d_cls + c, n=n) for p, c, n in zip(poff, coff, NS)],
            BOX_TIME: [binding.make_columns(xyz=d_pos + p, cls=d_t + t, n=n, cls_stride=8) for p, t, n in zip(poff, toff, NS)],
        }
        self.cols.update({ZRANGE: self.cols[BOX], ZSUM: self.cols[BOX], POLYGON: self.cols[BOX], ZSUM_CLASSES: self.cols[BOX_CLASS]})
        self.entry = {BOX: ctx.scan_dev_count_batch, CLASS: ctx.scan_dev_count_batch, BOX_CLASS: ctx.scan_dev_count_batch_combined,
                      BOX_TIME: ctx.scan_dev_count_batch_bounds_time}

    def query(self, kind, k, visit):
        """Segment k's predicate at the kind's visit-th call, and numpy's count.  Only segment VARIED depends on the visit."""
        v = visit if k == VARIED else 0
        lo, hi = [10 + k, 5, 0], [60 + k + 3 * v, 90, 99]
        cls, (t0, t1) = 1 + (k + v) % 3, (100.0 + 10 * k, 600.0 + 10 * k + 25 * v)
        x = self.xyz[k].astype(np.int64)
        box = np.all((x >= lo) & (x <= hi), axis=1)
        if kind == BOX:
            return pkg.Predicate.bounds(lo, hi), int(box.sum())
        if kind == CLASS:
            return pkg.Predicate.classification(cls), int((self.cls[k] == cls).sum())
        if kind == BOX_CLASS:
            return pkg.Predicate.bounds_class(lo, hi, cls), int((box & (self.cls[k] == cls)).sum())
        return pkg.Predicate.bounds_time(lo, hi, t0, t1), int((box & (self.t[k] >= t0) & (self.t[k] < t1)).sum())

    def later(self, kind, visit):
        """A call of one of the four later kinds at its visit-th shape, from "nothing yet" or zeroed words: (what the device
        holds, numpy's answer, the points of each segment in it).  The boxes are the box kind's with a z slab that widens with the
        visit, so that the height raster's few-cell shapes change with it too."""
        n = len(NS)
        v = [visit if k == VARIED else 0 for k in range(n)]
        boxes = [([10 + k, 5, 30 - k - v[k]], [60 + k + 3 * v[k], 90, 64 + k + v[k]]) for k in range(n)]
        preds = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
        inside = [polygon_ref.in_box(self.xyz[k], *boxes[k]) for k in range(n)]
        if kind == POLYGON:
            m = NVERTS[visit % len(NVERTS)]
            verts = [ak.outline(k, v[k], m) for k in range(n)]
            per = [int(polygon_ref.counted(self.xyz[k], *boxes[k], verts[k]).sum()) for k in range(n)]
            self.ctx.memset(self.d_total, 0, 8)
            self.ctx.scan_dev_count_batch_polygon(self.cols[kind], preds, [[(int(x), int(y)) for x, y in o] for o in verts], self.d_total)
            out = np.zeros(1, dtype=np.uint64)
            self.ctx.to_host(out, self.d_total)  # (waits for the context's stream)
            return out.astype(np.int64), np.asarray([sum(per)], dtype=np.int64), per
        nx, ny = (ZRANGE_SHAPES if kind == ZRANGE else ZSUM_SHAPES)[visit % len(ZRANGE_SHAPES if kind == ZRANGE else ZSUM_SHAPES)]
        cws = ak.cell_widths(boxes, nx, ny)
        refs = SimpleNamespace(ns=NS, xyz=self.xyz, cls=self.cls)
        if kind == ZRANGE:
            pre, words, dtype = zrange_ref.NOTHING, zrange_ref.WORDS, np.int32
            want = zrange_ref.Dev.want(refs, boxes, cws, nx, ny, range(n), pre=pre)[:2]
            per = [int(m.sum()) for m in inside]
            args = (preds, cws, nx, ny)
            entry = self.ctx.scan_dev_zrange_raster_batch
        elif kind == ZSUM:
            pre, words, dtype = zsum_ref.ZEROS, zsum_ref.WORDS, np.int64
            want = zsum_ref.Dev.want(refs, boxes, cws, nx, ny, range(n), pre=pre)
            per = [int(m.sum()) for m in inside]
            args = (preds, cws, nx, ny)
            entry = self.ctx.scan_dev_zsum_raster_batch
        else:
            classes = CLASS_SETS[visit % len(CLASS_SETS)]
            pre, words, dtype = zsum_classes_ref.ZEROS, zsum_classes_ref.WORDS, np.int64
            want = zsum_classes_ref.Dev.want(refs, boxes, cws, nx, ny, classes, range(n), pre=pre)
            per = [int((inside[k] & zsum_classes_ref.in_set(self.cls[k], classes)).sum()) for k in range(n)]
            args = (preds, cws, nx, ny, classes)
            entry = self.ctx.scan_dev_zsum_raster_batch_classes
        got = [np.zeros(words, dtype=dtype), np.zeros(words, dtype=dtype)]
        for d, a in zip((self.d_a, self.d_b), pre):
            self.ctx.to_device(d, np.ascontiguousarray(a, dtype=dtype))
        entry(self.cols[kind], *args, self.d_a, self.d_b)
        for d, a in zip((self.d_a, self.d_b), got):
            self.ctx.to_host(a, d)  # (waits for the context's stream)
        return np.concatenate(got).astype(np.int64), np.concatenate(want).astype(np.int64), per

    def count(self, kind, visit):
        if kind not in COUNTS:
            return self.later(kind, visit)
        preds, want = zip(*(self.query(kind, k, visit) for k in range(len(NS))))
        self.ctx.memset(self.d_total, 0, 8)
        self.entry[kind](self.cols[kind], list(preds), self.d_total)
        out = np.zeros(1, dtype=np.uint64)
        self.ctx.to_host(out, self.d_total)  # (waits for the context's stream)
        return int(out[0]), sum(want), want

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


def test_every_kind_after_every_kind_on_one_segment_table(gpu_ctx):
    pairs = set(zip(ORDER, ORDER[1:]))
    assert pairs == {(a, b) for a in KINDS for b in KINDS}
    s = Segments(gpu_ctx)
    try:
        visits, before = [0] * len(KINDS), {}
        for call, kind in enumerate(ORDER):
            got, want, per_segment = s.count(kind, visits[kind])
            if visits[kind]:  # one predicate changed since this kind's last call, and with it the answer
                if kind in COUNTS:
                    assert s.query(kind, VARIED, visits[kind])[1] != s.query(kind, VARIED, visits[kind] - 1)[1]
                else:
                    assert per_segment[VARIED] != before[kind][0][VARIED] and not np.array_equal(want, before[kind][1])
            before[kind] = (list(per_segment), want)
            assert all(w > 0 for w, n in zip(per_segment, NS) if n >= 511)
            wrong = np.flatnonzero(np.atleast_1d(got != want))
            assert len(wrong) == 0, (f"call {call}: kind {kind} after {ORDER[call - 1] if call else None}, visit {visits[kind]}: (word, got - want) = "
                                     f"{[(int(w), int(np.atleast_1d(got)[w] - np.atleast_1d(want)[w])) for w in wrong[:8]]}")
            visits[kind] += 1
    finally:
        s.free()
