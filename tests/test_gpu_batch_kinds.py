"""The four batched counts share one segment table (pcq_upload_segment_table: d_segments / h_segments of the context): box,
class, box AND class and box AND time on one context over the same seven small segments, called in an order that holds every
ordered pair of kinds — each kind twice in a row too, with one segment's predicate changed in between.  Every total against
numpy.

A table travels only when it differs from the one in HBM, and every kind here has as many segments as every other: an upload
that looked at the segment count alone would keep the previous call's table — the second call (box after box, one box wider)
already shows it, before any table of another layout could be read as this one's.

Segments of n = 0, 1, 511, 512, 513, 1535, 4133 points (a step of the pipeline is 512 points: none, one less, exactly one, one
more, one less than three, eight and a few), positions pieces 16-byte aligned, class blocks at byte offsets 0..3 of a dword,
time blocks at 0 and 8 modulo 16.
"""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

NS = (0, 1, 511, 512, 513, 1535, 4133)
BOX, CLASS, BOX_CLASS, BOX_TIME = range(4)
# every ordered pair of the four kinds, the equal ones included, in seventeen calls
ORDER = (0, 0, 1, 1, 0, 2, 1, 2, 0, 3, 1, 3, 2, 2, 3, 3, 0)
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
        self.blocks = [ctx.alloc(size + 64) for size in (psize, csize, tsize, 64)]
        d_pos, d_cls, d_t, self.d_total = self.blocks
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

    def count(self, kind, visit):
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
    assert pairs == {(a, b) for a in range(4) for b in range(4)}
    s = Segments(gpu_ctx)
    try:
        visits = [0, 0, 0, 0]
        for call, kind in enumerate(ORDER):
            got, want, per_segment = s.count(kind, visits[kind])
            if visits[kind]:  # one predicate changed since this kind's last call, and with it the answer
                assert s.query(kind, VARIED, visits[kind])[1] != s.query(kind, VARIED, visits[kind] - 1)[1]
            assert all(w > 0 for w, n in zip(per_segment, NS) if n >= 511)
            assert got == want, f"call {call}: kind {kind} after {ORDER[call - 1] if call else None}, visit {visits[kind]}: got - want = {got - want}"
            visits[kind] += 1
    finally:
        s.free()
