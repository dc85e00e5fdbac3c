"""The eight batched kinds over two segment sets of one upload: what test_gpu_batch_all_kinds.py and test_gpu_batch_streams.py share.

The batched entries keep one set of state per context: the segment table (d_segments / h_segments, five layouts, re-uploaded
when pcq_upload_segment_table finds a difference, freed and reallocated when a table outgrows it), the partials (one slice per
output word, grown by pcq_ensure_partials), and the scratch stream (pcq_scratch_stream).  This module builds the data, each
kind's visit-th query with numpy's answer, the launch, and the arithmetic of what each launch asks of that state.

Data: a SMALL set of the seven sizes of test_gpu_batch_kinds.py and a LARGE set of 23 segments cycling through the same sizes
(224 B x 23 > the table buffer's initial 4096 B), carved from one buffer per column: positions 16-byte aligned, class blocks at
byte offsets 0..3 of a dword, time blocks at 0 and 8 modulo 16.  Positions are integers in 0..99, class bytes come from five
values, times are integers in 0..999 with NaN, -0.0 and +inf planted in every segment of at least 511 points.

Expected values are numpy on the host arrays only: pp.in_box and the reference helpers of test_gpu_raster.py (Dev.want),
test_gpu_class_hist.py (Segments.want) and test_gpu_time_hist.py (numpy_hist), called on a plain namespace that holds this
module's arrays; the multi-box rows of test_gpu_batch_multi.py are bound to its seven segments and are restated here.
"""
import functools
import importlib
import os
import sys
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402
import test_gpu_class_hist as class_hist_ref  # noqa: E402
import test_gpu_raster as raster_ref  # noqa: E402
import test_gpu_time_hist as time_hist_ref  # noqa: E402

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

KINDS = BOX, CLASS, BOX_CLASS, BOX_TIME, MULTI, CLASS_HIST, TIME_HIST, RASTER = range(8)
NAMES = ("BOX", "CLASS", "BOX_CLASS", "BOX_TIME", "MULTI", "CLASS_HIST", "TIME_HIST", "RASTER")
SIZES = (0, 1, 511, 512, 513, 1535, 4133)
SMALL, LARGE = 0, 1
SET_SIZES = (SIZES, tuple(SIZES[i % 7] for i in range(23)))
VARIED = 6  # the segment (4133 points in both sets) whose predicate changes from one call of a kind to its next

RASTER_CELLS_MAX = 8192            # include/pcq.h: PCQ_RASTER_CELLS_MAX
REGION = RASTER_CELLS_MAX + 64     # u64 words of output per call
NQUERIES = (2, 8, 1, 3, 5, 4, 7, 6)
NBINS = (8, 1024, 1, 5, 1023, 64, 2, 8)
RASTERS = ((8, 8), (64, 128), (1, 1), (3, 5), (128, 64), (1, 37), (91, 90), (8, 8))
ULP_VISIT = 8                      # the time histogram's visit that repeats visit 7's edges with one edge moved by one ulp
ULP_EDGE = 4
EMPTY = ([5, 5, 5], [4, 4, 4])

# every ordered pair of the eight kinds, the equal ones included, in 65 calls: the de Bruijn sequence B(8, 2) in its
# lexicographically least form (0 0 1 0 2 .. 0 7 1 1 2 .. 6 7 7) with its first symbol again at the end, its symbols shifted by
# TIME_HIST, backwards.  The time histogram is the kind with nine visits and the last two calls are its visits 7 and 8, with
# the same number of bins: test_gpu_batch_all_kinds.py runs visit 8 on visit 7's set with visit 7's predicates, so that the two
# uploads differ in one bit of one edge behind the table and in nothing else.  The first multi-box table of the large set
# (call 3) comes before any table with 1024 edges behind it: it is the multi-box table that outgrows the table buffer's first size.


def _de_bruijn(k):
    seq, a = [], [0] * (2 * k)

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)

    db(1, 1)
    return seq


ORDER = (tuple((s + TIME_HIST) % 8 for s in _de_bruijn(8)) + (TIME_HIST,))[::-1]

# pitches of the five table layouts (pcq_internal.h: DevSegment, DevCombinedSegment, DevRasterSegment, DevBoundsTimeSegment,
# DevMultiSegment, whose 224 bytes a static_assert holds), the table buffer's first size and the partials' first size in words
PITCH = {BOX: 48, CLASS: 48, BOX_CLASS: 64, BOX_TIME: 80, MULTI: 224, CLASS_HIST: 64, TIME_HIST: 80, RASTER: 72}
TABLE_BYTES_INITIAL = 4096
PARTIALS_WORDS_MIN = 4096
K1_STEP = pp.K1.step

Query = namedtuple("Query", "kind set visit varied args words want contrib table_bytes slices waves")


class Host:
    """The host arrays of both sets, per set a list of segments."""

    def __init__(self):
        rng = np.random.default_rng(2611)
        self.xyz = [[rng.integers(0, 100, size=(n, 3), dtype=np.int32) for n in sizes] for sizes in SET_SIZES]
        self.cls = [[rng.choice(np.asarray([1, 2, 3, 9, 200], dtype=np.uint8), n) for n in sizes] for sizes in SET_SIZES]
        self.t = [[rng.integers(0, 1000, size=n).astype(np.float64) for n in sizes] for sizes in SET_SIZES]
        for ts in self.t:
            for t in ts:
                if len(t) >= 511:
                    t[7] = t[-1] = np.nan
                    t[100] = -0.0
                    t[300] = np.inf

    def refs(self, s):
        """What the reference helpers of the single-kind tests read from their `self`"""
        return SimpleNamespace(xyz=self.xyz[s], cls=self.cls[s], t=self.t[s])


@functools.lru_cache(maxsize=None)
def host():
    return Host()


def box_of(k, v):
    return [10 + k % 7, 5, 0], [60 + k % 7 + 3 * v, 90, 99]


def multi_box(k, q, v, nq):
    """Box q of segment k; every box of VARIED changes with the visit, so that every word of the answer does; some rows hold an
    empty box (not asked of that segment)"""
    if nq > 1 and k != VARIED and (k + q) % 5 == 4:
        return EMPTY
    v = v if k == VARIED else 0
    return [10 + k % 7 + q, 5, 2 * q], [60 + k % 7 - 3 * q + 3 * v, 90, 99 - q]


def edges_of(visit):
    """Fresh non-decreasing edges per visit: whole and half numbers, so that times lie on edges; 0.0 in front at some visits,
    where -0.0 belongs to the first bin"""
    nbins = NBINS[visit % 8]
    if visit == ULP_VISIT:
        e = edges_of(visit - 1).copy()
        e[ULP_EDGE] = np.nextafter(e[ULP_EDGE], np.inf)
        return e
    if nbins == 8:
        return 100.0 * np.arange(1, 10) + visit
    rng = np.random.default_rng(900 + visit)
    first, last = (0.0 if visit % 4 == 3 else 100.0 + visit), 900.0 - visit
    inner = np.sort(rng.integers(220, 1781, nbins - 1)) / 2.0
    return np.concatenate([[first], inner, [last]])


def cell_widths(boxes, nx, ny):
    """Per segment the smallest widths at which its box fits nx x ny cells, and 0..2 more: they differ between segments"""
    out = []
    for k, (lo, hi) in enumerate(boxes):
        out.append((-(-(hi[0] - lo[0] + 1) // nx) + k % 3, -(-(hi[1] - lo[1] + 1) // ny) + (k + 1) % 3))
    return out


def raster_waves(cells):
    """scan_raster.hip: 16 waves per CU, as many as their rasters fit in 160 KiB of LDS, whole SIMDs beyond four"""
    w = min(16, 160 * 1024 // (cells * 4))
    return w & ~3 if w > 4 else w


@functools.lru_cache(maxsize=None)
def query(kind, s, visit, varied=None):
    """The kind's visit-th call on set s: its arguments, numpy's answer (`words` of them), each segment's share of it.
    Only segment VARIED's predicate depends on the visit (`varied`: that segment at another visit, everything else as it is);
    the launch-level parameters (nqueries, edges, raster and cell widths) cycle by the visit."""
    h = host()
    n = len(SET_SIZES[s])
    vv = visit if varied is None else varied
    at = [vv if k == VARIED else 0 for k in range(n)]
    boxes = [box_of(k, at[k]) for k in range(n)]
    inside = [pp.in_box(h.xyz[s][k], *boxes[k]) for k in range(n)]
    preds = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
    slices, waves, extra = 1, pp.K1.waves_per_cu, 0
    if kind == BOX:
        contrib = [int(m.sum()) for m in inside]
        args, want = (preds,), [sum(contrib)]
    elif kind == CLASS:
        c = [1 + (k + at[k]) % 3 for k in range(n)]
        contrib = [pp.class_count(h.cls[s][k], c[k]) for k in range(n)]
        args, want, waves = ([pkg.Predicate.classification(x) for x in c],), [sum(contrib)], pp.K2.waves_per_cu
    elif kind == BOX_CLASS:
        c = [1 + (k + at[k]) % 3 for k in range(n)]
        contrib = [int((inside[k] & (h.cls[s][k] == c[k])).sum()) for k in range(n)]
        args, want = ([pkg.Predicate.bounds_class(*boxes[k], c[k]) for k in range(n)],), [sum(contrib)]
    elif kind == BOX_TIME:
        r = [(100.0 + 10 * (k % 7), 600.0 + 10 * (k % 7) + 25 * at[k]) for k in range(n)]
        contrib = [int((inside[k] & pp.in_range(h.t[s][k], *r[k])).sum()) for k in range(n)]
        args, want = ([pkg.Predicate.bounds_time(*boxes[k], *r[k]) for k in range(n)],), [sum(contrib)]
    elif kind == MULTI:
        nq = NQUERIES[visit % 8]
        rows = [[multi_box(k, q, vv, nq) for q in range(nq)] for k in range(n)]
        per = np.asarray([[pp.box_count(h.xyz[s][k], *rows[k][q]) for q in range(nq)] for k in range(n)], dtype=np.int64)
        contrib = [per[k] for k in range(n)]
        args, want = ([[pkg.Predicate.bounds(lo, hi) for lo, hi in row] for row in rows],), per.sum(axis=0)
        if nq > 1:  # (one box: the plain box entry, its table and its grid)
            slices, waves = (2 if nq <= 2 else 4 if nq <= 4 else 8), 12
    elif kind == CLASS_HIST:
        contrib = [int(m.sum()) for m in inside]
        args, want = (preds,), class_hist_ref.Segments.want(h.refs(s), boxes, range(n))
        slices, waves = 256, 4
    elif kind == TIME_HIST:
        e = edges_of(visit)
        contrib = [int(time_hist_ref.numpy_hist(h.t[s][k][inside[k]], [e[0], e[-1]])[0]) for k in range(n)]
        passing = np.concatenate([h.t[s][k][inside[k]] for k in range(n)])
        args, want = (preds, e), time_hist_ref.numpy_hist(passing, e)
        slices, waves, extra = len(e) - 1, 12, 8 * (len(e) + 1)  # (behind the table: the bin count and the edges)
    else:
        nx, ny = RASTERS[visit % 8]
        cws = cell_widths(boxes, nx, ny)
        contrib = [int(m.sum()) for m in inside]
        args, want = (preds, cws, nx, ny), raster_ref.Dev.want(h.refs(s), boxes, cws, nx, ny, range(n)).reshape(-1)
        slices, waves = nx * ny, raster_waves(nx * ny)
    want = np.asarray(want, dtype=np.int64)
    pitch = PITCH[BOX] if (kind == MULTI and slices == 1) else PITCH[kind]
    return Query(kind, s, visit, vv, args, len(want), want, contrib, pitch * n + extra, slices, waves)


def check_not_vacuous(q):
    """Every segment of at least 511 points gives more than none and fewer than all of its points to the answer, and VARIED's
    share is another one than at the kind's previous visit (the visit that repeats its predecessor's predicates apart: there
    the moved edge has to move a point)"""
    for k, n in enumerate(SET_SIZES[q.set]):
        if n >= 511:
            c = np.asarray(q.contrib[k])
            assert c.max() > 0 and c.max() < n, (NAMES[q.kind], q.set, q.visit, k, c)
    if q.visit and q.varied == q.visit:
        before = query(q.kind, q.set, q.visit, q.visit - 1)
        assert not np.array_equal(q.want, before.want) and not np.array_equal(q.contrib[VARIED], before.contrib[VARIED]), (NAMES[q.kind], q.visit)
    if q.kind == TIME_HIST and q.visit == ULP_VISIT:
        e = edges_of(q.visit - 1)
        assert np.array_equal(np.flatnonzero(q.args[1] != e), [ULP_EDGE])
        passing = np.concatenate([host().t[q.set][k][pp.in_box(host().xyz[q.set][k], *box_of(k, q.varied if k == VARIED else 0))]
                                  for k in range(len(SET_SIZES[q.set]))])
        assert not np.array_equal(q.want, time_hist_ref.numpy_hist(passing, e)), "the moved edge moves no point"


class Dev:
    """Both sets on the device of a context of its own, and one output region of REGION words per call, preset to distinct
    non-zero words"""

    def __init__(self, ctx, ncalls):
        self.ctx, self.ncalls = ctx, ncalls
        h = host()
        sizes = SET_SIZES[SMALL] + SET_SIZES[LARGE]
        nseg = len(sizes)
        poff, psize = pp.carve(sizes, [0] * nseg, 12)
        coff, csize = pp.carve(sizes, [(5 * i) % 16 for i in range(nseg)])
        toff, tsize = pp.carve(sizes, [8 * (i % 2) for i in range(nseg)], 8)
        self.blocks = [ctx.alloc(size + 64) for size in (psize, csize, tsize, 8 * REGION * ncalls)]
        d_pos, d_cls, d_t, self.d_out = self.blocks
        assert all(p % 16 == 0 for p in self.blocks) and all(o % 16 == 0 for o in poff)
        assert {(d_cls + o) % 4 for o, n in zip(coff, sizes) if n} == {0, 1, 2, 3}
        assert {(d_t + o) % 16 for o, n in zip(toff, sizes) if n} == {0, 8}
        for base, size, offs, parts in ((d_pos, psize, poff, h.xyz[SMALL] + h.xyz[LARGE]), (d_cls, csize, coff, h.cls[SMALL] + h.cls[LARGE]),
                                        (d_t, tsize, toff, h.t[SMALL] + h.t[LARGE])):
            img = np.zeros(size, dtype=np.uint8)
            for o, a in zip(offs, parts):
                img[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            ctx.to_device(base, img)
        self.cols, self.class_addr = [], []
        for s, first in ((SMALL, 0), (LARGE, len(SET_SIZES[SMALL]))):
            seg = [(d_pos + poff[first + k], d_cls + coff[first + k], d_t + toff[first + k], n) for k, n in enumerate(SET_SIZES[s])]
            plain = [binding.make_columns(xyz=p, n=n) for p, c, t, n in seg]
            with_class = [binding.make_columns(xyz=p, cls=c, n=n) for p, c, t, n in seg]
            with_time = [binding.make_columns(xyz=p, cls=t, n=n, cls_stride=8) for p, c, t, n in seg]
            self.cols.append({BOX: plain, MULTI: plain, RASTER: plain, CLASS: [binding.make_columns(cls=c, n=n) for p, c, t, n in seg],
                              BOX_CLASS: with_class, CLASS_HIST: with_class, BOX_TIME: with_time, TIME_HIST: with_time})
            self.class_addr.append([c for p, c, t, n in seg])
        self.preset = (1000 + 7 * np.arange(REGION * ncalls)).astype(np.uint64)
        ctx.to_device(self.d_out, self.preset)
        self.entry = {BOX: ctx.scan_dev_count_batch, CLASS: ctx.scan_dev_count_batch, BOX_CLASS: ctx.scan_dev_count_batch_combined,
                      BOX_TIME: ctx.scan_dev_count_batch_bounds_time, MULTI: ctx.scan_dev_count_batch_multi,
                      CLASS_HIST: ctx.scan_dev_class_hist_batch, TIME_HIST: ctx.scan_dev_time_hist_batch, RASTER: ctx.scan_dev_raster_batch}

    def launch(self, q, call, stream=None):
        """The query into the call's region; stream: a hipStream_t as an integer, or the context's own"""
        self.entry[q.kind](self.cols[q.set][q.kind], *q.args, self.d_out + 8 * REGION * call, stream=stream)

    def region(self, call):
        out = np.zeros(REGION, dtype=np.uint64)
        self.ctx.to_host(out, self.d_out + 8 * REGION * call)  # (waits for the context's stream)
        return out

    def regions(self):
        out = np.zeros(REGION * self.ncalls, dtype=np.uint64)
        self.ctx.to_host(out, self.d_out)  # (waits for the context's stream)
        return out.reshape(self.ncalls, REGION)

    def wrong(self, words, q, call):
        """None, or what is wrong with the call's region: the difference to the preset words is numpy's answer over the kind's
        words and nothing behind them"""
        added = words.astype(np.int64) - self.preset[REGION * call:REGION * (call + 1)].astype(np.int64)
        bad = np.flatnonzero(added[:q.words] != q.want)
        if len(bad):
            return f"got - want {[(int(b), int(added[b] - q.want[b])) for b in bad[:8]]} ({len(bad)} of {q.words} words)"
        behind = np.flatnonzero(added[q.words:])
        if len(behind):
            return f"words behind the answer changed: {[(int(b) + q.words, int(added[b + q.words])) for b in behind[:8]]}"
        return None

    def workgroups(self, q, cus):
        """The launch's grid (scan_batch_host.h, scan_count.hip: min(CUs x waves, steps + segments))"""
        sizes = SET_SIZES[q.set]
        if q.kind == CLASS:
            steps = sum(pp.class_layout(a, n)[2] for a, n in zip(self.class_addr[q.set], sizes))
            return pp.batch_grid(pp.K2, cus, steps, len(sizes))
        return pp.batch_grid(pp.Family(NAMES[q.kind], q.waves, K1_STEP), cus, sum(n // K1_STEP for n in sizes), len(sizes))

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


def regrowths(dev, queries, cus):
    """From the arithmetic of pcq_ensure_segment_table and pcq_ensure_partials: the calls at which the table buffer and the
    partials are freed and reallocated, with the new sizes"""
    table_cap, words_cap = 0, PARTIALS_WORDS_MIN
    while words_cap < cus * 16:  # (pcq_init asks for 16 words per CU)
        words_cap <<= 1
    tables, partials = [], []
    for call, q in enumerate(queries):
        if q.table_bytes > table_cap:
            table_cap = max(q.table_bytes, TABLE_BYTES_INITIAL)
            if call:
                tables.append((call, table_cap))
        need = dev.workgroups(q, cus) * q.slices
        if need > words_cap:
            while words_cap < need:
                words_cap <<= 1
            partials.append((call, need, words_cap))
    return tables, partials
