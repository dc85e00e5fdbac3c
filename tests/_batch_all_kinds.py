"""The twelve batched kinds over two segment sets of one upload: what test_gpu_batch_all_kinds.py and test_gpu_batch_streams.py share.

The batched entries keep one set of state per context: the segment table (d_segments / h_segments, eight layouts, re-uploaded
when pcq_upload_segment_table finds a difference, freed and reallocated when a table outgrows it), the partials (one slice per
output word, grown by pcq_ensure_partials), and the scratch stream (pcq_scratch_stream).  This module builds the data, each
kind's visit-th query with numpy's answer, the launch, and the arithmetic of what each launch asks of that state.

The first eight kinds (KINDS8) add into the first words of their region.  The four that came later use the state in ways of
their own: the height raster (ZRANGE) uploads under the density raster's table kind and FOLDS with a signed min / max into two
i32 arrays; the mean-height raster (ZSUM) shares that table kind too, has 2 x cells slices and two finishes, into two u64
arrays; its class-filtered twin (ZSUM_CLASSES) has a table kind of its own and its class set in the kernel's arguments; the
polygon count (POLYGON) has its edges in a trailer behind the table, whose size changes with the vertex count.

Data: a SMALL set of the seven sizes of test_gpu_batch_kinds.py and a LARGE set of 23 segments cycling through the same sizes
(224 B x 23 > the table buffer's initial 4096 B), carved from one buffer per column: positions 16-byte aligned, class blocks at
byte offsets 0..3 of a dword, time blocks at 0 and 8 modulo 16.  Positions are integers in 0..99, class bytes come from five
values, times are integers in 0..999 with NaN, -0.0 and +inf planted in every segment of at least 511 points.

Expected values are numpy on the host arrays only: pp.in_box and the reference helpers of test_gpu_raster.py (Dev.want),
test_gpu_class_hist.py (Segments.want), test_gpu_time_hist.py (numpy_hist), test_gpu_zrange_raster.py and test_gpu_zsum_raster.py
(Dev.want), _zsum_classes.py (Dev.want) and _polygon_rule.py (counted), called on a plain namespace that holds this module's
arrays; the multi-box rows of test_gpu_batch_multi.py are bound to its seven segments and are restated here.
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
import _polygon_rule as polygon_ref  # noqa: E402
import _zsum_classes as zsum_classes_ref  # noqa: E402
import test_gpu_class_hist as class_hist_ref  # noqa: E402
import test_gpu_raster as raster_ref  # noqa: E402
import test_gpu_time_hist as time_hist_ref  # noqa: E402
import test_gpu_zrange_raster as zrange_ref  # noqa: E402
import test_gpu_zsum_raster as zsum_ref  # noqa: E402

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

KINDS = BOX, CLASS, BOX_CLASS, BOX_TIME, MULTI, CLASS_HIST, TIME_HIST, RASTER, ZRANGE, ZSUM, ZSUM_CLASSES, POLYGON = range(12)
KINDS8 = KINDS[:8]                 # the kinds of the first sequence (ORDER)
NAMES = ("BOX", "CLASS", "BOX_CLASS", "BOX_TIME", "MULTI", "CLASS_HIST", "TIME_HIST", "RASTER", "ZRANGE", "ZSUM", "ZSUM_CLASSES", "POLYGON")
TWO_ARRAYS = (ZRANGE, ZSUM, ZSUM_CLASSES)  # their second array starts at word HALF of the call's region
SIZES = (0, 1, 511, 512, 513, 1535, 4133)
SMALL, LARGE = 0, 1
SET_SIZES = (SIZES, tuple(SIZES[i % 7] for i in range(23)))
VARIED = 6  # the segment (4133 points in both sets) whose predicate changes from one call of a kind to its next

RASTER_CELLS_MAX = 8192            # include/pcq.h: PCQ_RASTER_CELLS_MAX
REGION = RASTER_CELLS_MAX + 64     # u64 words of output per call
HALF = REGION // 2                 # (zrange: 2 x 4096 i32 and 64 more each; zsum: 2 x 2048 u64 and 64 more each)
ZRANGE_CELLS_MAX, ZSUM_CELLS_MAX = 4096, 2048  # include/pcq.h: PCQ_ZRANGE_CELLS_MAX, PCQ_ZSUM_CELLS_MAX
POLYGON_VERTS_MAX = 256            # include/pcq.h: PCQ_POLYGON_VERTS_MAX
NQUERIES = (2, 8, 1, 3, 5, 4, 7, 6)
NBINS = (8, 1024, 1, 5, 1023, 64, 2, 8)
RASTERS = ((8, 8), (64, 128), (1, 1), (3, 5), (128, 64), (1, 37), (91, 90), (8, 8))
ZRANGE_SHAPES = ((64, 64), (1, 1), (3, 5), (1, 37), (4096, 1), (37, 1), (128, 32), (2, 2), (1, 4096))
ZSUM_SHAPES = ((64, 32), (1, 1), (3, 5), (32, 64), (1, 37), (2048, 1), (5, 3), (16, 8), (1, 2048))
CHAIN_SHAPE = (64, 32)             # of the calls that share one raster table byte for byte
DATA_CLASSES = (1, 2, 3, 9, 200)
CLASS_SETS = ((2,), tuple(range(256)), (0, 255), tuple(c for c in range(256) if c not in (1, 2)), (1, 3, 200), (9,),
              tuple(c for c in range(256) if c != 200))
NVERTS = (3, 4, 5, 255, 256, 8, 64)
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

# The second sequence: every ordered pair of the twelve kinds in 145 calls (B(12, 2) with its first symbol again at the end), and
# behind them thirteen calls whose queries test_gpu_batch_all_kinds.py chooses (TAIL): seven over one raster table byte for byte
# (RASTER -> ZRANGE -> ZSUM -> RASTER -> ZSUM -> ZRANGE -> RASTER: after the first of them nothing is uploaded), the class-filtered
# table twice with two class sets, POLYGON -> TIME_HIST -> POLYGON with three trailer sizes, and a polygon call that differs from the
# one before it in one vertex, which changes one edge of the trailer.
TAIL = (RASTER, ZRANGE, ZSUM, RASTER, ZSUM, ZRANGE, RASTER, ZSUM_CLASSES, ZSUM_CLASSES, POLYGON, TIME_HIST, POLYGON, POLYGON)
ORDER12 = tuple(_de_bruijn(12)) + (0,) + TAIL

# pitches of the table layouts (pcq_internal.h: DevSegment, DevCombinedSegment, DevRasterSegment, DevBoundsTimeSegment,
# DevMultiSegment, whose 224 bytes a static_assert holds, DevRasterClassSegment, and DevPolygonSegment with a DevPolygonEdge of 16
# bytes per vertex behind the table), the table buffer's first size and the partials' first size in words
PITCH = {BOX: 48, CLASS: 48, BOX_CLASS: 64, BOX_TIME: 80, MULTI: 224, CLASS_HIST: 64, TIME_HIST: 80, RASTER: 72, ZRANGE: 72, ZSUM: 72,
         ZSUM_CLASSES: 80, POLYGON: 64}
POLYGON_EDGE_BYTES = 16
CLASS_TABLE_BYTES = 256            # raster_classes.h: of a workgroup's LDS, in front of the raster's words
TABLE_BYTES_INITIAL = 4096
PARTIALS_WORDS_MIN = 4096
K1_STEP = pp.K1.step

Query = namedtuple("Query", "kind set visit varied args words want contrib table_bytes slices waves")
# (want: the words a call adds — a raster's counts and behind them its sums for ZSUM and ZSUM_CLASSES — or, for ZRANGE, the
# lowest z per cell and behind them the highest, INT32_MAX / INT32_MIN where no point fell)


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
    """Segment k's box at its v-th shape: wider along x with v until it holds the data's last x, from then on shorter along y"""
    return [10 + k % 7, 5 + 3 * max(v - 11, 0), 0], [60 + k % 7 + 3 * min(v, 11), 90, 99]


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
    first, last = (0.0 if visit % 4 == 3 else 100.0 + visit % 10), 900.0 - visit % 10  # (the inner edges lie in 110 .. 890)
    inner = np.sort(rng.integers(220, 1781, nbins - 1)) / 2.0
    return np.concatenate([[first], inner, [last]])


def cell_widths(boxes, nx, ny):
    """Per segment the smallest widths at which its box fits nx x ny cells, and 0..2 more: they differ between segments"""
    out = []
    for k, (lo, hi) in enumerate(boxes):
        out.append((-(-(hi[0] - lo[0] + 1) // nx) + k % 3, -(-(hi[1] - lo[1] + 1) // ny) + (k + 1) % 3))
    return out


def raster_waves(cells, bytes_per_cell=4, in_front=0):
    """scan_raster.hip, scan_zrange.hip, scan_zsum.hip, scan_zsum_classes.hip: 16 waves per CU, as many as their rasters fit in
    160 KiB of LDS, whole SIMDs beyond four"""
    w = min(16, 160 * 1024 // (in_front + cells * bytes_per_cell))
    return w & ~3 if w > 4 else w


def slab_of(k, v):
    """The z faces of segment k's box where a slab is asked for: they move with the visit, so that a height raster of few cells,
    whose every cell sees the lowest and the highest z of the data, changes with it: from visit 1 on VARIED's slab is the widest"""
    return 36 - k % 7 - v, 64 + k % 7 + v


def outline(k, v, m):
    """Segment k's outline of m vertices at its v-th shape: a horizontal base from vertex 0 to vertex 1 below the middle of the data
    and a jagged arc of m - 2 vertices back over it (any closed sequence of vertices is an outline under the even-odd rule).  The
    base does not travel, so moving vertex 1 along x (`moved`) changes one edge of the trailer, the one from vertex 1 to vertex 2,
    and nothing else."""
    rng = np.random.default_rng([4021, k, v, m])
    base = int(rng.integers(12, 30))
    turn = np.pi * (np.arange(m - 2) + rng.random(m - 2)) / (m - 2)
    radius = rng.integers(25, 45, m - 2)
    arc = np.stack([50 + np.rint(radius * np.cos(turn)), 45 + np.rint(radius * np.sin(turn))], axis=1).astype(np.int64)
    verts = np.concatenate([[[int(rng.integers(15, 25)), base], [int(rng.integers(75, 85)), base]], arc])
    assert len(verts) == m and verts.min() >= 0 and verts.max() <= 99 and (arc[:, 1] > base).all()
    return verts


def travelling_edges(verts):
    """scan_polygon.hip: the edges of the trailer, every edge of the outline that is not horizontal, its lower end first"""
    v = [(int(x), int(y)) for x, y in verts]
    pairs = [(v[j], v[(j + 1) % len(v)]) for j in range(len(v))]
    return [(*p, *q) if p[1] < q[1] else (*q, *p) for p, q in pairs if p[1] != q[1]]


def raster_table(q):
    """The bytes of a launch's table of DevRasterSegment (pcq_internal.h; raster_cells.h: raster_segment_fill; pcq_api.hip:
    pcq_make_dev_pred; raster_div.h: raster_div_magic), a position block's place in its buffer for its address: what the upload
    compares for the density, the height and the mean-height raster alike.  nx and ny are no part of it."""
    import struct
    assert q.kind in (RASTER, ZRANGE, ZSUM)
    sizes = SET_SIZES[SMALL] + SET_SIZES[LARGE]
    poff, _ = pp.carve(sizes, [0] * len(sizes), 12)
    first = len(SET_SIZES[SMALL]) if q.set == LARGE else 0
    preds, cws = q.args[0], q.args[1]
    out, steps = b"", 0
    for k, n in enumerate(SET_SIZES[q.set]):
        lo, hi = [int(v) for v in preds[k].lmin], [int(v) for v in preds[k].lmax]
        assert all(-2**31 <= a <= b < 2**31 for a, b in zip(lo, hi))
        magic = [0xffffffff if w <= 1 else 2**32 // w for w in cws[k]]
        out += struct.pack("<QQQ3i3Iii2I2I", poff[first + k], n, steps, *lo, *[b - a for a, b in zip(lo, hi)], 0, 0, *cws[k], *magic)
        steps += n // K1_STEP
    assert len(out) == q.table_bytes
    return out


@functools.lru_cache(maxsize=None)
def query(kind, s, visit, varied=None, shape=None, slab=None, moved=False):
    """The kind's visit-th call on set s: its arguments, numpy's answer (`words` of them), each segment's share of it.
    Only segment VARIED's predicate depends on the visit (`varied`: that segment at another visit, everything else as it is);
    the launch-level parameters (nqueries, edges, raster and cell widths, class set) cycle by the visit.  The polygon count's
    boxes follow the visit and its outlines, their length included, follow `varied`.  shape: a raster of the caller's instead of
    the visit's; slab: the boxes' z faces from slab_of (the height raster's default) or the whole data (everyone else's); moved:
    vertex 1 of VARIED's outline seven steps further along x."""
    h = host()
    n = len(SET_SIZES[s])
    vv = visit if varied is None else varied
    at = [vv if k == VARIED else 0 for k in range(n)]
    if kind == POLYGON:
        at = [visit if k == VARIED else 0 for k in range(n)]
    boxes = [box_of(k, at[k]) for k in range(n)]
    if (kind == ZRANGE) if slab is None else slab:
        boxes = [([lo[0], lo[1], slab_of(k, at[k])[0]], [hi[0], hi[1], slab_of(k, at[k])[1]]) for k, (lo, hi) in enumerate(boxes)]
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
        assert (np.diff(e) >= 0).all()
        contrib = [int(time_hist_ref.numpy_hist(h.t[s][k][inside[k]], [e[0], e[-1]])[0]) for k in range(n)]
        passing = np.concatenate([h.t[s][k][inside[k]] for k in range(n)])
        args, want = (preds, e), time_hist_ref.numpy_hist(passing, e)
        slices, waves, extra = len(e) - 1, 12, 8 * (len(e) + 1)  # (behind the table: the bin count and the edges)
    elif kind == RASTER:
        nx, ny = RASTERS[visit % 8] if shape is None else shape
        cws = cell_widths(boxes, nx, ny)
        contrib = [int(m.sum()) for m in inside]
        args, want = (preds, cws, nx, ny), raster_ref.Dev.want(h.refs(s), boxes, cws, nx, ny, range(n)).reshape(-1)
        slices, waves = nx * ny, raster_waves(nx * ny)
    elif kind == ZRANGE:
        nx, ny = ZRANGE_SHAPES[visit % len(ZRANGE_SHAPES)] if shape is None else shape
        assert nx * ny <= ZRANGE_CELLS_MAX
        cws = cell_widths(boxes, nx, ny)
        contrib = [int(m.sum()) for m in inside]
        wmin, wmax, _ = zrange_ref.Dev.want(h.refs(s), boxes, cws, nx, ny, range(n), pre=zrange_ref.NOTHING)
        args, want = (preds, cws, nx, ny), np.concatenate([wmin[:nx * ny], wmax[:nx * ny]])
        slices, waves = nx * ny, raster_waves(nx * ny, 8)
    elif kind == ZSUM:
        nx, ny = ZSUM_SHAPES[visit % len(ZSUM_SHAPES)] if shape is None else shape
        assert nx * ny <= ZSUM_CELLS_MAX
        cws = cell_widths(boxes, nx, ny)
        contrib = [int(m.sum()) for m in inside]
        cnt, zsum = zsum_ref.Dev.want(h.refs(s), boxes, cws, nx, ny, range(n), pre=zsum_ref.ZEROS)
        args, want = (preds, cws, nx, ny), np.concatenate([cnt[:nx * ny], zsum[:nx * ny]])
        slices, waves = 2 * nx * ny, raster_waves(nx * ny, 16)
    elif kind == ZSUM_CLASSES:
        nx, ny = ZSUM_SHAPES[visit % len(ZSUM_SHAPES)] if shape is None else shape
        classes = CLASS_SETS[visit % len(CLASS_SETS)]
        cws = cell_widths(boxes, nx, ny)
        contrib = [int((inside[k] & zsum_classes_ref.in_set(h.cls[s][k], classes)).sum()) for k in range(n)]
        refs = SimpleNamespace(ns=SET_SIZES[s], xyz=h.xyz[s], cls=h.cls[s])
        cnt, zsum = zsum_classes_ref.Dev.want(refs, boxes, cws, nx, ny, classes, range(n), pre=zsum_classes_ref.ZEROS)
        args, want = (preds, cws, nx, ny, classes), np.concatenate([cnt[:nx * ny], zsum[:nx * ny]])
        slices, waves = 2 * nx * ny, raster_waves(nx * ny, 16, CLASS_TABLE_BYTES)
    else:
        m = NVERTS[vv % len(NVERTS)]
        assert 3 <= m <= POLYGON_VERTS_MAX
        verts = [outline(k, vv if k == VARIED else 0, m) for k in range(n)]
        if moved:
            verts[VARIED][1, 0] += 7
        contrib = [int(polygon_ref.counted(h.xyz[s][k], *boxes[k], verts[k]).sum()) for k in range(n)]
        args, want = (preds, tuple(tuple((int(x), int(y)) for x, y in v) for v in verts)), [sum(contrib)]
        waves, extra = 16, POLYGON_EDGE_BYTES * n * m  # (behind the table: room for every vertex's edge, whatever the outlines hold)
    want = np.asarray(want, dtype=np.int64)
    pitch = PITCH[BOX] if (kind == MULTI and slices == 1) else PITCH[kind]
    return Query(kind, s, visit, vv, args, len(want), want, contrib, pitch * n + extra, slices, waves)


def check_not_vacuous(q):
    """Every segment of at least 511 points gives more than none and fewer than all of its points to the answer, and VARIED's
    share is another one than at the kind's previous visit (the visit that repeats its predecessor's predicates apart: there
    the moved edge has to move a point)"""
    if q.kind == ZSUM_CLASSES and not set(q.args[4]) & set(DATA_CLASSES):
        # a set that holds no class of the data: the launch runs and adds nothing, where another call's set would have
        assert not q.want.any() and query(ZSUM, q.set, q.visit, q.varied).want.any()
        return
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


def zrange_preset(region):
    """A region of distinct non-zero words with the presets of test_gpu_zrange_raster.py over its two i32 arrays: per word nothing
    yet, a value inside the data's range, one below it, one above it, so that folding both ways is seen"""
    w = region.view(np.int32)
    w[:zrange_ref.WORDS] = zrange_ref.PRE_MIN
    w[2 * HALF:2 * HALF + zrange_ref.WORDS] = zrange_ref.PRE_MAX


def expected(q, pre):
    """The REGION words of a call's region behind the call, from the words `pre` in front of it: the first eight kinds add `want`
    into the first words; the mean-height rasters add their counts there and their sums from word HALF; the height raster folds its
    minima into the i32 words from the start and its maxima into those from word HALF.  Every other word stays."""
    out = pre.copy()
    if q.kind == ZRANGE:
        w, cells = out.view(np.int32), q.words // 2
        w[:cells] = np.minimum(w[:cells], q.want[:cells])
        w[2 * HALF:2 * HALF + cells] = np.maximum(w[2 * HALF:2 * HALF + cells], q.want[cells:])
    elif q.kind in TWO_ARRAYS:
        cells = q.words // 2
        out[:cells] += q.want[:cells].view(np.uint64)
        out[HALF:HALF + cells] += q.want[cells:].view(np.uint64)
    else:
        out[:q.words] += q.want.view(np.uint64)
    return out


class Dev:
    """Both sets on the device of a context of its own, and one output region of REGION words per call, preset to distinct
    non-zero words; calls: their number, or their queries — then the regions of the height raster's calls hold its presets"""

    def __init__(self, ctx, calls):
        queries = None if isinstance(calls, int) else list(calls)
        ncalls = calls if queries is None else len(queries)
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
                              BOX_CLASS: with_class, CLASS_HIST: with_class, BOX_TIME: with_time, TIME_HIST: with_time,
                              ZRANGE: plain, ZSUM: plain, POLYGON: plain, ZSUM_CLASSES: with_class})
            self.class_addr.append([c for p, c, t, n in seg])
        self.preset = (1000 + 7 * np.arange(REGION * ncalls)).astype(np.uint64)
        for call, q in enumerate(queries or ()):
            if q.kind == ZRANGE:
                zrange_preset(self.preset[REGION * call:REGION * (call + 1)])
        ctx.to_device(self.d_out, self.preset)
        self.entry = {BOX: ctx.scan_dev_count_batch, CLASS: ctx.scan_dev_count_batch, BOX_CLASS: ctx.scan_dev_count_batch_combined,
                      BOX_TIME: ctx.scan_dev_count_batch_bounds_time, MULTI: ctx.scan_dev_count_batch_multi,
                      CLASS_HIST: ctx.scan_dev_class_hist_batch, TIME_HIST: ctx.scan_dev_time_hist_batch, RASTER: ctx.scan_dev_raster_batch,
                      ZRANGE: ctx.scan_dev_zrange_raster_batch, ZSUM: ctx.scan_dev_zsum_raster_batch,
                      ZSUM_CLASSES: ctx.scan_dev_zsum_raster_batch_classes, POLYGON: ctx.scan_dev_count_batch_polygon}

    def launch(self, q, call, stream=None):
        """The query into the call's region; stream: a hipStream_t as an integer, or the context's own"""
        at = self.d_out + 8 * REGION * call
        outs = (at, at + 8 * HALF) if q.kind in TWO_ARRAYS else (at,)
        self.entry[q.kind](self.cols[q.set][q.kind], *q.args, *outs, stream=stream)

    def region(self, call):
        out = np.zeros(REGION, dtype=np.uint64)
        self.ctx.to_host(out, self.d_out + 8 * REGION * call)  # (waits for the context's stream)
        return out

    def regions(self):
        out = np.zeros(REGION * self.ncalls, dtype=np.uint64)
        self.ctx.to_host(out, self.d_out)  # (waits for the context's stream)
        return out.reshape(self.ncalls, REGION)

    def before(self, call):
        """The call's region as it was preset"""
        return self.preset[REGION * call:REGION * (call + 1)]

    def wrong(self, words, q, call):
        """None, or what is wrong with the call's region: behind the call it holds what `expected` makes of the preset words —
        numpy's answer added or folded into the kind's words and nothing behind them"""
        want = expected(q, self.before(call))
        bad = np.flatnonzero(words != want)
        if not len(bad):
            return None
        if q.kind == ZRANGE:
            g, w = words.view(np.int32), want.view(np.int32)
            bad = np.flatnonzero(g != w)
            return f"(i32 word, got, want) {[(int(b), int(g[b]), int(w[b])) for b in bad[:8]]} ({len(bad)} words; {q.words // 2} cells)"
        added = words.astype(np.int64) - self.before(call).astype(np.int64)
        asked = want.astype(np.int64) - self.before(call).astype(np.int64)
        cells = q.words // 2
        inside = (bad < q.words) if q.kind not in TWO_ARRAYS else ((bad < cells) | ((bad >= HALF) & (bad < HALF + cells)))
        if inside.any():
            return f"got - want {[(int(b), int(added[b] - asked[b])) for b in bad[inside][:8]]} ({int(inside.sum())} of {q.words} words)"
        return f"words behind the answer changed: {[(int(b), int(added[b])) for b in bad[:8]]}"

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
