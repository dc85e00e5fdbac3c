"""Seeded random cases for eleven batched entries: a segment set, one query per segment and entry, and numpy's answers.

draw(seed) is a pure function of BASE + PCQ_TEST_SEED_BASE + seed (test_gpu_random.py's soak switch).  Nothing here touches a
GPU or the library: test_random_batches_plan.py proves on the CPU that the committed seeds satisfy every precondition of every
entry and reach what they are meant to reach, test_gpu_random_batches.py runs them.

What is drawn jointly, per case (include/pcq.h names what every entry accepts; only that is drawn):
  segments   1 .. 24; n from N_LIST (a wave, the three loads of a 256-point tile, a K1 step of 512, the class batch's 4096 bytes)
             or uniform in 1 .. 4500, at most about CAP points a case; positions pieces 16-byte aligned, class pieces at a random
             byte phase 0 .. 15, time pieces at phase 0 or 8, carved from one buffer per column (_pipeline_plan.carve)
  positions  per segment one of: "small" 0 .. 99; "near" a few thousand steps around an origin anywhere in the i32 range; "wide" the
             whole i32 range with INT32_MIN / INT32_MAX planted on some axes; "sites" all points on 1 .. 4 lattice sites
  classes    all 256 values, or 2 .. 5 of them
  times      integers, and planted: NaN, both infinities, both zeros, a denormal, and the doubles below, on and above the segment's
             range bounds and the launch's histogram edges
  boxes      around one of the segment's own points, half widths from HALF per axis; a minority empty (lmin > lmax), outside the
             i32 range, or open on one side far beyond it.  Every entry draws its own.
  per entry  a class; a time range (empty, reversed, NaN and infinite ones among them); 1 .. 8 boxes (rows without a live box
             among them); 1 .. 1024 bins with equal neighbours, infinities and -0.0 among the edges; rasters up to the entries'
             limits with cell widths from CELL_WIDTHS or any u32, the box cut to the raster; outlines of 3 .. 12 vertices (256 in
             some cases) in and around the box: on data points, with horizontal and vertical edges, in random order (so they
             intersect themselves), the hull of box and outline at most 2^31 - 1 wide.

Answers restate include/pcq.h on int64 / f64 host arrays: inclusive integer compares for boxes, IEEE compares for ranges and bins
(bin = #{edges <= t} - 1), floor division on int64 for cells, np.minimum.at / np.maximum.at for the height raster, np.add.at of 1
and of z on int64 for the mean-height raster (no sum of CAP i32 values leaves the i64 range), and
_polygon_rule.inside_exact (Python integers) for the outlines: for every boxed point where that takes at most EXACT_BUDGET
edge tests per segment, else _polygon_rule.inside (the same rule in int64, exact inside the entry's bound: every product is below
2^62) with inside_exact on a sample of EXACT_SAMPLE of them.  Every answer is kept per segment ([S, words]): a launch's answer is the sum
(height raster: the fold) over the segments.

The mean-height raster ("zsum") came after the other ten had committed seeds: everything it draws comes from a generator of its
own, seeded from (BASE + PCQ_TEST_SEED_BASE + seed, ZSUM_TAG), behind everything else, so that the ten draw what they always drew
(test_random_batches_plan.py pins a digest of that).
"""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402
import _polygon_rule as rule  # noqa: E402

BASE = 52000
SEED_BASE = int(os.environ.get("PCQ_TEST_SEED_BASE", "0"))  # a soak run: other seeds than the committed ones
SEEDS = range(48)

FIRST_TEN = ("box", "class", "box_class", "box_time", "multi", "class_hist", "time_hist", "raster", "zrange", "polygon")
ENTRIES = FIRST_TEN + ("zsum",)
COUNTS_WITH_STEPS = ("box", "box_class", "box_time", "multi", "polygon", "zsum")
ZSUM_TAG = 0x7a73756d  # ("zsum") the second word of the seed of the entry's own generator
N_LIST = (0, 1, 2, 63, 64, 65, 85, 86, 170, 171, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535)
N_UNIFORM_MAX = 4500
S_MAX = 24
CAP = 40000
K1_STEP = pp.K1.step
DISTS = ("small", "near", "wide", "sites")
HALF = (0, 1, 7, 1000, 2**31, 2**40)
HALF_P = (0.08, 0.10, 0.17, 0.25, 0.25, 0.15)
CELL_WIDTHS = (1, 2, 3, 7, 641, 2**24)
I32_MIN, I32_MAX = -2**31, 2**31 - 1
SPAN_MAX = 2**31 - 1          # include/pcq.h: the polygon entry's exactness bound
MULTI_BOX_MAX, CLASS_BINS, TIME_BINS_MAX, RASTER_CELLS_MAX, ZRANGE_CELLS_MAX, POLYGON_VERTS_MAX = 8, 256, 1024, 8192, 4096, 256
ZSUM_CELLS_MAX = 2048
EXACT_BUDGET, EXACT_SAMPLE = 40000, 96
RASTER_SHAPES = ((1, 1), (8, 8), (3, 5), (1, 37), (64, 64), (91, 45), (4096, 1), (1, 4096), (2, 2048))
ZSUM_SHAPES = ((2048, 1), (1, 2048), (64, 32), (3, 5), (1, 1), (8, 8), (1, 37))


# ---------------------------------------------------------------------------------------------------------------------------------
# the rules of include/pcq.h
# ---------------------------------------------------------------------------------------------------------------------------------
def box_is_empty(lo, hi):
    """lmin > lmax on an axis, or a box outside the i32 value range"""
    return any(max(int(a), I32_MIN) > min(int(b), I32_MAX) for a, b in zip(lo, hi))


def bins_of(t, edges):
    """#{i : e[i] <= t} - 1 per time, IEEE compares (NaN: -1)"""
    with np.errstate(invalid="ignore"):
        return (edges[None, :] <= t[:, None]).sum(axis=1) - 1


def in_range(t, t0, t1):
    with np.errstate(invalid="ignore"):
        return pp.in_range(t, t0, t1)


def cells_of(p, sel, lo, cw, nx, ny):
    cx = (p[sel, 0] - int(lo[0])) // int(cw[0])
    cy = (p[sel, 1] - int(lo[1])) // int(cw[1])
    assert cx.min(initial=0) >= 0 and cx.max(initial=0) < nx and cy.min(initial=0) >= 0 and cy.max(initial=0) < ny
    return cy * nx + cx


def inside_outline(p, sel, verts, rng):
    """Of the points p[sel]: inside the outline"""
    idx = np.flatnonzero(sel)
    out = np.zeros(len(idx), dtype=bool)
    if len(idx) * len(verts) <= EXACT_BUDGET:
        for j, i in enumerate(idx):
            out[j] = rule.inside_exact(p[i, 0], p[i, 1], verts)
        return out
    out = rule.inside(p[idx, 0], p[idx, 1], verts)
    for j in rng.choice(len(idx), EXACT_SAMPLE, replace=False):
        assert out[j] == rule.inside_exact(p[idx[j], 0], p[idx[j], 1], verts)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------------------------------------------------------------
def draw_sizes(rng):
    S = int(rng.integers(1, S_MAX + 1))
    n = [int(rng.integers(1, N_UNIFORM_MAX + 1)) if rng.random() < 0.3 else int(rng.choice(N_LIST)) for _ in range(S)]
    while sum(n) > CAP:
        n[int(np.argmax(n))] = int(rng.choice(N_LIST))
    return n


def anywhere(rng, size=None):
    return rng.integers(I32_MIN, I32_MAX + 1, size=size, dtype=np.int64)


def draw_positions(rng, n, dist):
    if dist == "small":
        p = rng.integers(0, 100, (n, 3))
    elif dist == "near":
        p = np.clip(anywhere(rng, 3)[None, :] + rng.integers(-3000, 3001, (n, 3)), I32_MIN, I32_MAX)
    elif dist == "wide":
        p = anywhere(rng, (n, 3))
        for a in range(3):
            for v in (I32_MIN, I32_MAX):
                if n and rng.random() < 0.6:
                    p[rng.integers(0, n), a] = v
    else:
        k = int(rng.integers(1, 5))
        sites = np.concatenate([draw_positions(rng, 1, DISTS[int(rng.integers(0, 3))]) for _ in range(k)])
        p = sites[rng.integers(0, k, n)]
    return p.astype(np.int32).reshape(n, 3)


def draw_box(rng, p, at=None):
    """A box around one of the points p (int64 [n][3]): point `at`, or any"""
    c = [int(v) for v in (p[rng.integers(0, len(p)) if at is None else at] if len(p) else anywhere(rng, 3))]
    hw = [int(rng.choice(HALF, p=HALF_P)) for _ in range(3)]
    lo, hi = [c[a] - hw[a] for a in range(3)], [c[a] + hw[a] for a in range(3)]
    u, a = rng.random(), int(rng.integers(0, 3))
    if u < 0.07:    # empty
        lo[a], hi[a] = c[a] + 1 + int(rng.integers(0, 5)), c[a]
    elif u < 0.12:  # outside the i32 range
        lo[a], hi[a] = (2**31, 2**31 + 2**35) if rng.random() < 0.5 else (-2**40, I32_MIN - 1)
    elif u < 0.24:  # open on one side
        if rng.random() < 0.5:
            lo[a] = -2**45
        else:
            hi[a] = 2**45
    return lo, hi


def draw_times(rng, n, bounds):
    t = rng.integers(0, 1000, n).astype(np.float64)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324]
    for b in bounds:
        if np.isfinite(b):
            special += [np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf)]
    pick = rng.random(n) < 0.2
    t[pick] = rng.choice(np.asarray(special), int(pick.sum()))
    return t


def draw_range(rng, t=None):
    """A range; t: a time to draw it around (the time of the point its box is drawn around)"""
    a, b = sorted(float(v) / 2 for v in rng.integers(0, 2000, 2))
    u = rng.random()
    if t is not None and np.isfinite(t) and u > 0.6:  # t on the start, or the last double below the end, or inside
        v = rng.random()
        return (t, t + b / 8 + 0.5) if v < 0.3 else (t - a / 8 - 0.5, np.nextafter(t, np.inf)) if v < 0.6 else (t - a / 8, t + b / 8 + 0.5)
    if u < 0.06:
        return a, a
    if u < 0.12:
        return b + 1.0, a
    if u < 0.17:
        return (np.nan, b) if rng.random() < 0.5 else (a, np.nan)
    if u < 0.25:
        return -np.inf, np.inf
    return a, b + 0.5


def draw_edges(rng):
    nbins = int(rng.choice([1, 2, 3, 7, 64, 1023, 1024, int(rng.integers(1, TIME_BINS_MAX + 1))]))
    e = np.sort(rng.integers(0, 2000, nbins + 1)).astype(np.float64) / 2  # (half numbers; equal neighbours from a hundred edges on)
    if rng.random() < 0.3:
        e[0] = -np.inf
    elif rng.random() < 0.4:
        e[0] = -0.0
    if rng.random() < 0.3:
        e[-1] = np.inf
    return e


def draw_raster_shape(rng, cells_max):
    while True:
        if rng.random() < 0.7:
            nx, ny = RASTER_SHAPES[int(rng.integers(0, len(RASTER_SHAPES)))]
            if rng.random() < 0.5:
                nx, ny = ny, nx
        else:
            nx = int(rng.integers(1, 200))
            ny = int(rng.integers(1, max(2, min(200, cells_max // nx + 1))))
        if cells_max == RASTER_CELLS_MAX and rng.random() < 0.3:
            nx *= 2
        if nx * ny <= cells_max:
            return nx, ny


def draw_raster_box(rng, p, dims):
    """(lo, hi, cell widths): the origin inside the i32 range, the box cut to dims cells on x and y"""
    cw = [int(rng.choice(CELL_WIDTHS)) if rng.random() < 0.8 else int(rng.integers(1, 2**32)) for _ in range(2)]
    lo, hi = draw_box(rng, p)
    if rng.random() < 0.6:  # the raster laid over the box's centre point, the box its whole extent
        c = [int(v) for v in (p[rng.integers(0, len(p))] if len(p) else anywhere(rng, 3))]
        for a in range(2):
            lo[a] = c[a] - int(rng.integers(0, dims[a] * cw[a]))
            hi[a] = 2**40
    for a in range(2):
        lo[a] = min(max(lo[a], I32_MIN), I32_MAX)
        hi[a] = min(hi[a], lo[a] + dims[a] * cw[a] - 1 - int(rng.choice([0, 0, 1, cw[a] // 2])))
    return lo, hi, cw


def draw_outline(rng, p, nverts):
    """(lo, hi, vertices): the hull of the box's x and y ranges (clamped to i32) and the vertices spans at most SPAN_MAX"""
    lo, hi = draw_box(rng, p)
    if box_is_empty(lo, hi):  # (its vertices are not examined)
        return lo, hi, [[int(v) for v in anywhere(rng, 2)] for _ in range(nverts)]
    region = []
    for a in range(2):
        b0, b1 = max(lo[a], I32_MIN), min(hi[a], I32_MAX)
        if b1 - b0 > SPAN_MAX:  # cut the box, around the data where there is any
            mid = int(p[rng.integers(0, len(p)), a]) if len(p) else 0
            b0 = min(max(mid - SPAN_MAX // 2, I32_MIN), I32_MAX - SPAN_MAX)
            b1 = b0 + SPAN_MAX
            lo[a], hi[a] = b0, b1
        room = SPAN_MAX - (b1 - b0)
        grow = min(room // 2, (b1 - b0) // 2 + 8)
        region.append((max(I32_MIN, b0 - int(rng.integers(0, grow + 1))), min(I32_MAX, b1 + int(rng.integers(0, grow + 1)))))
    near = np.flatnonzero((p[:, 0] >= region[0][0]) & (p[:, 0] <= region[0][1]) & (p[:, 1] >= region[1][0]) & (p[:, 1] <= region[1][1]))
    verts = []
    if rng.random() < 0.4:  # the region's corners in order first: a rectangle, which the later vertices fold over itself
        (x0, x1), (y0, y1) = region
        verts = [[x0, y0], [x1, y0], [x1, y1], [x0, y1]][:nverts]
    for j in range(len(verts), nverts):
        u = rng.random()
        if u < 0.3 and len(near):
            v = [int(p[near[rng.integers(0, len(near))], a]) for a in range(2)]
        else:
            v = [int(rng.integers(region[a][0], region[a][1] + 1)) for a in range(2)]
            if u > 0.8 and verts:  # a vertical or a horizontal edge
                a = int(rng.integers(0, 2))
                v[a] = verts[-1][a]
        verts.append(v)
    return lo, hi, verts


# ---------------------------------------------------------------------------------------------------------------------------------
# a case
# ---------------------------------------------------------------------------------------------------------------------------------
def draw(seed):
    rng = np.random.default_rng(BASE + SEED_BASE + seed)
    c = SimpleNamespace(seed=seed)
    n = c.n = draw_sizes(rng)
    S = c.S = len(n)
    c.cphase = [int(v) for v in rng.integers(0, 16, S)]
    c.tphase = [8 * int(v) for v in rng.integers(0, 2, S)]
    c.poff, c.psize = pp.carve(n, [0] * S, 12)
    c.coff, c.csize = pp.carve(n, c.cphase)
    c.toff, c.tsize = pp.carve(n, c.tphase, 8)
    c.dist = [DISTS[int(rng.integers(0, 4))] for _ in range(S)]
    c.xyz = [draw_positions(rng, n[k], c.dist[k]) for k in range(S)]
    P = [x.astype(np.int64) for x in c.xyz]
    c.class_values, c.cls = [], []
    for k in range(S):
        vals = np.arange(256) if rng.random() < 0.5 else rng.choice(256, int(rng.integers(2, 6)), replace=False)
        c.class_values.append(vals.astype(np.uint8))
        c.cls.append(rng.choice(c.class_values[k], n[k]))
    # the launch-level parameters
    c.edges = draw_edges(rng)
    c.nq = int(rng.integers(1, MULTI_BOX_MAX + 1))
    c.raster_dims = draw_raster_shape(rng, RASTER_CELLS_MAX)
    c.zrange_dims = draw_raster_shape(rng, ZRANGE_CELLS_MAX)
    c.nverts = POLYGON_VERTS_MAX if rng.random() < 0.1 else int(rng.integers(3, 13))
    # per segment
    interior = c.edges[rng.integers(0, len(c.edges), 3)]
    bounds = [float(v) / 2 for v in rng.integers(0, 2000, 2)]  # (where ranges start and end, before a segment has its own)
    c.t = [draw_times(rng, n[k], [*bounds, c.edges[0], c.edges[-1], *interior]) for k in range(S)]
    centre = [int(rng.integers(0, max(n[k], 1))) for k in range(S)]  # the point that box AND class / time are drawn around
    c.ranges = [draw_range(rng, c.t[k][centre[k]] if n[k] else None) for k in range(S)]
    for k in range(S):  # the doubles next to this segment's bounds, on points of its own
        near = [w for b in c.ranges[k] if np.isfinite(b) for w in (np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf))]
        if near and n[k]:
            pick = np.flatnonzero((rng.random(n[k]) < 0.1) & (np.arange(n[k]) != centre[k]))
            c.t[k][pick] = rng.choice(np.asarray(near), len(pick))
    c.qclass = [int(c.cls[k][centre[k]]) if n[k] and rng.random() < 0.85 else int(rng.integers(0, 256)) for k in range(S)]
    c.cclass = [int(rng.choice(c.class_values[k])) if rng.random() < 0.85 else int(rng.integers(0, 256)) for k in range(S)]
    c.box = {e: [draw_box(rng, P[k], centre[k] if e in ("box_class", "box_time") else None) for k in range(S)]
             for e in ("box", "box_class", "box_time", "class_hist", "time_hist")}
    c.multi = []
    for k in range(S):
        row = [draw_box(rng, P[k]) for _ in range(c.nq)]
        if rng.random() < 0.15:  # a row without a live box
            row = [([5, 5, 5], [4, 4, 4 + q]) for q in range(c.nq)]
        c.multi.append(row)
    c.raster = [draw_raster_box(rng, P[k], c.raster_dims) for k in range(S)]
    c.zrange = [draw_raster_box(rng, P[k], c.zrange_dims) for k in range(S)]
    c.polygon = [draw_outline(rng, P[k], c.nverts) for k in range(S)]
    answers(c, P, rng)
    draw_zsum(c, P, np.random.default_rng([BASE + SEED_BASE + seed, ZSUM_TAG]))
    return c


def draw_zsum(c, P, rng):
    """The mean-height raster's shape, boxes, cell widths and answers, from a generator of its own: c.zsum_dims, c.zsum, and
    c.share["zsum"] = (counts, z sums), each [S, cells] int64; c.mask["zsum"][k]: the counted points of segment k"""
    if rng.random() < 0.75:
        nx, ny = ZSUM_SHAPES[int(rng.integers(0, len(ZSUM_SHAPES)))]
    else:
        nx = int(rng.integers(1, 200))
        ny = int(rng.integers(1, max(2, min(200, ZSUM_CELLS_MAX // nx + 1))))
    assert nx * ny <= ZSUM_CELLS_MAX
    c.zsum_dims = (nx, ny)
    c.zsum = [draw_raster_box(rng, P[k], c.zsum_dims) for k in range(c.S)]
    cnt, zsum = np.zeros((c.S, nx * ny), dtype=np.int64), np.zeros((c.S, nx * ny), dtype=np.int64)
    c.mask["zsum"] = []
    for k in range(c.S):
        lo, hi, cw = c.zsum[k]
        sel = pp.in_box(P[k], lo, hi)
        cell = cells_of(P[k], sel, lo, cw, nx, ny)
        np.add.at(cnt[k], cell, 1)
        np.add.at(zsum[k], cell, P[k][sel, 2])
        c.mask["zsum"].append(sel)
    c.share["zsum"] = (cnt, zsum)


def words_of(c, entry):
    if entry == "zsum":
        return c.zsum_dims[0] * c.zsum_dims[1]
    return {"multi": c.nq, "class_hist": CLASS_BINS, "time_hist": len(c.edges) - 1, "raster": c.raster_dims[0] * c.raster_dims[1],
            "zrange": c.zrange_dims[0] * c.zrange_dims[1]}.get(entry, 1)


def boxes_of(c, entry, k):
    """The boxes of segment k under the entry (the class batch: none)"""
    if entry == "class":
        return []
    if entry == "multi":
        return c.multi[k]
    if entry in ("raster", "zrange", "polygon", "zsum"):
        return [getattr(c, entry)[k][:2]]
    return [c.box[entry][k]]


def answers(c, P, rng):
    """c.share[entry]: [S, words] int64, what each segment adds to each word (zrange: the pair of per-segment minima and maxima,
    INT32_MAX and INT32_MIN where a segment has no point in a cell); c.mask[entry][k]: the counted points of segment k (multi: of
    any box), for the entries of COUNTS_WITH_STEPS; c.passing: the boxed points of the box entry"""
    S = c.S
    c.share = {e: np.zeros((S, words_of(c, e)), dtype=np.int64) for e in FIRST_TEN if e != "zrange"}
    cells = words_of(c, "zrange")
    zmin, zmax = np.full((S, cells), I32_MAX, dtype=np.int64), np.full((S, cells), I32_MIN, dtype=np.int64)
    c.mask = {e: [] for e in COUNTS_WITH_STEPS if e in FIRST_TEN}
    c.passing = []
    nbins = len(c.edges) - 1
    for k in range(S):
        p, cl, t = P[k], c.cls[k], c.t[k]
        sel = pp.in_box(p, *c.box["box"][k])
        c.share["box"][k, 0] = sel.sum()
        c.mask["box"].append(sel)
        c.passing.append(p[sel])
        c.share["class"][k, 0] = (cl == c.cclass[k]).sum()
        sel = pp.in_box(p, *c.box["box_class"][k]) & (cl == c.qclass[k])
        c.share["box_class"][k, 0] = sel.sum()
        c.mask["box_class"].append(sel)
        sel = pp.in_box(p, *c.box["box_time"][k]) & in_range(t, *c.ranges[k])
        c.share["box_time"][k, 0] = sel.sum()
        c.mask["box_time"].append(sel)
        anyq = np.zeros(len(p), dtype=bool)
        for q, (lo, hi) in enumerate(c.multi[k]):
            sel = pp.in_box(p, lo, hi)
            c.share["multi"][k, q] = sel.sum()
            anyq |= sel
        c.mask["multi"].append(anyq)
        sel = pp.in_box(p, *c.box["class_hist"][k])
        c.share["class_hist"][k] = np.bincount(cl[sel], minlength=CLASS_BINS)
        sel = pp.in_box(p, *c.box["time_hist"][k])
        b = bins_of(t[sel], c.edges)
        c.share["time_hist"][k] = np.bincount(b[(b >= 0) & (b < nbins)], minlength=nbins)
        lo, hi, cw = c.raster[k]
        sel = pp.in_box(p, lo, hi)
        c.share["raster"][k] = np.bincount(cells_of(p, sel, lo, cw, *c.raster_dims), minlength=words_of(c, "raster"))
        lo, hi, cw = c.zrange[k]
        sel = pp.in_box(p, lo, hi)
        cell = cells_of(p, sel, lo, cw, *c.zrange_dims)
        np.minimum.at(zmin[k], cell, p[sel, 2])
        np.maximum.at(zmax[k], cell, p[sel, 2])
        lo, hi, verts = c.polygon[k]
        sel = pp.in_box(p, lo, hi)
        sel[sel] = inside_outline(p, sel, verts, rng)
        c.share["polygon"][k, 0] = sel.sum()
        c.mask["polygon"].append(sel)
    c.share["zrange"] = (zmin, zmax)


def answer(c, entry):
    if entry == "zrange":
        zmin, zmax = c.share[entry]
        return zmin.min(axis=0), zmax.max(axis=0)
    if entry == "zsum":
        cnt, zsum = c.share[entry]
        return cnt.sum(axis=0), zsum.sum(axis=0)
    return c.share[entry].sum(axis=0)


def live(c, entry):
    """Per segment: it gives something to the answer"""
    if entry == "zrange":
        return (c.share[entry][0] != I32_MAX).any(axis=1)
    if entry == "zsum":
        return c.share[entry][0].any(axis=1)
    return c.share[entry].any(axis=1)


def dead(c, entry):
    """Per segment: points under a predicate that is empty, which the kernels skip (multi: no live box in the row; the class batch,
    whose predicates are never empty: no points)"""
    if entry == "class":
        return np.asarray([n == 0 for n in c.n])
    return np.asarray([c.n[k] > 0 and all(box_is_empty(lo, hi) for lo, hi in boxes_of(c, entry, k)) for k in range(c.S)])


@functools.lru_cache(maxsize=4)
def case(seed):
    return draw(seed)
