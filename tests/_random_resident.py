"""Seeded random cases for the count queries over a dataset resident in HBM (include/pcq_query.h): 2 .. 6 LAST files with GPS
times, one world-space query per entry drawn around the files' own world points, and numpy's answer on the stored integers.

draw(seed) is a pure function of BASE + PCQ_TEST_SEED_BASE + seed.  test_random_batches_plan.py proves the committed seeds on the
CPU (no refused call, answers worth asking for, a lying header that decides an answer); test_gpu_random_resident.py runs them.

Files      formats with GPS time; n from _random_batches.N_LIST (0 among them) or uniform in 1 .. 4500; scales from SCALES — one
           value for all three axes in about half the files, else drawn per axis — and offsets from OFFSETS per axis; stored
           integers within +-50, +-5000 or +-200000 per axis, or all on a few sites; in about one file in five the header bounds
           are tighter than the points, so that the header early-out (inclusive, on the HEADER's box) is observable.
Queries    a world box around a world point of some file (in a lying file: preferably one its header hides) with half widths from
           HALF_WORLD per axis.  The reference's conversion (pcq_box_to_local, bug for bug: every min component divides by
           scale[0]) fails with PCQ_ERR_PANIC where it turns a box inside out in a file's lattice, which a small box in a file
           of unequal scales often does: refusal() restates every rule by which an entry refuses a call, and a draw is repeated
           until it names none, so every call of the GPU test has to return 0.  Rasters: more cells than one launch holds, in
           some seeds rows longer than a launch (so a row is cut into pieces), cell sizes that are whole multiples of every
           file's x and y step under the product's own rule |c / s - k| <= 1e-9 k.  Outlines: 3 .. 12 vertices (256 in some
           seeds) whose rounded hull fits every surviving file's lattice.
Answers    per file whose header meets the query's world box: pkg.box_to_local (pinned to the oracle by test_abi_and_host.py),
           inclusive integer compares, IEEE compares on the times, floor division for cells, numpy.rint((w - offset) / scale) for
           vertices and _polygon_rule for the outline, (Z * scale) + offset in two roundings for world z, NaN for a cell no
           point reaches, points_scanned the points of the files whose headers meet the box.

The mean-height rasters ("zmean", "zmean_classes": include/pcq_query_stats.h, pcq_query_classes.h) came after the other ten had
committed seeds: each draws its query from a generator of its own, seeded from (BASE + PCQ_TEST_SEED_BASE + seed, its tag), so
that the ten draw what they always drew (test_random_batches_plan.py pins a digest of that).  Their rasters have more cells than
PCQ_ZSUM_CELLS_MAX, so every call is cut into blocks; the class sets are one class the files hold, a few, all 256 and the empty
set.  The answer restates the rule written above ResidentDataset::zmean_raster in Python floats: the surviving files grouped by
the bits of (scale_z, offset_z) in the order of each group's first file; per group and cell a = offset * float(cnt), b = scale *
float(sum), W += a + b, N += cnt; then W / N, or NaN where N == 0.
"""
import functools
import importlib
import os
import struct
import sys
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402
import _polygon_rule as rule  # noqa: E402
import _time_images as ti  # noqa: E402
from _random_batches import I32_MAX, I32_MIN, N_LIST, N_UNIFORM_MAX, SEED_BASE, draw_edges, in_range  # noqa: E402

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

BASE = 64000
SEEDS = range(24)
FIRST_TEN = ("bounds", "class", "bounds_class", "bounds_time", "many", "by_class", "by_time", "raster", "zrange", "polygon")
ENTRIES = FIRST_TEN + ("zmean", "zmean_classes")
RASTER_ENTRIES = ("raster", "zrange", "zmean", "zmean_classes")
Z_LATTICE_ENTRIES = ("zrange", "zmean", "zmean_classes")  # raster_segments with z_lattice = true
TAGS = {"zmean": 0x7a6d, "zmean_classes": 0x7a6d63}     # ("zm", "zmc") the second word of the seed of the entry's own generator
BOX_ENTRIES = ("bounds", "bounds_class", "bounds_time", "by_class", "by_time")
TIME_FORMATS = (1, 3, 4, 5, 6, 7, 8, 9, 10)
SCALES = (0.001, 0.01, 0.1, 0.25, 0.5, 1.0)
OFFSETS = (0.0, 100.0, -2500.5, 389400.0, 1e6)
RANGES = (50, 5000, 200000)
HALF_WORLD = (0.0, 0.5, 5.0, 100.0, 1e4, 1e7)
HALF_WORLD_P = (0.06, 0.1, 0.14, 0.25, 0.25, 0.2)
HALF_Z = (100.0, 1e4, 1e7)
CELL_SIZES = (0.5, 1.0, 2.0, 2.5, 5.0, 10.0, 50.0, 250.0)
MULTI_BOX_MAX, RASTER_CELLS_MAX, ZRANGE_CELLS_MAX, POLYGON_VERTS_MAX = 8, 8192, 4096, 256
ZSUM_CELLS_MAX = 2048
QUERY_RASTER_CELLS_MAX = 1 << 20
RASTER_SHAPES = ((100, 120), (300, 40), (10, 2000), (91, 91), (9000, 2), (16385, 1), (1, 9000))   # all above RASTER_CELLS_MAX
ZRANGE_SHAPES = ((80, 80), (10, 2000), (65, 64), (5000, 2), (4097, 1), (1, 5000), (8193, 3))      # all above ZRANGE_CELLS_MAX
ZMEAN_CELL_SIZES = (250.0, 10000.0, 100000.0, 1000000.0)  # of the rasters laid over several files: in the coarse ones files of several z lattices share cells
ZMEAN_SHAPES = ((2049, 3), (1, 5000), (5000, 2), (70, 70), (46, 45), (10, 2000), (4097, 1), (33, 63))  # all above ZSUM_CELLS_MAX
TRIES = 60


# ---------------------------------------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------------------------------------
def draw_file(rng, edges, bounds):
    f = SimpleNamespace()
    f.fmt = int(rng.choice(TIME_FORMATS))
    n = f.n = int(rng.integers(1, N_UNIFORM_MAX + 1)) if rng.random() < 0.3 else int(rng.choice(N_LIST))
    f.scale = tuple([float(rng.choice(SCALES))] * 3) if rng.random() < 0.5 else tuple(float(v) for v in rng.choice(SCALES, 3))
    f.offset = tuple(float(v) for v in rng.choice(OFFSETS, 3))
    r = [int(rng.choice(RANGES)) for _ in range(2)] + [1000]
    xyz = np.stack([rng.integers(-r[a], r[a] + 1, n) for a in range(3)], axis=1)
    if n and rng.random() < 0.2:  # all on a few sites
        xyz = xyz[rng.integers(0, min(n, 4), n)]
    f.xyz = xyz.astype(np.int32).reshape(n, 3)
    vals = np.arange(256) if rng.random() < 0.5 else rng.choice(256, int(rng.integers(2, 6)), replace=False)
    f.cls = rng.choice(vals.astype(np.uint8), n)
    t = rng.integers(0, 1000, n).astype(np.float64)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324]
    for b in (*bounds, edges[0], edges[-1], *edges[rng.integers(0, len(edges), 3)]):
        if np.isfinite(b):
            special += [np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf)]
    pick = rng.random(n) < 0.2
    t[pick] = rng.choice(np.asarray(special), int(pick.sum()))
    f.t = t
    f.world = ti.world(f.xyz, f.scale, f.offset)
    w = f.world if n else np.zeros((1, 3))
    f.hmin, f.hmax = w.min(axis=0), w.max(axis=0)
    f.hidden = np.zeros(n, dtype=bool)
    f.lying = bool(n >= 2 and rng.random() < 0.22)
    if f.lying:  # the header ends at the median of one axis: the points beyond it are hidden from it
        a = int(rng.integers(0, 3))
        mid = float(np.median(f.world[:, a]))
        if rng.random() < 0.5:
            f.hmax[a] = mid
            f.hidden = f.world[:, a] > mid
        else:
            f.hmin[a] = mid
            f.hidden = f.world[:, a] < mid
        f.lying = bool(f.hidden.any())
    return f


def image(f):
    """The LAST image of a file, its header's bounds those of f.hmin / f.hmax"""
    img = ti.last_image(f.fmt, f.xyz, f.cls, np.zeros((f.n, 3), dtype=np.uint16), f.t, scale=f.scale, offset=f.offset).copy()
    for a in range(3):
        img[179 + 16 * a:195 + 16 * a] = np.frombuffer(struct.pack("<2d", f.hmax[a], f.hmin[a]), dtype=np.uint8)
    return img


# ---------------------------------------------------------------------------------------------------------------------------------
# the host layer's rules (host/resident.cpp, include/pcq_query.h)
# ---------------------------------------------------------------------------------------------------------------------------------
def meets(f, bmin, bmax):
    """The header early-out: the header's box meets the query's, inclusive"""
    return bool(np.all(f.hmin <= np.asarray(bmax)) and np.all(f.hmax >= np.asarray(bmin)))


def survivors(files, bmin, bmax, header=True):
    """(file, lmin, lmax) of the files that are scanned: the header meets the box, the box converts, the file has points.
    Raises pkg.PcqError (PCQ_ERR_PANIC) where the product's call fails: a file whose header meets the box and in whose lattice
    the box comes out with min > max, points or no points."""
    out = []
    for f in files:
        if header and not meets(f, bmin, bmax):
            continue
        lmin, lmax = pkg.box_to_local(list(bmin), list(bmax), list(f.scale), list(f.offset))
        if f.n:
            out.append((f, lmin, lmax))
    return out


def raster_world_box(q):
    return tuple(q.bmin), (q.bmin[0] + float(q.nx) * q.cell, q.bmin[1] + float(q.ny) * q.cell, q.zmax)


def polygon_world_box(q):
    v = np.asarray(q.xy, dtype=np.float64)
    return (float(v[:, 0].min()), float(v[:, 1].min()), q.zmin), (float(v[:, 0].max()), float(v[:, 1].max()), q.zmax)


def steps_of(cell, scale):
    """The cell in lattice steps, or None: k = nearbyint(c / s) in 1 .. 2^32 - 1 with |c / s - k| <= 1e-9 k"""
    cw = cell / scale
    k = np.rint(cw)
    return int(k) if 1.0 <= k <= 4294967295.0 and abs(cw - k) <= 1e-9 * k else None


def lattice(xy, f):
    """numpy.rint((w - offset) / scale): two f64 operations in this order, ties to even"""
    v = np.asarray(xy, dtype=np.float64)
    return np.stack([np.rint((v[:, a] - np.float64(f.offset[a])) / np.float64(f.scale[a])) for a in range(2)], axis=1)


def refusal(files, entry, q):
    """None, or why the product refuses the query"""
    if entry == "class":
        return None
    boxes = (list(zip(q.bmin, q.bmax)) if entry == "many" else [raster_world_box(q)] if entry in RASTER_ENTRIES
             else [polygon_world_box(q)] if entry == "polygon" else [(q.bmin, q.bmax)])
    alive = []
    for bmin, bmax in boxes:
        if not all(np.isfinite(v) for v in (*bmin, *bmax)) or any(a > b for a, b in zip(bmin, bmax)):
            return "min > max in world space"
        try:
            alive = survivors(files, bmin, bmax)
        except pkg.PcqError as e:
            return f"a surviving file's box: {e}"
    if entry in RASTER_ENTRIES:
        if not 0 < q.nx * q.ny <= QUERY_RASTER_CELLS_MAX or not (np.isfinite(q.cell) and q.cell > 0):
            return "raster shape"
        for f, lmin, lmax in alive:
            if any(steps_of(q.cell, f.scale[a]) is None for a in range(2)):
                return "the cell is no whole number of lattice steps"
            if not all(I32_MIN <= lmin[a] <= I32_MAX for a in range(2)):
                return "the origin lies outside a file's lattice"
            if entry in Z_LATTICE_ENTRIES and not (np.isfinite(f.scale[2]) and f.scale[2] > 0):
                return "the z scale is not finite and above 0"
            if f.n >= 2**32 and entry in ("zmean", "zmean_classes"):
                return "2^32 points or more in a file"
        if entry == "zmean_classes" and not all(0 <= int(v) < 256 for v in q.classes):
            return "a class outside a byte"
    if entry == "polygon":
        if not 3 <= len(q.xy) <= POLYGON_VERTS_MAX:
            return "vertex count"
        for f, lmin, lmax in alive:
            v = lattice(q.xy, f)
            if not np.all((v >= I32_MIN) & (v <= I32_MAX)) or np.any(v.max(axis=0) - v.min(axis=0) > I32_MAX):
                return "the outline does not fit a file's lattice"
    e = getattr(q, "edges", None)  # (attached to the box once it is accepted)
    if e is not None and (len(e) < 2 or np.isnan(e).any() or np.any(e[:-1] > e[1:])):
        return "edges"
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy's answers
# ---------------------------------------------------------------------------------------------------------------------------------
def scanned_of(alive):
    return sum(f.n for f, _, _ in alive)


def z_groups(alive):
    """The surviving files by the bits of (scale_z, offset_z), groups in the order of their first file, files in load order"""
    groups = {}
    for row in alive:
        groups.setdefault(struct.pack("<dd", row[0].scale[2], row[0].offset[2]), []).append(row)
    return list(groups.values())


def zmean_groups(files, q, classes, header=True):
    """(per z lattice in merge order its (scale_z, offset_z, counts, sums of the stored z), both int64 per cell; points_scanned).
    classes None: every point.  No file here comes near 2^32 points, so a group is one batch."""
    alive = survivors(files, *raster_world_box(q), header)
    words = q.nx * q.ny
    table = np.ones(256, dtype=bool)
    if classes is not None:
        table[:] = False
        table[list(classes)] = True
    out = []
    for members in z_groups(alive):
        cnt, zsum = np.zeros(words, dtype=np.int64), np.zeros(words, dtype=np.int64)
        for f, lmin, lmax in members:
            k = [steps_of(q.cell, f.scale[a]) for a in range(2)]
            p = f.xyz.astype(np.int64)
            sel = pp.in_box(p, [lmin[0], lmin[1], lmin[2]], [lmin[0] + q.nx * k[0] - 1, lmin[1] + q.ny * k[1] - 1, lmax[2]]) & table[f.cls]
            cell = ((p[sel, 1] - lmin[1]) // k[1]) * q.nx + (p[sel, 0] - lmin[0]) // k[0]
            np.add.at(cnt, cell, 1)
            np.add.at(zsum, cell, p[sel, 2])
        out.append((float(members[0][0].scale[2]), float(members[0][0].offset[2]), cnt, zsum))
    return out, scanned_of(alive)


def zmean_merge(groups, words, product=None):
    """(count, zmean): the rule above ResidentDataset::zmean_raster in Python floats, which round every product and fuse nothing:
    per group in order and per cell a = offset * float(cnt), b = scale * float(sum), W += a + b, N += cnt; then W / N, NaN where N
    is 0.  product: another way to a group's term (the plan test's mutants)"""
    W, N = [0.0] * words, np.zeros(words, dtype=np.int64)
    for scale, offset, cnt, zsum in groups:
        for c in np.flatnonzero(cnt).tolist():  # (a cell the group does not reach adds offset * 0.0 + scale * 0.0 = 0.0)
            if product is None:
                a = offset * float(int(cnt[c]))
                b = scale * float(int(zsum[c]))
                W[c] += a + b
            else:
                W[c] += product(scale, offset, int(cnt[c]), int(zsum[c]))
        N += cnt
    zmean = np.asarray([W[c] / float(int(N[c])) if N[c] else np.nan for c in range(words)], dtype=np.float64)
    return N, zmean


def fused_term(scale, offset, cnt, zsum):
    """A group's term with scale * sum contracted into the add: one rounding of scale * sum + a instead of two, exact in rationals
    (a = offset * float(cnt) is exact for OFFSETS, so contracting the other product changes nothing)"""
    return float(Fraction(scale) * zsum + Fraction(offset * float(cnt)))


def zmean_mutants(groups, words):
    """(cells whose mean changes when the groups merge in the reverse order, cells whose mean changes under fused_term)"""
    bits = zmean_merge(groups, words)[1].view(np.uint64)
    return (int((zmean_merge(groups[::-1], words)[1].view(np.uint64) != bits).sum()),
            int((zmean_merge(groups, words, fused_term)[1].view(np.uint64) != bits).sum()))


def zmean_answer(files, q, classes, header=True):
    """(count, zmean, points_scanned, per group its counts)"""
    groups, scanned = zmean_groups(files, q, classes, header)
    count, zmean = zmean_merge(groups, q.nx * q.ny)
    return count, zmean, scanned, [g[2] for g in groups]


def answer(files, entry, q, header=True):
    """The entry's outputs as a dict of int64 / f64 arrays and integers"""
    if entry in ("zmean", "zmean_classes"):
        count, zmean, scanned, _ = zmean_answer(files, q, q.classes if entry == "zmean_classes" else None, header)
        return dict(count=count, zmean=zmean, scanned=scanned)
    if entry == "class":
        return dict(matches=sum(int((f.cls == q.cls).sum()) for f in files), scanned=sum(f.n for f in files))
    if entry == "many":
        per = [survivors(files, a, b, header) for a, b in zip(q.bmin, q.bmax)]
        read = 0
        for g in range(0, len(per), MULTI_BOX_MAX):
            met = {id(f): f.n for alive in per[g:g + MULTI_BOX_MAX] for f, _, _ in alive}
            read += sum(met.values())
        return dict(matches=np.asarray([sum(pp.box_count(f.xyz, lo, hi) for f, lo, hi in alive) for alive in per], dtype=np.int64),
                    scanned=np.asarray([scanned_of(alive) for alive in per], dtype=np.int64), read=read)
    if entry in ("raster", "zrange"):
        box = raster_world_box(q)
        alive = survivors(files, *box, header)
        cnt = np.zeros(q.nx * q.ny, dtype=np.int64)
        zlo, zhi = np.full(q.nx * q.ny, np.nan), np.full(q.nx * q.ny, np.nan)
        for f, lmin, lmax in alive:
            k = [steps_of(q.cell, f.scale[a]) for a in range(2)]
            p = f.xyz.astype(np.int64)
            sel = pp.in_box(p, [lmin[0], lmin[1], lmin[2]], [lmin[0] + q.nx * k[0] - 1, lmin[1] + q.ny * k[1] - 1, lmax[2]])
            cell = ((p[sel, 1] - lmin[1]) // k[1]) * q.nx + (p[sel, 0] - lmin[0]) // k[0]
            np.add.at(cnt, cell, 1)
            z = (f.xyz[sel, 2].astype(np.float64) * f.scale[2]) + f.offset[2]
            np.fmin.at(zlo, cell, z)
            np.fmax.at(zhi, cell, z)
        out = dict(scanned=scanned_of(alive))
        out.update(dict(raster=cnt) if entry == "raster" else dict(zlo=zlo, zhi=zhi))
        return out
    if entry == "polygon":
        box = polygon_world_box(q)
        alive = survivors(files, *box, header)
        total = 0
        for f, lmin, lmax in alive:
            v = lattice(q.xy, f).astype(np.int64)
            total += int(rule.counted(f.xyz, [int(v[:, 0].min()), int(v[:, 1].min()), lmin[2]], [int(v[:, 0].max()), int(v[:, 1].max()), lmax[2]],
                                      v.tolist()).sum())
        return dict(matches=total, scanned=scanned_of(alive))
    alive = survivors(files, q.bmin, q.bmax, header)
    out = dict(scanned=scanned_of(alive))
    if entry == "bounds":
        out["matches"] = sum(pp.box_count(f.xyz, lo, hi) for f, lo, hi in alive)
    elif entry == "bounds_class":
        out["matches"] = sum(int((pp.in_box(f.xyz, lo, hi) & (f.cls == q.cls)).sum()) for f, lo, hi in alive)
    elif entry == "bounds_time":
        out["matches"] = sum(int((pp.in_box(f.xyz, lo, hi) & in_range(f.t, q.t0, q.t1)).sum()) for f, lo, hi in alive)
    elif entry == "by_class":
        out["hist"] = sum([np.bincount(f.cls[pp.in_box(f.xyz, lo, hi)], minlength=256) for f, lo, hi in alive], np.zeros(256, dtype=np.int64))
    else:
        t = np.concatenate([f.t[pp.in_box(f.xyz, lo, hi)] for f, lo, hi in alive] + [np.zeros(0)])
        out["hist"] = np.asarray([int(in_range(t, q.edges[b], q.edges[b + 1]).sum()) for b in range(len(q.edges) - 1)], dtype=np.int64)
    return out


def total(ans):
    """How much an answer holds: its matches, or the cells a height raster reaches"""
    for key in ("matches", "hist", "raster", "count"):
        if key in ans:
            return int(np.sum(ans[key]))
    return int((~np.isnan(ans["zlo"])).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# queries
# ---------------------------------------------------------------------------------------------------------------------------------
def a_world_point(rng, files):
    """(file, index, world point): of a file with points, in a lying file often one that its header hides"""
    full = [f for f in files if f.n]
    if not full:
        return None, None, np.asarray([float(rng.choice(OFFSETS)) for _ in range(3)])
    f = full[int(rng.integers(0, len(full)))]
    idx = np.flatnonzero(f.hidden) if f.lying and rng.random() < 0.4 else np.arange(f.n)
    i = int(idx[rng.integers(0, len(idx))])
    return f, i, f.world[i]


def draw_box(rng, files, **more):
    """A box around a world point; more: cls=True — the class to ask for, mostly that point's; t=(t0, t1) — the case's time range,
    or an empty, a reversed, a NaN or an unbounded one; edges — the case's"""
    f, i, c = a_world_point(rng, files)
    h = [float(rng.choice(HALF_WORLD, p=HALF_WORLD_P)) for _ in range(3)]
    q = SimpleNamespace(bmin=tuple(float(c[a] - h[a]) for a in range(3)), bmax=tuple(float(c[a] + h[a]) for a in range(3)))
    if "cls" in more:
        q.cls = int(f.cls[i]) if f is not None and rng.random() < 0.85 else int(rng.integers(0, 256))
    if "t" in more:
        t0, t1 = more["t"]
        u = rng.random()
        q.t0, q.t1 = (t0, t0) if u < 0.04 else (t1, t0) if u < 0.08 else (np.nan, t1) if u < 0.12 else (-np.inf, np.inf) if u < 0.2 else (t0, t1)
    if "edges" in more:
        q.edges = more["edges"]
    return q


def draw_raster(rng, files, shapes):
    f, i, c = a_world_point(rng, files)
    nx, ny = shapes[int(rng.integers(0, len(shapes)))]
    cell = float(rng.choice(CELL_SIZES))
    hz = float(rng.choice(HALF_Z))
    return SimpleNamespace(bmin=(float(c[0] - rng.random() * nx * cell), float(c[1] - rng.random() * ny * cell), float(c[2] - hz)),
                           zmax=float(c[2] + hz), cell=cell, nx=nx, ny=ny)


SET_KINDS = ("none", "all", "one", "few")
SET_KINDS_P = (0.12, 0.2, 0.38, 0.3)


def draw_zmean(rng, files, kind=None):
    """A raster of more cells than one launch holds around a world point; kind (of SET_KINDS): and a class set — the empty one, all
    256, one class (mostly that point's) or a few of the files' classes with a stranger among them"""
    f, i, c = a_world_point(rng, files)
    nx, ny = ZMEAN_SHAPES[int(rng.integers(0, len(ZMEAN_SHAPES)))]
    cell = float(rng.choice(CELL_SIZES))
    hz = float(rng.choice(HALF_Z))
    lo, hi = np.asarray(c, dtype=np.float64), np.asarray(c, dtype=np.float64)
    if f is not None and rng.random() < 0.6:  # over a point of every other file that still fits: files of several z lattices in one raster
        cell, hz = float(rng.choice(ZMEAN_CELL_SIZES)), HALF_Z[-1]
        others = [g for g in files if g.n and g is not f]
        for j in rng.permutation(len(others)):
            w = others[j].world[int(rng.integers(0, others[j].n))]
            a, b = np.minimum(lo, w), np.maximum(hi, w)
            if b[0] - a[0] < 0.9 * nx * cell and b[1] - a[1] < 0.9 * ny * cell:
                lo, hi = a, b
    room = [min(n * cell - (hi[a] - lo[a]), cell / 2, 2e5) for a, n in enumerate((nx, ny))]  # (the origin stays inside the finest lattices)
    q = SimpleNamespace(bmin=(float(lo[0] - rng.random() * room[0]), float(lo[1] - rng.random() * room[1]), float(lo[2] - hz)),
                        zmax=float(hi[2] + hz), cell=cell, nx=nx, ny=ny)
    if kind is not None:
        held = np.unique(np.concatenate([g.cls for g in files] + [np.zeros(1, dtype=np.uint8)]))
        if kind == "none":
            q.classes = ()
        elif kind == "all":
            q.classes = tuple(range(256))
        elif kind == "one":
            q.classes = (int(f.cls[i]) if f is not None and rng.random() < 0.85 else int(rng.choice(held)),)
        else:
            few = set(int(v) for v in rng.choice(held, int(rng.integers(2, 6)))) | {int(rng.integers(0, 256))}
            if f is not None and rng.random() < 0.7:
                few.add(int(f.cls[i]))
            q.classes = tuple(sorted(few))
    return q


def most_merged(rng, files, entry, make):
    """Of TRIES queries the one, among those the product accepts, that tells the most about the merge: a mean that another order of
    the groups changes, a mean that a fused product changes (zmean_mutants), then the most z lattices in one cell and the most cells
    that two lattices reach.  None: none accepted."""
    best, best_score = None, None
    for _ in range(TRIES):
        q = make()
        if refusal(files, entry, q) is not None:
            continue
        groups, _ = zmean_groups(files, q, q.classes if entry == "zmean_classes" else None)
        reach = np.sum([g[2] > 0 for g in groups], axis=0) if groups else np.zeros(1, dtype=np.int64)
        order, fused = zmean_mutants(groups, q.nx * q.ny)
        score = ((order > 0) + (fused > 0), int(reach.max()), int((reach >= 2).sum()))
        if best is None or score > best_score:
            best, best_score = q, score
    return best


def draw_polygon(rng, files):
    f, i, c = a_world_point(rng, files)
    nverts = POLYGON_VERTS_MAX if rng.random() < 0.12 else int(rng.integers(3, 13))
    h = [float(rng.choice((1.0, 100.0, 1e4, 1e6))) for _ in range(2)]
    lo, hi = [c[a] - h[a] for a in range(2)], [c[a] + h[a] for a in range(2)]
    near = np.zeros((0, 3)) if f is None else f.world[np.all((f.world[:, :2] >= lo) & (f.world[:, :2] <= hi), axis=1)]
    xy = [] if rng.random() < 0.4 else [[lo[0], lo[1]], [hi[0], lo[1]], [hi[0], hi[1]], [lo[0], hi[1]]][:nverts]
    while len(xy) < nverts:
        u = rng.random()
        if u < 0.3 and len(near):
            v = [float(w) for w in near[rng.integers(0, len(near)), :2]]
        else:
            v = [float(rng.uniform(lo[a], hi[a])) for a in range(2)]
            if u > 0.8 and xy:
                a = int(rng.integers(0, 2))
                v[a] = xy[-1][a]
        xy.append(v)
    hz = float(rng.choice(HALF_Z))
    return SimpleNamespace(xy=xy, zmin=float(c[2] - hz), zmax=float(c[2] + hz))


def accepted(rng, files, entry, make):
    """make() until the product would not refuse it — and, six times in seven, until numpy's answer holds something; failing that,
    a query that every lattice converts: a box that holds everything, a raster or an outline beyond every header"""
    legal = None
    for _ in range(TRIES):
        q = make()
        if refusal(files, entry, q) is None:
            legal = q
            if rng.random() < 0.15 or total(answer(files, entry, q)) > 0:
                return q
    if legal is not None:
        return legal
    far = 3e7
    q = (SimpleNamespace(xy=[[far, far], [far + 9.0, far], [far, far + 9.0]], zmin=-1.0, zmax=1.0) if entry == "polygon"
         else SimpleNamespace(bmin=(far, far, -1.0), zmax=1.0, cell=1.0, nx=make().nx, ny=1, classes=(2,)) if entry in RASTER_ENTRIES
         else make())
    if entry in BOX_ENTRIES:
        q.bmin, q.bmax = (-1e7, -1e7, -1e7), (1e7, 1e7, 1e7)
    assert refusal(files, entry, q) is None, entry
    return q


def draw(seed):
    rng = np.random.default_rng(BASE + SEED_BASE + seed)
    c = SimpleNamespace(seed=seed)
    edges = draw_edges(rng)
    if rng.random() < 0.15:  # more bins than one launch holds
        edges = np.sort(rng.integers(0, 2000, int(rng.integers(1026, 1500)))).astype(np.float64) / 2
    t0, t1 = float(rng.integers(0, 800)) / 2, float(rng.integers(1200, 2000)) / 2
    c.files = [draw_file(rng, edges, (t0, t1)) for _ in range(int(rng.integers(2, 7)))]
    files = c.files
    c.q = {"class": SimpleNamespace(cls=int(rng.choice(np.concatenate([f.cls for f in files] + [np.zeros(1, dtype=np.uint8)]))))}
    more = {"bounds": {}, "bounds_class": dict(cls=True), "bounds_time": dict(t=(t0, t1)), "by_class": {}, "by_time": dict(edges=edges)}
    for entry in BOX_ENTRIES:
        c.q[entry] = accepted(rng, files, entry, lambda: draw_box(rng, files, **more[entry]))
    boxes = [accepted(rng, files, "bounds", lambda: draw_box(rng, files)) for _ in range(int(rng.integers(1, 21)))]
    c.q["many"] = SimpleNamespace(bmin=[b.bmin for b in boxes], bmax=[b.bmax for b in boxes])
    assert refusal(files, "many", c.q["many"]) is None
    c.q["raster"] = accepted(rng, files, "raster", lambda: draw_raster(rng, files, RASTER_SHAPES))
    c.q["zrange"] = accepted(rng, files, "zrange", lambda: draw_raster(rng, files, ZRANGE_SHAPES))
    c.q["polygon"] = accepted(rng, files, "polygon", lambda: draw_polygon(rng, files))
    for entry in ("zmean", "zmean_classes"):  # (each from a generator of its own, behind everything the first ten draw)
        own = np.random.default_rng([BASE + SEED_BASE + seed, TAGS[entry]])
        kind = str(own.choice(SET_KINDS, p=SET_KINDS_P)) if entry == "zmean_classes" else None
        c.q[entry] = most_merged(own, files, entry, lambda: draw_zmean(own, files, kind))
        if c.q[entry] is None:
            c.q[entry] = accepted(own, files, entry, lambda: draw_zmean(own, files, kind))
        c.q[entry].kind = kind
    c.answer = {e: answer(files, e, c.q[e]) for e in ENTRIES}
    # the entries whose answer a lying header decides: with every header ignored the answer is another one
    c.lie_decides = []
    if any(f.lying for f in files):
        for e in ENTRIES:
            if e != "class":
                try:
                    if total(answer(files, e, c.q[e], header=False)) != total(c.answer[e]):
                        c.lie_decides.append(e)
                except (pkg.PcqError, TypeError):  # (a file the header keeps out does not convert the box, or has no whole cell)
                    pass
    return c


@functools.lru_cache(maxsize=None)
def case(seed):
    """draw(seed), kept: the mean-height entries try TRIES queries each"""
    return draw(seed)
