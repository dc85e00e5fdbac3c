"""The height-spread raster's merge (host/zmoments_merge.h, include/pcq_query_moments.h) restated in python: integers as python ints,
floats as python floats (IEEE f64, round to nearest even, no fused multiply-add), every product and quotient a statement of its own.
A batch of one cell is (scale, offset, cnt, sum, lo, hi): the z lattice and the four exact words of pcq_scan_dev_zmoments_raster_batch.

merge(batches) is the product's formula; merge(batches, mutant=...) is one of four wrong ones the tests prove they would see; exact()
is the same statistic in rationals, for the independent check; words() makes a batch's four integers of stored heights.

Below that, what the GPU tests of the device entry share: the segment sizes, the preset words, and Dev — segments in HBM, four arrays
to add into, numpy's answer to a call on int64.
"""
import math
import os
import struct
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402

NAN = float("nan")
MUTANTS = ("fused_wb", "m2_twice", "no_delta", "d_low_only")


def bits(x):
    """the 64 bits of an f64, so that NaNs and signed zeros compare"""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def words(zs):
    """(cnt, sum, lo, hi) of a list of stored i32 heights: what one launch from zeroed words gives (fewer than 2^32 points)"""
    zs = [int(z) for z in zs]
    return len(zs), sum(zs), sum((z * z) & 0xffffffff for z in zs), sum((z * z) >> 32 for z in zs)


def _fma(a, b, c):
    """a * b + c rounded once: exact in rationals, then to the nearest f64 (Fraction -> float rounds to nearest even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def merge(batches, mutant=None):
    """(count, zmean, zstd) of one cell over its batches in order"""
    assert mutant is None or mutant in MUTANTS
    W, M, N = 0.0, 0.0, 0
    for scale, offset, cnt, s, lo, hi in batches:
        if cnt == 0:
            continue
        assert 0 < cnt < 2**32 and -2**63 <= s < 2**63 and 0 <= lo < 2**64 and 0 <= hi < 2**64
        Q = hi * 2**32 + lo
        D = cnt * Q - s * s
        assert 0 <= D < 2**127
        n = float(cnt)
        dh = float(D >> 64) * 2.0**64
        dl = float(D & (2**64 - 1))
        d = dh + dl
        if mutant == "d_low_only":
            d = dl
        a = offset * n
        b = scale * float(s)
        wb = a + b
        if mutant == "fused_wb":
            wb = _fma(scale, float(s), a)
        ss = scale * scale
        q = d / n
        if mutant == "m2_twice":
            q = q / n
        m2 = ss * q
        if N and mutant != "no_delta":
            mb = wb / n
            mw = W / float(N)
            delta = mb - mw
            dd = delta * delta
            nn = float(N) * n
            f = nn / float(N + cnt)
            t = dd * f
            M += t
        M += m2
        W += wb
        N += cnt
    if not N:
        return 0, NAN, NAN
    v = M / float(N)
    return N, W / float(N), math.sqrt(v)


def exact(batches):
    """(count, mean, variance) in rationals, the scale and offset taken as the f64 values they are"""
    N, S1, S2 = 0, Fraction(0), Fraction(0)
    for scale, offset, cnt, s, lo, hi in batches:
        sc, off = Fraction(scale), Fraction(offset)
        N += cnt
        S1 += off * cnt + sc * s
        S2 += off * off * cnt + 2 * off * sc * s + sc * sc * (hi * 2**32 + lo)
    if not N:
        return 0, None, None
    mean = S1 / N
    return N, mean, S2 / N - mean * mean


def sqrt_fraction(v, digits=40):
    """the square root of a non-negative rational to `digits` decimal digits, as a rational"""
    scaled = v * 10**(2 * digits)
    return Fraction(math.isqrt(scaled.numerator // scaled.denominator), 10**digits)


# ---------------------------------------------------------------------------------------------------------------------------------
# the device entry (pcq_scan_dev_zmoments_raster_batch) against numpy: what the GPU tests share.  Nothing below runs at import.
# ---------------------------------------------------------------------------------------------------------------------------------
NS = (0, 1, 511, 512, 513, 1535, 4133)
I32_MIN, I32_MAX = -2**31, 2**31 - 1
CELLS_MAX = 1024
WORDS = CELLS_MAX + 64
NAMES = ("count", "sum", "zsq_lo", "zsq_hi")
EMPTY = ([5, 5, 5], [4, 4, 4])
PRE = (np.asarray([(0, 2**32 - 1, 2**40 + c)[c % 3] for c in range(WORDS)], dtype=np.int64),
       np.asarray([(0, -1, 2**62, -2**62 + c)[c % 4] for c in range(WORDS)], dtype=np.int64),
       np.asarray([(0, 2**32 - 1, 2**33 + c)[c % 3] for c in range(WORDS)], dtype=np.int64),
       np.asarray([(2**32 - 1, -1 - c, 0)[c % 3] for c in range(WORDS)], dtype=np.int64))
ZEROS = tuple(np.zeros(WORDS, dtype=np.int64) for _ in NAMES)
PLANTED = (I32_MIN, I32_MAX, 0, -1, 46341, -46341, 65535, -65535, 65536, -65536)


def origin(k):
    return 1000 * k - 300, 77 - 500 * k


def box_of(k, nx, ny, cw, z=None):
    """Segment k's box: nx x ny full cells from its origin, and a slab of z that keeps about half of the i32 range"""
    ox, oy = origin(k)
    zlo, zhi = (-2**30 + k, 2**30 - k) if z is None else z
    return [ox, oy, zlo], [ox + nx * cw[0] - 1, oy + ny * cw[1] - 1, zhi]


def draw(rng, nx, ny, cws, margin=2, ns=NS):
    """Positions of every segment: x and y independent over the segment's raster and `margin` lattice steps around it, z over the
    whole i32 range (both signs, squares with both halves set)"""
    out = []
    for k, n in enumerate(ns):
        ox, oy = origin(k)
        out.append(np.stack([ox + rng.integers(-margin, nx * cws[k][0] + margin, n), oy + rng.integers(-margin, ny * cws[k][1] + margin, n),
                             rng.integers(I32_MIN, I32_MAX + 1, n)], axis=1).astype(np.int32))
    return out


def four(z):
    """what a point of height z (int64 array) adds to the four words of its cell (int64 adds wrap modulo 2^64, as the entry's do)"""
    return np.ones_like(z), z, (z * z) & 0xffffffff, (z * z) >> 32


class Dev:
    """Segments of `ns` points in HBM, four arrays of WORDS words to add into, and numpy's answer to a call"""

    def __init__(self, ctx, ns=NS):
        import importlib
        self.pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
        binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
        self.ctx, self.ns = ctx, tuple(ns)
        self.poff, self.psize = pp.carve(self.ns, [0] * len(self.ns), 12)
        self.blocks = [ctx.alloc(self.psize + 64)] + [ctx.alloc(8 * WORDS) for _ in range(6)]
        self.d_pos, self.d_words, self.d_zsum_words = self.blocks[0], self.blocks[1:5], self.blocks[5:7]
        assert all(p % 16 == 0 for p in self.blocks) and all(o % 16 == 0 for o in self.poff)
        self.cols = [binding.make_columns(xyz=self.d_pos + p, n=n) for p, n in zip(self.poff, self.ns)]
        self.xyz = None
        self.pre = PRE
        self.wraps = None

    def upload(self, xyz):
        assert [len(a) for a in xyz] == list(self.ns)
        img = np.zeros(self.psize, dtype=np.uint8)
        for o, a in zip(self.poff, xyz):
            img[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.ctx.to_device(self.d_pos, img)
        self.xyz = xyz

    def cells_and_z(self, boxes, cws, nx, ny, segments=None):
        """(cell, z) of every point the call keeps, int64"""
        cells, zs = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
        for k, (lo, hi), cw in zip(range(len(self.ns)) if segments is None else segments, boxes, cws):
            p = self.xyz[k][pp.in_box(self.xyz[k], lo, hi)].astype(np.int64)
            cell = ((p[:, 1] - int(lo[1])) // int(cw[1])) * nx + (p[:, 0] - int(lo[0])) // int(cw[0])
            assert not len(cell) or (0 <= cell.min() and cell.max() < nx * ny)
            cells.append(cell), zs.append(p[:, 2])
        return np.concatenate(cells), np.concatenate(zs)

    def presets(self, cell, z):
        """PRE, with 2^64 - 1 in the low word of every other cell that receives a point whose z^2 mod 2^32 is not 0"""
        lo = PRE[2].copy()
        hit = np.zeros(WORDS, dtype=bool)
        hit[cell[((z * z) & 0xffffffff) != 0]] = True
        wrap = np.flatnonzero(hit)[::2]
        lo[wrap] = -1
        return (PRE[0], PRE[1], lo, PRE[3]), len(wrap)

    def want(self, cell, z, pre):
        out = [p.copy() for p in pre]
        for w, v in zip(out, four(z)):
            np.add.at(w, cell, v)
        return out

    def preset(self, pre):
        self.pre = pre
        for d, p in zip(self.d_words, pre):
            self.ctx.to_device(d, np.ascontiguousarray(p, dtype=np.int64))

    def words(self, ds=None):
        out = []
        for d in self.d_words if ds is None else ds:
            w = np.zeros(WORDS, dtype=np.int64)
            self.ctx.to_host(w, d)  # (waits for the context's stream)
            out.append(w)
        return out

    def launch(self, boxes, cws, nx, ny, segments=None, cols=None, preds=None, ds=None, stream=None):
        if cols is None:
            cols = self.cols if segments is None else [self.cols[k] for k in segments]
        if preds is None:
            preds = [self.pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
        self.ctx.scan_dev_zmoments_raster_batch(cols, preds, cws, nx, ny, *(self.d_words if ds is None else ds), stream=stream)

    def compare(self, want, nx, ny):
        for name, g, w in zip(NAMES, self.words(), want):
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (name, nx, ny, [(int(c), int(g[c]), int(w[c])) for c in bad[:12]], len(bad))

    def check(self, boxes, cws, nx, ny, segments=None, pre=None, stream=None, sync=None):
        """One call from the preset words (None: presets()): every word of the four arrays is numpy's; returns what the call added to
        the raster's words of each array"""
        cell, z = self.cells_and_z(boxes, cws, nx, ny, segments)
        wraps = None
        if pre is None:
            pre, wraps = self.presets(cell, z)
        self.preset(pre)
        self.launch(boxes, cws, nx, ny, segments, stream=stream)
        if sync:
            sync()
        want = self.want(cell, z, pre)
        self.compare(want, nx, ny)
        self.wraps = wraps
        return [(w - p)[:nx * ny] for w, p in zip(want, pre)]

    def unchanged(self):
        return all(np.array_equal(g, p) for g, p in zip(self.words(), self.pre))

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


# ---------------------------------------------------------------------------------------------------------------------------------
# the host entry (pcq_query_resident_bounds_zstd_raster) restated over the files of tests/_resident_files.py
# ---------------------------------------------------------------------------------------------------------------------------------
def file_words(h, ras):
    """four int64 arrays of nx * ny: points, sum of the stored z, and the low and high halves of the sum of their squares per cell
    of one file (a _resident_files.Held) — the stored integers inside lmin .. lmin + n k - 1 on x and y (lmin from pcq_box_to_local,
    k the cell in the file's lattice steps) and inside the converted z range.  ras: (bmin, zmax, cell_size, nx, ny)"""
    import importlib
    import _resident_files as rf
    pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
    bmin, zmax, cell, nx, ny = ras
    box = rf.world_box(ras)
    lmin, lmax = pkg.box_to_local(list(box[0]), list(box[1]), list(h.scale), list(h.offset))
    k = [round(cell / h.scale[a]) for a in range(2)]
    assert all(abs(cell / h.scale[a] - k[a]) <= 1e-9 * k[a] for a in range(2))
    x = h.xyz.astype(np.int64)
    cx, cy = (x[:, 0] - lmin[0]) // k[0], (x[:, 1] - lmin[1]) // k[1]
    sel = (x[:, 0] >= lmin[0]) & (cx < nx) & (x[:, 1] >= lmin[1]) & (cy < ny) & (x[:, 2] >= lmin[2]) & (x[:, 2] <= lmax[2])
    z = x[sel, 2]
    out = [np.zeros(nx * ny, dtype=np.int64) for _ in range(4)]
    for w, v in zip(out, four(z)):
        np.add.at(w, cy[sel] * nx + cx[sel], v)
    return out


def batches_of(held, ras):
    """The surviving files (header meets the world box, points) grouped by bitwise-equal (scale[2], offset[2]), in the order of each
    group's first file, each group's exact integers per cell: [(scale, offset, [cnt, sum, lo, hi])]"""
    import _resident_files as rf
    box = rf.world_box(ras)
    out = {}
    for h in held:
        if not rf.meets(h, box) or not len(h.xyz):
            continue
        key = struct.pack("<dd", h.scale[2], h.offset[2])
        w = file_words(h, ras)
        if key in out:
            out[key] = (out[key][0], out[key][1], [a + b for a, b in zip(out[key][2], w)])
        else:
            out[key] = (float(h.scale[2]), float(h.offset[2]), w)
    return list(out.values())  # (dicts keep insertion order)


def restated(held, ras):
    """(count, bits of zmean, bits of zstd) per cell from merge(), the number of cells whose batches are two or more with points,
    and the number of batches"""
    _, _, _, nx, ny = ras
    groups = batches_of(held, ras)
    cnt, mean, std, both = [], [], [], 0
    for c in range(nx * ny):
        bs = [(scale, offset) + tuple(int(w[c]) for w in ws) for scale, offset, ws in groups]
        n, m, s = merge(bs)
        both += sum(b[2] > 0 for b in bs) >= 2
        cnt.append(n), mean.append(bits(m)), std.append(bits(s))
    return np.asarray(cnt, dtype=np.uint64), np.asarray(mean, dtype=np.uint64), np.asarray(std, dtype=np.uint64), both, len(groups)
