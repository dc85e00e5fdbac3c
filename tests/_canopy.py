"""What the tests of pcq_scan_dev_zrange_raster_batch_classes share: _zsum_classes.Dev with two i32 arrays and two sets — segments of
positions and class bytes carved from two buffers in HBM, the positions pieces 16-byte aligned, class piece k at byte misalignment
mis[k] of a dword — and numpy's answer: into a copy of the presets, np.minimum.at of z over the points that pp.in_box keeps and whose
class byte is in the LOW set, np.maximum.at of z over those whose class byte is in the HIGH set.  Nothing here is a test."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402
from _zsum_classes import ALL, box_of, draw, in_set, origin  # noqa: E402,F401

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

CELLS_MAX = 4096
WORDS = CELLS_MAX + 64
I32_MIN, I32_MAX = -2**31, 2**31 - 1
SENT = np.full(WORDS, I32_MAX, dtype=np.int32), np.full(WORDS, I32_MIN, dtype=np.int32)
# presets that are no sentinels, inside the z the draws use (-50 .. 49), so that a fold keeps some words and replaces others; the
# two arrays differ in every word, so a fold into the wrong array shows
PRE_MIN = np.asarray([(-7, 12, I32_MAX, -40, 3)[c % 5] for c in range(WORDS)], dtype=np.int32)
PRE_MAX = np.asarray([(8, I32_MIN, -11, 41, -2, 30, -33)[c % 7] for c in range(WORDS)], dtype=np.int32)
assert (PRE_MIN != PRE_MAX).all()
BUT_7_18 = tuple(c for c in range(256) if c not in (7, 18))


class Dev:
    """Segments of ns[k] points.  upload(xyz, cls, mis) lays the data out; launch / want / check / compare with the two sets."""

    def __init__(self, ctx, ns):
        self.ctx, self.ns = ctx, tuple(ns)
        self.poff, self.psize = pp.carve(self.ns, [0] * len(self.ns), 12)
        _, self.csize = pp.carve(self.ns, [15] * len(self.ns), 1)  # (room for every phase)
        self.blocks = [ctx.alloc(self.psize + 64), ctx.alloc(self.csize + 64), ctx.alloc(4 * WORDS), ctx.alloc(4 * WORDS)]
        self.d_pos, self.d_cls, self.d_min, self.d_max = self.blocks
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
        cimg = np.full(self.csize + 64, 0xa5, dtype=np.uint8)
        for o, c in zip(coff, cls):
            cimg[o:o + len(c)] = np.asarray(c, dtype=np.uint8)
        self.ctx.to_device(self.d_cls, cimg)
        self.xyz, self.cls, self.mis = list(xyz), [np.asarray(c, dtype=np.uint8) for c in cls], list(mis)
        self.cols = [binding.make_columns(xyz=self.d_pos + p, cls=self.d_cls + c, n=n) for p, c, n in zip(self.poff, coff, self.ns)]
        assert [(self.d_cls + c) % 4 for c in coff] == [m % 4 for m in mis]

    def want(self, boxes, cws, nx, ny, low, high, segments=None, pre=(PRE_MIN, PRE_MAX)):
        zmin, zmax = pre[0].copy(), pre[1].copy()
        for k, (lo, hi), cw in zip(range(len(self.ns)) if segments is None else segments, boxes, cws):
            box = pp.in_box(self.xyz[k], lo, hi)
            p = self.xyz[k].astype(np.int64)
            cell = ((p[:, 1] - int(lo[1])) // max(int(cw[1]), 1)) * nx + (p[:, 0] - int(lo[0])) // max(int(cw[0]), 1)
            assert not box.any() or (0 <= cell[box].min() and cell[box].max() < nx * ny)
            z = self.xyz[k][:, 2]
            kl, kh = box & in_set(self.cls[k], low), box & in_set(self.cls[k], high)
            np.minimum.at(zmin, cell[kl], z[kl])
            np.maximum.at(zmax, cell[kh], z[kh])
        return zmin, zmax

    def preset(self, pre=(PRE_MIN, PRE_MAX)):
        self.ctx.to_device(self.d_min, np.ascontiguousarray(pre[0], dtype=np.int32))
        self.ctx.to_device(self.d_max, np.ascontiguousarray(pre[1], dtype=np.int32))

    def words(self):
        zmin, zmax = np.zeros(WORDS, dtype=np.int32), np.zeros(WORDS, dtype=np.int32)
        self.ctx.to_host(zmin, self.d_min)  # (waits for the context's stream)
        self.ctx.to_host(zmax, self.d_max)
        return zmin, zmax

    def launch(self, boxes, cws, nx, ny, low, high, segments=None, cols=None, preds=None, d_zmin=None, d_zmax=None, stream=None):
        if cols is None:
            cols = self.cols if segments is None else [self.cols[k] for k in segments]
        if preds is None:
            preds = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
        self.ctx.scan_dev_zrange_raster_batch_classes(cols, preds, cws, nx, ny, low, high, self.d_min if d_zmin is None else d_zmin,
                                                      self.d_max if d_zmax is None else d_zmax, stream=stream)

    def compare(self, want, what=""):
        got = self.words()
        for name, g, w in (("zmin", got[0], want[0]), ("zmax", got[1], want[1])):
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (name, what, [(int(c), int(g[c]), int(w[c])) for c in bad[:12]], len(bad))

    def check(self, boxes, cws, nx, ny, low, high, segments=None, pre=(PRE_MIN, PRE_MAX), stream=None):
        """One call from the preset words: every word of both arrays, the guard words behind nx * ny among them, is numpy's; returns
        numpy's (zmin, zmax) of the first nx * ny cells"""
        self.preset(pre)
        self.launch(boxes, cws, nx, ny, low, high, segments, stream=stream)
        want = self.want(boxes, cws, nx, ny, low, high, segments, pre)
        assert np.array_equal(want[0][nx * ny:], pre[0][nx * ny:]) and np.array_equal(want[1][nx * ny:], pre[1][nx * ny:])
        self.compare(want, (nx, ny, sorted(low)[:8], sorted(high)[:8], self.mis))
        return want[0][:nx * ny], want[1][:nx * ny]

    def unchanged(self, pre=(PRE_MIN, PRE_MAX)):
        zmin, zmax = self.words()
        return np.array_equal(zmin, pre[0]) and np.array_equal(zmax, pre[1])

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


# ---------------------------------------------------------------------------------------------------------------------
# the resident entry: include/pcq_query_canopy.h's definition restated over _resident_files.Held
# ---------------------------------------------------------------------------------------------------------------------
def host_canopy(lib, r, ras, low, high, height=True, scanned=True, fill=(-7.25, 3.5, 11.0, 77)):
    """pcq_query_resident_bounds_canopy_raster into outputs preset to `fill`: (status, zground, zsurface, height, points_scanned)"""
    import ctypes as C
    bmin, zmax, cell, nx, ny = ras
    zg, zs, h = (np.full(nx * ny, v, dtype=np.float64) for v in fill[:3])
    s = C.c_uint64(fill[3])
    pd = C.POINTER(C.c_double)
    g = None if low is None else (C.c_uint32 * 8)(*binding.class_set_words(low))
    u = None if high is None else (C.c_uint32 * 8)(*binding.class_set_words(high))
    rc = lib.pcq_query_resident_bounds_canopy_raster(r, (C.c_double * 3)(*bmin), zmax, cell, nx, ny, g, u, zg.ctypes.data_as(pd),
                                                     zs.ctypes.data_as(pd), h.ctypes.data_as(pd) if height else None,
                                                     C.byref(s) if scanned else None)
    return rc, zg.reshape(ny, nx), zs.reshape(ny, nx), h.reshape(ny, nx), s.value


def host_untouched(zg, zs, h, s, fill=(-7.25, 3.5, 11.0, 77)):
    return (zg == fill[0]).all() and (zs == fill[1]).all() and (h == fill[2]).all() and s == fill[3]


def file_extremes(h, ras, low, high):
    """(lowest stored z per cell over the points of `low`, highest over the points of `high`) of one file, int64 with the sentinels
    INT32_MAX / INT32_MIN where it has none"""
    import _resident_files as rf
    bmin, zmax, cell, nx, ny = ras
    box = rf.world_box(ras)
    lmin, lmax = pkg.box_to_local(list(box[0]), list(box[1]), list(h.scale), list(h.offset))
    k = [round(cell / h.scale[a]) for a in range(2)]
    assert all(abs(cell / h.scale[a] - k[a]) <= 1e-9 * k[a] for a in range(2))
    x = h.xyz.astype(np.int64)
    cx, cy = (x[:, 0] - lmin[0]) // k[0], (x[:, 1] - lmin[1]) // k[1]
    sel = (x[:, 0] >= lmin[0]) & (cx < nx) & (x[:, 1] >= lmin[1]) & (cy < ny) & (x[:, 2] >= lmin[2]) & (x[:, 2] <= lmax[2])
    zmin, zmax_i = np.full((ny, nx), I32_MAX, dtype=np.int64), np.full((ny, nx), I32_MIN, dtype=np.int64)
    a, b = sel & in_set(h.cls, low), sel & in_set(h.cls, high)
    np.minimum.at(zmin, (cy[a], cx[a]), x[a, 2])
    np.maximum.at(zmax_i, (cy[b], cx[b]), x[b, 2])
    return zmin, zmax_i


def numpy_canopy(held, ras, low, high):
    """The header's definition: (zground, zsurface, height).  Groups of bitwise-equal (scale[2], offset[2]) among the files whose
    header meets the world box and that have points, in the order of each group's first file; a word that stayed at its sentinel gives
    nothing, whatever the other array holds (the sentinel rule)."""
    import struct
    import _resident_files as rf
    _, _, _, nx, ny = ras
    box = rf.world_box(ras)
    groups = {}
    for h in held:
        if rf.meets(h, box) and len(h.xyz):
            groups.setdefault(struct.pack("<dd", h.scale[2], h.offset[2]), (np.float64(h.scale[2]), np.float64(h.offset[2]), []))[2].append(h)
    lo, hi = np.full((ny, nx), np.nan), np.full((ny, nx), np.nan)
    for scale, offset, members in groups.values():
        zmin, zmax_i = np.full((ny, nx), I32_MAX, dtype=np.int64), np.full((ny, nx), I32_MIN, dtype=np.int64)
        for h in members:
            a, b = file_extremes(h, ras, low, high)
            zmin, zmax_i = np.minimum(zmin, a), np.maximum(zmax_i, b)
        wa = zmin.astype(np.float64) * scale + offset   # (the product an array of rounded f64 before the add: numpy fuses nothing)
        wb = zmax_i.astype(np.float64) * scale + offset
        with np.errstate(invalid="ignore"):
            lo = np.where((zmin != I32_MAX) & ~(lo <= wa), wa, lo)
            hi = np.where((zmax_i != I32_MIN) & ~(hi >= wb), wb, hi)
    return lo, hi, hi - lo


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()
