"""The small LAST corpora of the resident-dataset tests (tests/test_gpu_resident_*.py), from one writer.

FIVE_FILES is the corpus most of them share: formats 1, 3 and 6; 3*4096+17, 4096, 100, 0 and 2*4096+5 points; differing scales
and offsets, one of them anisotropic (the box conversion of last.rs:100-102 then moves a min corner); and one file (LYING) whose
header says x <= LYING_XMAX although its points go beyond, so that the header early-out (last.rs:92-94) is observable.  Every
module writes it with its own seed: the bytes on disk are pinned by tests/test_resident_files.py.
"""
import collections
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import _time_images as ti  # noqa: E402

ISO = (0.01, 0.01, 0.01)
# (format, points, scale, offset); ints are x, y in [-5000, 5000), z in [-1000, 1000)
FIVE_FILES = [(1, 3 * 4096 + 17, ti.SCALE, ti.OFFSET),             # world x [50, 150), y [-300, -100), z [-42.5, 57.5): anisotropic
              (3, 4096, ISO, (0.0, 0.0, 0.0)),                      # x, y [-50, 50), z [-10, 10)
              (6, 100, (0.001, 0.001, 0.001), (100.0, -200.0, 0.0)),  # x [95, 105), y [-205, -195), z [-1, 1)
              (1, 0, ISO, (0.0, 0.0, 0.0)),
              (3, 2 * 4096 + 5, ISO, (300.0, 0.0, 0.0))]            # x [250, 350): its header says x <= 300
LYING, LYING_XMAX = 4, 300.0

# What a file holds: the stored integers, class bytes and times, its lattice, its header AABB (as written) and its bytes.
Held = collections.namedtuple("Held", "xyz cls t scale offset hmin hmax image")


def write_files(d, specs, seed, lying=None, classes=None):
    """Writes one LAST file per (format, points, scale, offset) of `specs` into the directory d, file k from
    _time_images.points(n, seed + k); returns (paths, [Held]).  lying: the index of the file whose header x maximum becomes
    LYING_XMAX.  classes: the class bytes are default_rng(960 + k).choice(classes, n) instead."""
    paths, held = [], []
    for k, (fmt, n, scale, offset) in enumerate(specs):
        xyz, cls, rgb, t = ti.points(n, seed + k)
        if classes is not None:
            cls = np.random.default_rng(960 + k).choice(np.asarray(classes, dtype=np.uint8), n)
        img = ti.last_image(fmt, xyz, cls, rgb, t, scale=scale, offset=offset).copy()
        w = ti.world(xyz, scale, offset) if n else np.zeros((1, 3))
        hmin, hmax = w.min(axis=0), w.max(axis=0)
        if k == lying:
            assert hmax[0] > LYING_XMAX + 40.0
            hmax[0] = LYING_XMAX
            img[179:195] = np.frombuffer(struct.pack("<2d", hmax[0], hmin[0]), dtype=np.uint8)
        p = str(d / f"f{k}_{fmt}_{n}.last")
        img.tofile(p)
        paths.append(p)
        held.append(Held(xyz, cls, t, scale, offset, hmin, hmax, img))
    return paths, held


def meets(h, box):
    """The header early-out: the file's header AABB meets the box (inclusive)."""
    return bool(np.all(h.hmin <= np.asarray(box[1])) and np.all(h.hmax >= np.asarray(box[0])))


def world_box(ras):
    """The world box of a raster (bmin, zmax, cell_size, nx, ny)."""
    bmin, zmax, cell, nx, ny = ras
    return tuple(bmin), (bmin[0] + nx * cell, bmin[1] + ny * cell, zmax)
