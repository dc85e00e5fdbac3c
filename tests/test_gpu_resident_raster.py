"""host/resident.cpp: where in this box are the points, from one pass over a dataset kept in HBM.
pcq_query_resident_count_bounds_raster must give, for every cell of the raster, the number of stored integer points of the surviving
files inside that cell's integer sub-box — lmin from pcq_box_to_local, the cell a whole number of each file's lattice steps — with
the points_scanned of pcq_query_resident_count_bounds for the same world box.

The five small LAST files of tests/_resident_files.py (FIVE_FILES): formats 1, 3 and 6; 3*4096+17, 4096, 100, 0 and
2*4096+5 points; differing scales and offsets, one of them anisotropic; and one file whose header bounds are tighter than its
points, so that the header early-out (last.rs:92-94) is observable.  The rasters lie over that test's boxes, cut to whole cells.
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _host  # noqa: E402
import _resident_files as rf  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

PCQ_ERR_PANIC, PCQ_ERR_UNSUPPORTED = pkg.PCQ_ERR_PANIC, pkg.PCQ_ERR_UNSUPPORTED
FILES = rf.FIVE_FILES
meets, world_box = rf.meets, rf.world_box
LYING = rf.LYING
BIG = 1e6
# (bmin, zmax, cell_size, nx, ny): every cell size is a whole number of lattice steps of every file
RASTERS = {"every": ((-BIG, -BIG, -BIG), BIG, 62500.0, 32, 32),        # meets every header
           "single": ((-20.0, -20.0, -5.0), 5.0, 0.5, 80, 80),          # a single file
           "missed": ((500.003, -260.0, -30.0), 40.0, 1.0, 100, 120),   # every header misses it; more than 8192 cells
           "slab": ((100.003, -300.0, -BIG), BIG, 0.1, 10, 2000),       # a thin slab of two files; more than 8192 cells
           "lie": ((320.0, -50.0, -10.0), 10.0, 0.25, 80, 400)}         # the lying file's points outside its header


class Q:
    def __init__(self):
        self.lib = _host.lib()

    err = staticmethod(_host.err)
    load = staticmethod(_host.load)
    bounds = staticmethod(_host.bounds)

    def raster(self, r, ras, sentinel=77, scanned=True):
        bmin, zmax, cell, nx, ny = ras
        words = np.arange(sentinel, sentinel + nx * ny, dtype=np.uint64)
        s = C.c_uint64(sentinel)
        rc = self.lib.pcq_query_resident_count_bounds_raster(r, (C.c_double * 3)(*bmin), zmax, cell, nx, ny,
                                                             words.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(s) if scanned else None)
        return rc, words.astype(np.int64).reshape(ny, nx), s.value


@pytest.fixture(scope="module")
def q():
    return Q()


def corpus(d):
    return rf.write_files(d, FILES, 950, LYING)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The files, and per file what tests/_resident_files.py holds of it."""
    return corpus(tmp_path_factory.mktemp("resident_raster"))


def numpy_raster(held, ras, header=True):
    """np.add.at over the files whose headers meet the raster's world box: the stored integers inside lmin .. lmin + n k - 1 on x and
    y (lmin from pcq_box_to_local, k the cell in the file's lattice steps) and inside the converted z range"""
    bmin, zmax, cell, nx, ny = ras
    box = world_box(ras)
    out = np.zeros((ny, nx), dtype=np.int64)
    for h in held:
        if (header and not meets(h, box)) or not len(h.xyz):
            continue
        lmin, lmax = pkg.box_to_local(list(box[0]), list(box[1]), list(h.scale), list(h.offset))
        k = [round(cell / h.scale[a]) for a in range(2)]
        assert all(abs(cell / h.scale[a] - k[a]) <= 1e-9 * k[a] for a in range(2))
        x = h.xyz.astype(np.int64)
        cx, cy = (x[:, 0] - lmin[0]) // k[0], (x[:, 1] - lmin[1]) // k[1]
        sel = (x[:, 0] >= lmin[0]) & (cx < nx) & (x[:, 1] >= lmin[1]) & (cy < ny) & (x[:, 2] >= lmin[2]) & (x[:, 2] <= lmax[2])
        np.add.at(out, (cy[sel], cx[sel]), 1)
    return out


@pytest.fixture(scope="module")
def dataset(q, files):
    r = q.load(files[0])
    yield r
    q.lib.pcq_query_resident_free(r)


@pytest.mark.parametrize("name", list(RASTERS))
def test_every_cell_is_numpy_on_the_files_integers(q, files, dataset, name):
    _, held = files
    ras = RASTERS[name]
    box = world_box(ras)
    rc, got, scanned = q.raster(dataset, ras)
    assert rc == 0, q.err()
    want = numpy_raster(held, ras)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in bad[:12]]
    rc, m, s = q.bounds(dataset, box)
    assert rc == 0 and s == scanned == sum(len(h.xyz) for h in held if meets(h, box))
    n = [len(h.xyz) for h in held]
    if name == "every":
        assert scanned == sum(n) and got.sum() == sum(n) and (got > 0).sum() > 1
    elif name == "single":
        assert scanned == n[1] and 0 < got.sum() < n[1] and (got > 0).sum() > 200
    elif name == "missed":
        assert scanned == 0 and got.sum() == 0
    elif name == "slab":
        assert scanned == n[0] + n[2] and 0 < got.sum() < scanned and (got > 0).sum() > 20
    else:  # the lying file: its points match in integer space, its header says no, and the header decides
        assert numpy_raster([held[LYING]], ras, header=False).sum() > 0
        assert not any(meets(f, box) for f in held) and scanned == 0 and got.sum() == 0


def test_a_raster_above_the_launch_limit_is_its_blocks(q, files, dataset):
    """96 x 96 cells (more than PCQ_RASTER_CELLS_MAX, so the entry tiles) against its nine 32 x 32 blocks asked one at a time"""
    _, held = files
    bmin, zmax, cell = (-24.0, -24.0, -5.0), 5.0, 0.5
    rc, whole, scanned = q.raster(dataset, (bmin, zmax, cell, 96, 96))
    assert rc == 0, q.err()
    assert np.array_equal(whole, numpy_raster(held, (bmin, zmax, cell, 96, 96)))
    assert scanned == len(held[1].xyz) and whole.sum() > 300
    for j in range(3):
        for i in range(3):
            sub = ((bmin[0] + 32 * i * cell, bmin[1] + 32 * j * cell, bmin[2]), zmax, cell, 32, 32)
            rc, block, _ = q.raster(dataset, sub)
            assert rc == 0, q.err()
            assert np.array_equal(block, whole[32 * j:32 * j + 32, 32 * i:32 * i + 32]), (i, j)


def test_points_scanned_may_be_null(q, dataset):
    rc, got, s = q.raster(dataset, RASTERS["single"], scanned=False)
    assert rc == 0 and s == 77 and got.sum() > 0


def test_a_cell_that_is_no_whole_step_is_unsupported(q, files, dataset):
    bmin, zmax, _, nx, ny = RASTERS["single"]
    for cell in (0.015, 0.5 + 1e-6, 0.001):  # 1.5 steps, 50.0001 steps, a tenth of a step of the file of scale 0.01
        rc, got, s = q.raster(dataset, (bmin, zmax, cell, 4, 4))
        assert rc == PCQ_ERR_UNSUPPORTED, (cell, rc, q.err())
        assert os.path.basename(files[0][1]).encode() in q.err()
        assert np.array_equal(got.reshape(-1), np.arange(77, 77 + 16)) and s == 77
    rc, got, _ = q.raster(dataset, RASTERS["single"])
    assert rc == 0 and got.sum() > 0


def test_a_box_that_panics_leaves_the_raster_untouched(q, dataset):
    bmin, _, cell, nx, ny = RASTERS["single"]
    rc, got, s = q.raster(dataset, (bmin, bmin[2] - 1.0, cell, 4, 4))
    assert rc == PCQ_ERR_PANIC and np.array_equal(got.reshape(-1), np.arange(77, 77 + 16)) and s == 77
    rc, got, _ = q.raster(dataset, RASTERS["single"])
    assert rc == 0 and got.sum() > 0
