"""host/resident.cpp: how rough is this box, cell by cell, from one pass over a dataset kept in HBM.
pcq_query_resident_bounds_zstd_raster (include/pcq_query_moments.h) must give, for every cell of the raster, the count and the mean of
pcq_query_resident_bounds_zmean_raster, bit for bit, and the population standard deviation of the world z that its header comment
DEFINES — restated in tests/_zmoments.py on python ints and floats, fed here with numpy's exact integers of every batch (count, sum
of the stored z, the two halves of the sum of their squares) and compared bit for bit.

Six small LAST files written through tests/_resident_files.py, on two z lattices that share cells: two files of z scale 0.05 and
offset 7.5 and two of scale 0.01 and offset 0, interleaved in load order so that each lattice's batch is gathered from files that
are not neighbours; one file without points; one file the box misses.  Every cell with points of both lattices runs the delta term
of the merge.  Rasters: 40 x 30 cells (more than PCQ_ZMOMENTS_CELLS_MAX: two blocks per batch), 8 x 8, and 40 x 30 fine cells in
which many cells hold a single point.  (Every file here is far below 2^32 points: a group is one batch.)

What turns it red: a block's words scattered to the wrong cells or arrays; groups merged in another order; the mean raster's W
changed; a sample (n - 1) deviation; any float operation of host/zmoments_merge.h reordered; an output written by a failing call.
"""
import ctypes as C
import importlib
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _host  # noqa: E402
import _resident_files as rf  # noqa: E402
import _zmoments as zm  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

PCQ_ERR_PANIC, PCQ_ERR_UNSUPPORTED = pkg.PCQ_ERR_PANIC, pkg.PCQ_ERR_UNSUPPORTED
ISO = rf.ISO
meets, world_box = rf.meets, rf.world_box
# (format, points, scale, offset); ints are x, y in [-5000, 5000), z in [-1000, 1000)
FILES = [(1, 4096 + 9, (0.01, 0.02, 0.05), (0.0, 0.0, 7.5)),      # x [-50, 50), y [-100, 100), z [-42.5, 57.5)
         (3, 700, ISO, (1.0, -1.0, 0.0)),                          # x [-49, 51), y [-51, 49), z [-10, 10)
         (1, 0, ISO, (0.0, 0.0, 0.0)),                             # no points
         (3, 2 * 4096, (0.02, 0.01, 0.05), (10.0, -10.0, 7.5)),    # x [-90, 110), y [-60, 40): the first file's z lattice
         (3, 500, ISO, (5000.0, 5000.0, 0.0)),                     # far away: every box here misses it
         (6, 3000, ISO, (5.0, 5.0, 0.0))]                          # x, y [-45, 55): the second file's z lattice
MISSED = 4
# (bmin, zmax, cell_size, nx, ny): every cell size is a whole number of lattice steps of every file
RASTERS = {"two blocks": ((-100.0, -75.0, -1e6), 1e6, 5.0, 40, 30),
           "8 x 8": ((-80.0, -80.0, -20.0), 30.0, 20.0, 8, 8),
           "fine": ((-10.0, -10.0, -1e6), 1e6, 0.5, 40, 30)}
SENTINEL = 77


def sentinels(n):
    a = np.arange(SENTINEL, SENTINEL + n, dtype=np.float64)
    return np.arange(SENTINEL, SENTINEL + n, dtype=np.uint64) * 3 + 1, -a - 0.25, a * 0.5 + 0.125


def untouched(count, mean, std, s):
    a, b, c = sentinels(count.size)
    return (np.array_equal(count.reshape(-1), a) and mean.reshape(-1).tobytes() == b.tobytes() and std.reshape(-1).tobytes() == c.tobytes()
            and s == SENTINEL)


class Q:
    def __init__(self):
        self.lib = _host.lib()

    err = staticmethod(_host.err)
    load = staticmethod(_host.load)

    def zstd(self, r, ras, scanned=True):
        bmin, zmax, cell, nx, ny = ras
        count, mean, std = sentinels(nx * ny)
        s = C.c_uint64(SENTINEL)
        dd = C.POINTER(C.c_double)
        rc = self.lib.pcq_query_resident_bounds_zstd_raster(r, (C.c_double * 3)(*bmin), zmax, cell, nx, ny, count.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                            mean.ctypes.data_as(dd), std.ctypes.data_as(dd), C.byref(s) if scanned else None)
        return rc, count, mean, std, s.value

    def zmean(self, r, ras):
        bmin, zmax, cell, nx, ny = ras
        count, mean, _ = sentinels(nx * ny)
        s = C.c_uint64(SENTINEL)
        rc = self.lib.pcq_query_resident_bounds_zmean_raster(r, (C.c_double * 3)(*bmin), zmax, cell, nx, ny, count.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                             mean.ctypes.data_as(C.POINTER(C.c_double)), C.byref(s))
        return rc, count, mean, s.value


@pytest.fixture(scope="module")
def q():
    return Q()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return rf.write_files(tmp_path_factory.mktemp("resident_zstd"), FILES, 2950)


@pytest.fixture(scope="module")
def dataset(q, files):
    r = q.load(files[0])
    yield r
    q.lib.pcq_query_resident_free(r)


restated = zm.restated


def check(q, r, held, ras, scanned=True):
    rc, count, mean, std, s = q.zstd(r, ras, scanned)
    assert rc == 0, q.err()
    want_cnt, want_mean, want_std, both, ngroups = restated(held, ras)
    assert np.array_equal(count, want_cnt)
    for name, got, want in (("zmean", mean, want_mean), ("zstd", std, want_std)):
        bad = np.flatnonzero(got.view(np.uint64) != want)
        assert len(bad) == 0, (name, [(int(c), float(got[c]), hex(int(want[c])), int(count[c])) for c in bad[:8]], len(bad))
    assert np.array_equal(np.isnan(std), count == 0) and np.array_equal(np.isnan(mean), count == 0)
    assert (std[count > 0] >= 0).all()
    want_scanned = sum(len(h.xyz) for h in held if meets(h, world_box(ras)))
    assert s == (want_scanned if scanned else SENTINEL)
    # count and zmean are the mean-height raster's, bit for bit, and so is points_scanned
    rc, c2, m2, s2 = q.zmean(r, ras)
    assert rc == 0 and np.array_equal(c2, count) and m2.tobytes() == mean.tobytes() and s2 == want_scanned
    return count.astype(np.int64), mean, std, both, ngroups


@pytest.mark.parametrize("name", list(RASTERS))
@pytest.mark.parametrize("scanned", [True, False])
def test_every_cell_is_the_definition(q, files, dataset, name, scanned):
    _, held = files
    ras = RASTERS[name]
    assert not meets(held[MISSED], world_box(ras)) and sum(meets(h, world_box(ras)) and len(h.xyz) > 0 for h in held) == 4
    cnt, mean, std, both, ngroups = check(q, dataset, held, ras, scanned)
    assert ngroups == 2 and both > {"two blocks": 300, "8 x 8": 20, "fine": 3}[name]  # cells in which the delta term runs
    if name == "two blocks":
        assert ras[3] * ras[4] > 1024 and (cnt[1024:] > 0).sum() > 50 and (cnt == 0).sum() > 50
    if name == "fine":  # a single point has no spread: exactly +0.0, not a rounding residue
        single = cnt == 1
        assert single.sum() > 100 and not std[single].view(np.uint64).any()
        assert (std[cnt > 1] > 0).sum() > 10
    # the spread is what numpy gives on the world heights, to rounding: the definition is not off by a factor
    world = np.concatenate([h.xyz[:, 2] * h.scale[2] + h.offset[2] for h in held if meets(h, world_box(ras))])
    assert 0 < np.nanmax(std) <= world.max() - world.min()


def test_a_raster_of_three_blocks_and_its_parts(q, files, dataset):
    """64 x 48 cells (three times PCQ_ZMOMENTS_CELLS_MAX: three launches per batch) and its 32 x 32 and 32 x 16 parts asked one at a
    time (one launch each), each against the definition.  (The parts are rasters of their own: the conversion of another world
    origin into an anisotropic file's lattice moves their cells against the whole's, so they are not compared with its slices.)"""
    _, held = files
    bmin, zmax, cell = (-64.0, -48.0, -1e6), 1e6, 2.0
    cnt, _, _, both, _ = check(q, dataset, held, (bmin, zmax, cell, 64, 48))
    assert both > 1000 and (cnt.reshape(48, 64)[32:] > 0).sum() > 500
    for j, h in ((0, 32), (32, 16)):
        for i in (0, 32):
            sub = ((bmin[0] + i * cell, bmin[1] + j * cell, bmin[2]), zmax, cell, 32, h)
            assert check(q, dataset, held, sub)[0].sum() > 500


def test_failures_leave_the_outputs_untouched(q, files, dataset):
    """bmin[2] > zmax panics; a cell size that is no whole number of a scanned file's lattice steps is unsupported and names the file;
    then the dataset still answers"""
    bmin, cell = (-20.0, -20.0, -5.0), 0.5  # (a corner inside the first file's header box: a raster of any cell size scans it)
    for scanned in (True, False):
        rc, count, mean, std, s = q.zstd(dataset, (bmin, bmin[2] - 1.0, cell, 4, 4), scanned)
        assert rc == PCQ_ERR_PANIC and untouched(count, mean, std, s)
        for bad in (0.015, 0.5 + 1e-6, 0.001):  # 1.5 steps, 50.0001 steps, a tenth of a step of a file of scale 0.01
            rc, count, mean, std, s = q.zstd(dataset, (bmin, 5.0, bad, 4, 4), scanned)
            assert rc == PCQ_ERR_UNSUPPORTED, (bad, rc, q.err())
            assert os.path.basename(files[0][0]).encode() in q.err() and untouched(count, mean, std, s)
    rc, count, _, _, _ = q.zstd(dataset, RASTERS["8 x 8"])
    assert rc == 0 and count.any()


@pytest.mark.parametrize("zscale", [float("inf"), 0.0])
def test_a_file_without_a_finite_z_scale_is_unsupported(q, tmp_path_factory, zscale):
    """raster_segments' z lattice rule, the mean-height raster's: a scanned file whose z scale (bytes 147 .. 154 of its header) is
    not finite or not above 0 is named, the outputs stay, and a raster whose world box its header misses is served"""
    d = tmp_path_factory.mktemp("resident_zstd_flat")
    paths, held = rf.write_files(d, [(3, 4096, ISO, (0.0, 0.0, 0.0)), (1, 600, ISO, (200.0, 0.0, 1.0))], 2970)
    img = held[1].image.copy()
    assert struct.unpack("<3d", img[131:155].tobytes()) == ISO
    img[147:155] = np.frombuffer(struct.pack("<d", zscale), dtype=np.uint8)
    img.tofile(paths[1])
    r = q.load(paths)
    try:
        rc, count, mean, std, s = q.zstd(r, ((-1e6, -1e6, -1e6), 1e6, 62500.0, 32, 32))
        assert rc == PCQ_ERR_UNSUPPORTED, (rc, q.err())
        assert os.path.basename(paths[1]).encode() in q.err() and untouched(count, mean, std, s)
        ras = ((-20.0, -20.0, -5.0), 5.0, 0.5, 32, 32)
        assert not meets(held[1], world_box(ras))
        cnt, _, _, both, ngroups = check(q, r, held, ras)
        assert ngroups == 1 and both == 0 and cnt.sum() > 20
    finally:
        q.lib.pcq_query_resident_free(r)
