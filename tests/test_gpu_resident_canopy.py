"""host/resident.cpp: how high above the ground is this box, cell by cell, from one pass over a dataset kept in HBM.
pcq_query_resident_bounds_canopy_raster (include/pcq_query_canopy.h) must give, for every cell of the raster, the zground, zsurface
and height its header comment DEFINES, restated in numpy on int64 / float64 over Held.xyz / Held.cls (tests/_canopy.py: numpy_canopy)
and compared bit for bit; both sets full bit for bit with pcq_query_resident_bounds_zrange_raster; points_scanned with that entry's.

The five small LAST files of tests/_resident_files.py (FIVE_FILES: three z lattices, a file without points, a file whose header lies)
with class bytes drawn from (2, 5, 7, 9, 18, 200), and a sixth file on the second file's z lattice whose classes are (5, 200) only: a
file without a point of the ground set.  Rasters inside one block of 4096 cells and of several blocks, one that every header misses.
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _canopy as cn  # noqa: E402
import _host  # noqa: E402
import _resident_files as rf  # noqa: E402
import _time_images as ti  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

PCQ_ERR_ARG, PCQ_ERR_PANIC, PCQ_ERR_UNSUPPORTED = pkg.PCQ_ERR_ARG, pkg.PCQ_ERR_PANIC, pkg.PCQ_ERR_UNSUPPORTED
BIG = 1e6
CLASSES = (2, 5, 7, 9, 18, 200)
NO_GROUND = (3, 2048 + 9, rf.ISO, (20.0, 10.0, 0.0))  # x [-30, 70), y [-40, 60): over the second file, on its z lattice
# (bmin, zmax, cell_size, nx, ny)
RASTERS = {"every": ((-BIG, -BIG, -BIG), BIG, 62500.0, 32, 32),        # meets every header; one block
           "single": ((-20.0, -20.0, -5.0), 5.0, 0.5, 80, 80),          # the second and the sixth file; 6400 cells: two blocks
           "missed": ((500.003, -260.0, -30.0), 40.0, 1.0, 100, 120),   # every header misses it
           "slab": ((100.003, -300.0, -BIG), BIG, 0.1, 10, 2000),       # a thin slab of two files of two lattices; five blocks, rows of 10
           "fine": ((-30.0, -40.0, -BIG), BIG, 2.0, 50, 50)}            # the second and the sixth file whole; 2500 cells: one block
MATCHING = ("every", "single", "slab", "fine")
SETS = {"canopy": ((2,), cn.BUT_7_18), "equal": ((2, 9), (2, 9)), "swapped": (cn.BUT_7_18, (2,)), "no-ground": ((), (5, 200)),
        "no-surface": ((2,), ()), "none": ((), ()), "full": (cn.ALL, cn.ALL)}


@pytest.fixture(scope="module")
def lib():
    return _host.lib()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    paths, held = rf.write_files(tmp_path_factory.mktemp("resident_canopy"), rf.FIVE_FILES, 2950, rf.LYING, classes=CLASSES)
    more, held6 = rf.write_files(tmp_path_factory.mktemp("resident_canopy_no_ground"), [NO_GROUND], 2960, classes=(5, 200))
    return paths + more, held + held6


@pytest.fixture(scope="module")
def dataset(files):
    r = _host.load(files[0])
    yield r
    _host.free(r)


def zrange(lib, r, ras):
    bmin, zmax, cell, nx, ny = ras
    lo, hi = np.full(nx * ny, -1.5), np.full(nx * ny, -2.5)
    s = C.c_uint64(5)
    pd = C.POINTER(C.c_double)
    rc = lib.pcq_query_resident_bounds_zrange_raster(r, (C.c_double * 3)(*bmin), zmax, cell, nx, ny, lo.ctypes.data_as(pd), hi.ctypes.data_as(pd), C.byref(s))
    return rc, lo.reshape(ny, nx), hi.reshape(ny, nx), s.value


def test_the_corpus_has_what_the_tests_need(files):
    """On the CPU, before anything runs on the GPU"""
    _, held = files
    assert not cn.in_set(held[5].cls, (2, 9)).any() and len(held[3].xyz) == 0
    for name in MATCHING:
        g, s, h = cn.numpy_canopy(held, RASTERS[name], *SETS["canopy"])
        assert (~np.isnan(h)).sum() > (10 if name in ("single", "fine") else 0), name
        assert name not in ("single", "fine") or (np.isnan(g) & ~np.isnan(s)).any(), name  # a cell with a surface and no ground
        g2, s2, _ = cn.numpy_canopy(held, RASTERS[name], *SETS["swapped"])
        assert not cn.same_bits(g, g2) and not cn.same_bits(s, s2), name
    assert np.isnan(cn.numpy_canopy(held, RASTERS["missed"], *SETS["full"])[2]).all()
    g, s, _ = cn.numpy_canopy(held, RASTERS["single"], *SETS["canopy"])
    only6 = cn.numpy_canopy([held[5]], RASTERS["single"], *SETS["canopy"])
    assert np.isnan(only6[0]).all() and (~np.isnan(only6[1])).any()  # the sixth file gives surface and no ground


@pytest.mark.parametrize("key", list(SETS))
@pytest.mark.parametrize("name", list(RASTERS))
def test_every_cell_is_the_definition_in_numpy(lib, files, dataset, name, key):
    _, held = files
    ras, (low, high) = RASTERS[name], SETS[key]
    wg, ws, wh = cn.numpy_canopy(held, ras, low, high)
    rc, zg, zs, h, scanned = cn.host_canopy(lib, dataset, ras, low, high)
    assert rc == 0, _host.err()
    for what, got, want in (("zground", zg, wg), ("zsurface", zs, ws), ("height", h, wh)):
        # (NaN where numpy's is NaN, whatever its payload; every other word bit for bit)
        bad = np.argwhere((np.isnan(got) != np.isnan(want)) | (~np.isnan(want) & (got.view(np.uint64) != want.view(np.uint64))))
        assert len(bad) == 0, (what, [(int(y), int(x), float(got[y, x]), float(want[y, x])) for y, x in bad[:8]])
    assert np.array_equal(np.isnan(h), np.isnan(zg) | np.isnan(zs))
    rc, lo, hi, s = zrange(lib, dataset, ras)
    assert rc == 0 and s == scanned == sum(len(f.xyz) for f in held if rf.meets(f, rf.world_box(ras)))  # whatever the classes
    if key == "full":  # bit for bit the unfiltered entry
        assert cn.same_bits(lo, zg) and cn.same_bits(hi, zs)
    if key == "none":
        assert np.isnan(zg).all() and np.isnan(zs).all() and np.isnan(h).all()
    if key == "no-ground":
        assert np.isnan(zg).all() and np.isnan(h).all() and (name == "missed" or (~np.isnan(zs)).any())
    if key == "no-surface":
        assert np.isnan(zs).all() and np.isnan(h).all() and (name == "missed" or (~np.isnan(zg)).any())


def test_height_and_points_scanned_may_be_null(lib, dataset):
    rc, zg, zs, h, s = cn.host_canopy(lib, dataset, RASTERS["single"], *SETS["canopy"], height=False, scanned=False)
    assert rc == 0 and s == 77 and (h == 11.0).all() and (~np.isnan(zg)).sum() > 30 and (~np.isnan(zs)).sum() > 100


def test_the_sentinel_rule(lib, tmp_path_factory):
    """A ground point stored at exactly Z = INT32_MAX reads as no point, and so does a surface point at INT32_MIN; at the other end of
    the range each is an ordinary value.  One file of ten points in four cells of a 4 x 1 raster, ground {2}, surface {5}."""
    I32_MIN, I32_MAX = cn.I32_MIN, cn.I32_MAX
    pts = [(50, 2, I32_MAX), (50, 5, 100),        # cell 0: the only ground point is at the sentinel: no ground; a surface
           (150, 5, I32_MIN), (150, 2, -50),      # cell 1: the only surface point is at its sentinel: no surface; a ground
           (250, 2, I32_MAX), (250, 2, 7), (250, 5, I32_MIN), (250, 5, 9),  # cell 2: each sentinel beside an ordinary value, which wins
           (350, 5, I32_MAX), (350, 2, I32_MIN)]  # cell 3: the extremes the other way round are values
    n = len(pts)
    xyz = np.asarray([(x, 50, z) for x, _, z in pts], dtype=np.int32)
    cls = np.asarray([c for _, c, _ in pts], dtype=np.uint8)
    _, _, rgb, t = ti.points(n, 2970)
    img = ti.last_image(3, xyz, cls, rgb, t, scale=rf.ISO, offset=(0.0, 0.0, 0.0)).copy()
    w = ti.world(xyz, rf.ISO, (0.0, 0.0, 0.0))
    p = str(tmp_path_factory.mktemp("resident_canopy_sentinels") / "sentinels.last")
    img.tofile(p)
    held = [rf.Held(xyz, cls, t, rf.ISO, (0.0, 0.0, 0.0), w.min(axis=0), w.max(axis=0), img)]
    ras = ((0.0, 0.0, -1e9), 1e9, 1.0, 4, 1)
    r = _host.load([p])
    try:
        rc, zg, zs, h, s = cn.host_canopy(lib, r, ras, (2,), (5,))
        assert rc == 0 and s == n, _host.err()
        wg, ws, wh = cn.numpy_canopy(held, ras, (2,), (5,))
        for got, want in ((zg, wg), (zs, ws), (h, wh)):
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
        assert np.isnan(zg[0, 0]) and zs[0, 0] == 1.0 and np.isnan(h[0, 0])
        assert zg[0, 1] == -0.5 and np.isnan(zs[0, 1]) and np.isnan(h[0, 1])
        assert zg[0, 2] == 7 * 0.01 and zs[0, 2] == 9 * 0.01 and h[0, 2] == 9 * 0.01 - 7 * 0.01
        assert zg[0, 3] == I32_MIN * 0.01 and zs[0, 3] == I32_MAX * 0.01 and h[0, 3] == I32_MAX * 0.01 - I32_MIN * 0.01
    finally:
        _host.free(r)


@pytest.mark.parametrize("key", ["canopy", "none"])
def test_refusals_leave_the_outputs_untouched(lib, files, dataset, key):
    """a null set, PCQ_ERR_PANIC and the PCQ_ERR_UNSUPPORTED of a cell that is no whole lattice step, also for the empty sets"""
    low, high = SETS[key]
    bmin, zmax, cell, nx, ny = RASTERS["single"]
    for sets in ((None, high), (low, None)):
        rc, zg, zs, h, s = cn.host_canopy(lib, dataset, RASTERS["single"], *sets)
        assert rc == PCQ_ERR_ARG and cn.host_untouched(zg, zs, h, s)
    rc, zg, zs, h, s = cn.host_canopy(lib, dataset, (bmin, bmin[2] - 1.0, cell, 4, 4), low, high)
    assert rc == PCQ_ERR_PANIC and cn.host_untouched(zg, zs, h, s)
    for bad in (0.015, 0.5 + 1e-6, 0.001):  # 1.5 steps, 50.0001 steps, a tenth of a step of the file of scale 0.01
        rc, zg, zs, h, s = cn.host_canopy(lib, dataset, (bmin, zmax, bad, 4, 4), low, high)
        assert rc == PCQ_ERR_UNSUPPORTED, (bad, rc, _host.err())
        assert os.path.basename(files[0][1]).encode() in _host.err()
        assert cn.host_untouched(zg, zs, h, s)
    rc, zg, _, _, _ = cn.host_canopy(lib, dataset, RASTERS["single"], *SETS["canopy"])
    assert rc == 0 and (~np.isnan(zg)).any()


@pytest.mark.parametrize("key", ["canopy", "none"])
def test_a_file_without_a_z_scale_is_unsupported(lib, tmp_path_factory, key):
    """scale[2] = 0: the file is named and the outputs stay, also for the empty sets"""
    d = tmp_path_factory.mktemp("resident_canopy_flat_" + key)
    paths, _ = rf.write_files(d, [(3, 4096, rf.ISO, (0.0, 0.0, 0.0)), (1, 600, (0.01, 0.01, 0.0), (200.0, 0.0, 1.0))], 2980, classes=CLASSES)
    r = _host.load(paths)
    try:
        rc, zg, zs, h, s = cn.host_canopy(lib, r, ((-BIG, -BIG, -BIG), BIG, 62500.0, 32, 32), *SETS[key])
        assert rc == PCQ_ERR_UNSUPPORTED, (rc, _host.err())
        assert os.path.basename(paths[1]).encode() in _host.err() and cn.host_untouched(zg, zs, h, s)
    finally:
        _host.free(r)
