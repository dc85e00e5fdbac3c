"""The height-spread raster on drawn cases: 16 seeds (PCQ_TEST_SEED_BASE moves the whole range for a soak run) of the device entry
and 16 of the resident entry.  Every seed draws from a generator of its own — (BASE + PCQ_TEST_SEED_BASE + seed, TAG) — so no other
random suite's cases move.

Device entry (pcq_scan_dev_zmoments_raster_batch): a random number of segments of random sizes up to a few thousand points (0, 1 and
sizes around the 512-point step among them), a random raster of at most PCQ_ZMOMENTS_CELLS_MAX cells with random cell widths per
segment, z over the whole i32 range with the i32 limits and +-65535, +-65536 planted.  Every word of the four arrays and the 64
behind the launch limit against numpy on int64, from the wrapping presets and from zeroed words.

Resident entry (pcq_query_resident_bounds_zstd_raster): 2 to 6 small LAST files (tests/_resident_files.py) of random formats, sizes
(0 among them), z scales and z offsets from a few values so that lattices repeat among files that are not neighbours, a raster of a
random shape (above PCQ_ZMOMENTS_CELLS_MAX in some cases) and cell size laid over the files' common ground.  count, zmean and zstd of
every cell bit for bit against tests/_zmoments.py on numpy's exact integers, and count and zmean against the mean-height raster.

What turns it red: what turns tests/test_gpu_zmoments_raster.py and tests/test_gpu_resident_zstd.py red, at shapes nobody chose.
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
import _zmoments as zm  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

TRIES = 60
SEED_BASE = int(os.environ.get("PCQ_TEST_SEED_BASE", "0"))  # a soak run: other seeds than the committed ones
BASE = 8300
DEV_TAG, RES_TAG = 0x7a6d6f, 0x7a7364  # ("zmo", "zsd") the second word of each generator's seed
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536)
Z_LATTICES = ((0.01, 0.0), (0.05, 7.5), (0.001, -2000.0), (0.25, 100.5))
XY_SCALES = (0.01, 0.02, 0.05)
CELL_SIZES = (0.5, 1.0, 2.0, 5.0, 20.0)
SHAPES = ((8, 8), (1, 1), (40, 30), (64, 17), (3, 5), (1025, 1), (1, 700), (33, 32))


def draw_device(seed):
    rng = np.random.default_rng([BASE + SEED_BASE + seed, DEV_TAG])
    S = int(rng.integers(1, 12))
    ns = [int(rng.choice(SIZES)) if rng.random() < 0.5 else int(rng.integers(0, 5000)) for _ in range(S)]
    nx = int(rng.integers(1, 65)) if rng.random() < 0.8 else int(rng.choice([1, zm.CELLS_MAX]))
    ny = int(rng.integers(1, zm.CELLS_MAX // nx + 1))
    cws = [(int(rng.integers(1, 700)), int(rng.integers(1, 700))) for _ in range(S)]
    xyz = zm.draw(rng, nx, ny, cws, margin=3, ns=ns)
    for a in xyz:
        if len(a):
            at = rng.integers(0, len(a), 6)
            a[at, 2] = rng.choice(zm.PLANTED, 6)
    zs = [(-2**40, 2**40) if rng.random() < 0.3 else None for _ in range(S)]
    boxes = [zm.box_of(k, nx, ny, cws[k], zs[k]) for k in range(S)]
    return ns, nx, ny, cws, xyz, boxes


def draw_resident(seed):
    """(file specs for _resident_files.write_files, its seed, raster): ints are x, y in [-5000, 5000), z in [-1000, 1000)"""
    rng = np.random.default_rng([BASE + SEED_BASE + seed, RES_TAG])
    specs = []
    for _ in range(int(rng.integers(2, 7))):
        zl = Z_LATTICES[int(rng.integers(0, len(Z_LATTICES) if rng.random() < 0.5 else 2))]
        scale = (float(rng.choice(XY_SCALES)), float(rng.choice(XY_SCALES)), zl[0])
        offset = (float(rng.integers(-3, 4)) * 10.0, float(rng.integers(-3, 4)) * 10.0, zl[1])
        n = int(rng.choice([0, 1, 700, 4096, 4096 + 9, 9000]))
        specs.append((int(rng.choice([1, 3, 6])), n, scale, offset))
    for _ in range(TRIES):  # a raster the entry accepts: the world box converts into every file's lattice (pcq_box_to_local)
        nx, ny = SHAPES[int(rng.integers(0, len(SHAPES)))]
        cell = float(rng.choice(CELL_SIZES))
        zfaces = (-1e6, 1e6) if rng.random() < 0.5 else (float(rng.integers(-30, 0)), float(rng.integers(1, 40)))
        bmin = (-float(rng.integers(0, nx + 1)) * cell * 0.5, -float(rng.integers(0, ny + 1)) * cell * 0.5, zfaces[0])
        ras = (bmin, zfaces[1], cell, nx, ny)
        box = rf.world_box(ras)
        try:
            for _, _, scale, offset in specs:
                pkg.box_to_local(list(box[0]), list(box[1]), list(scale), list(offset))
        except binding.PcqError:
            continue
        return specs, 3000 + 10 * seed, ras
    raise AssertionError(f"seed {seed}: no accepted raster in {TRIES} tries")


def test_draws_are_pure_functions_of_the_seed():
    a, b = draw_device(3), draw_device(3)
    assert a[:4] == b[:4] and all(np.array_equal(x, y) for x, y in zip(a[4], b[4])) and a[5] == b[5]
    assert 1 <= a[1] * a[2] <= zm.CELLS_MAX
    assert draw_resident(5) == draw_resident(5) and draw_resident(5) != draw_resident(6)


@pytest.mark.parametrize("seed", range(16))
def test_device_entry(gpu_ctx, seed):
    ns, nx, ny, cws, xyz, boxes = draw_device(seed)
    dev = zm.Dev(gpu_ctx, ns)
    try:
        dev.upload(xyz)
        try:
            dev.check(boxes, cws, nx, ny)
            dev.check(boxes, cws, nx, ny, pre=zm.ZEROS)
        except AssertionError as e:
            raise AssertionError(f"seed {seed} (PCQ_TEST_SEED_BASE {SEED_BASE}): n {ns}, {nx} x {ny} cells of {cws}: {e}") from e
    finally:
        dev.free()


@pytest.mark.parametrize("seed", range(16))
def test_resident_entry(tmp_path, seed):
    specs, file_seed, ras = draw_resident(seed)
    paths, held = rf.write_files(tmp_path, specs, file_seed)
    lib = _host.lib()
    r = _host.load(paths)
    try:
        bmin, zmax, cell, nx, ny = ras
        n = nx * ny
        count, mean, std = np.full(n, 7, dtype=np.uint64), np.full(n, -1.5), np.full(n, -2.5)
        count2, mean2 = count.copy(), mean.copy()
        s, s2 = C.c_uint64(7), C.c_uint64(7)
        pu, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
        b3 = (C.c_double * 3)(*bmin)
        rc = lib.pcq_query_resident_bounds_zstd_raster(r, b3, zmax, cell, nx, ny, count.ctypes.data_as(pu), mean.ctypes.data_as(pd),
                                                       std.ctypes.data_as(pd), C.byref(s))
        where = f"seed {seed} (PCQ_TEST_SEED_BASE {SEED_BASE}): files {specs}, raster {ras}"
        assert rc == 0, (where, _host.err())
        want_cnt, want_mean, want_std, _, _ = zm.restated(held, ras)
        assert np.array_equal(count, want_cnt), where
        assert np.array_equal(mean.view(np.uint64), want_mean), where
        bad = np.flatnonzero(std.view(np.uint64) != want_std)
        assert len(bad) == 0, (where, [(int(c), float(std[c]), int(count[c])) for c in bad[:8]])
        assert s.value == sum(len(h.xyz) for h in held if rf.meets(h, rf.world_box(ras))), where
        rc = lib.pcq_query_resident_bounds_zmean_raster(r, b3, zmax, cell, nx, ny, count2.ctypes.data_as(pu), mean2.ctypes.data_as(pd), C.byref(s2))
        assert rc == 0 and np.array_equal(count2, count) and mean2.tobytes() == mean.tobytes() and s2.value == s.value, where
    finally:
        _host.free(r)
