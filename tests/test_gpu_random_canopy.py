"""The canopy-height raster on drawn cases: 16 seeds of the device entry and 16 of the resident entry (PCQ_TEST_SEED_BASE moves both
ranges for a soak run).

Device: a random number of segments of random sizes up to a few thousand points (0, 1 and sizes around the 512-point step among
them), a random misalignment of every class block, a random raster of at most PCQ_ZRANGE_CLASSES_CELLS_MAX cells with random cell
widths per segment, class bytes over all 256 values and two random sets of 0 .. 256 classes drawn independently; every word of both
arrays, and the 64 behind the launch limit, against numpy (tests/_canopy.py), from presets that are no sentinels and from the sentinels.

Resident: two to five small LAST files of random sizes on one to three z lattices, a random raster of 1 .. 9000 cells over them, two
random sets of the classes the files hold; zground, zsurface and height against the header's definition in numpy, bit for bit.
draw_*(seed) are pure functions of their BASE + PCQ_TEST_SEED_BASE + seed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _canopy as cn  # noqa: E402
import _host  # noqa: E402
import _resident_files as rf  # noqa: E402

pytestmark = pytest.mark.gpu

SEED_BASE = int(os.environ.get("PCQ_TEST_SEED_BASE", "0"))  # a soak run: other seeds than the committed ones
BASE, HOST_BASE = 7300, 7400
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536)
FILE_CLASSES = (1, 2, 5, 7, 9, 18, 64, 200, 255)
LATTICES = ((0.01, 0.0), (0.05, 7.5), (0.001, -3.0))  # (scale[2], offset[2])


def draw_set(rng, universe=range(256)):
    universe = list(universe)
    n = int(rng.choice([0, 1, 2, len(universe) - 1, len(universe), int(rng.integers(0, len(universe) + 1))]))
    return tuple(int(universe[i]) for i in rng.permutation(len(universe))[:n])


def draw_device(seed):
    rng = np.random.default_rng(BASE + SEED_BASE + seed)
    S = int(rng.integers(1, 12))
    ns = [int(rng.choice(SIZES)) if rng.random() < 0.5 else int(rng.integers(0, 5000)) for _ in range(S)]
    mis = [int(m) for m in rng.integers(0, 16, S)]
    nx = int(rng.integers(1, 65))
    ny = int(rng.integers(1, cn.CELLS_MAX // nx + 1))
    cws = [(int(rng.integers(1, 700)), int(rng.integers(1, 700))) for _ in range(S)]
    low, high = draw_set(rng), draw_set(rng)
    xyz, cls = cn.draw(rng, ns, nx, ny, cws, classes=range(256), margin=3)
    zs = [(-2**40, 2**40) if rng.random() < 0.3 else None for _ in range(S)]
    boxes = [cn.box_of(k, nx, ny, cws[k], zs[k]) for k in range(S)]
    return ns, mis, nx, ny, cws, low, high, xyz, cls, boxes


def draw_host(seed):
    """(file specs, the writer's seed, raster, low, high)"""
    rng = np.random.default_rng(HOST_BASE + SEED_BASE + seed)
    specs = []
    for _ in range(int(rng.integers(2, 6))):
        sz, oz = LATTICES[int(rng.integers(0, len(LATTICES)))]
        n = int(rng.choice([0, 1, 511, 513, 4096])) if rng.random() < 0.3 else int(rng.integers(1, 9000))
        specs.append((int(rng.choice([1, 3, 6])), n, (0.01, 0.01, sz), (float(rng.integers(-3, 4)) * 10.0, float(rng.integers(-3, 4)) * 10.0, oz)))
    cell = float(rng.choice([0.25, 0.5, 1.0, 2.0, 10.0]))  # whole numbers of steps of 0.01
    nx = int(rng.integers(1, 120))
    ny = int(rng.integers(1, 9000 // nx + 1))
    bmin = (float(rng.integers(-80, 40)), float(rng.integers(-80, 40)), float(rng.choice([-1e6, -5.0, 0.0])))
    zmax = float(rng.choice([1e6, 5.0, 20.0]))
    return specs, 8000 + 16 * seed, (bmin, zmax, cell, nx, ny), draw_set(rng, FILE_CLASSES), draw_set(rng, FILE_CLASSES)


def test_draws_are_pure_functions_of_the_seed():
    a, b = draw_device(3), draw_device(3)
    assert a[:7] == b[:7] and all(np.array_equal(x, y) for x, y in zip(a[7] + a[8], b[7] + b[8]))
    assert 1 <= a[2] * a[3] <= cn.CELLS_MAX
    assert draw_host(5) == draw_host(5) and draw_host(5) != draw_host(6)
    kinds = [(bool(d[5]), bool(d[6]), d[5] == d[6]) for d in map(draw_device, range(16))]
    assert (True, True, False) in kinds  # two non-empty sets that differ are among the committed seeds


@pytest.mark.parametrize("seed", range(16))
def test_device_every_word_is_numpys(gpu_ctx, seed):
    ns, mis, nx, ny, cws, low, high, xyz, cls, boxes = draw_device(seed)
    dev = cn.Dev(gpu_ctx, ns)
    try:
        dev.upload(xyz, cls, mis)
        try:
            dev.check(boxes, cws, nx, ny, low, high)
            dev.check(boxes, cws, nx, ny, low, high, pre=cn.SENT)
        except AssertionError as e:
            raise AssertionError(f"seed {seed} (PCQ_TEST_SEED_BASE {SEED_BASE}): n {ns}, class misalignments {mis}, {nx} x {ny} cells of {cws}, "
                                 f"{len(low)} low and {len(high)} high classes: {e}") from e
    finally:
        dev.free()


@pytest.mark.parametrize("seed", range(16))
def test_resident_every_cell_is_the_definition(tmp_path, seed):
    specs, wseed, ras, low, high = draw_host(seed)
    paths, held = rf.write_files(tmp_path, specs, wseed, classes=FILE_CLASSES)
    lib = _host.lib()
    r = _host.load(paths)
    try:
        wg, ws, wh = cn.numpy_canopy(held, ras, low, high)
        rc, zg, zs, h, scanned = cn.host_canopy(lib, r, ras, low, high)
        assert rc == 0, (seed, _host.err())
        assert scanned == sum(len(f.xyz) for f in held if rf.meets(f, rf.world_box(ras)))
        for what, got, want in (("zground", zg, wg), ("zsurface", zs, ws), ("height", h, wh)):
            bad = np.argwhere((np.isnan(got) != np.isnan(want)) | (~np.isnan(want) & (got.view(np.uint64) != want.view(np.uint64))))
            assert len(bad) == 0, (f"seed {seed} (PCQ_TEST_SEED_BASE {SEED_BASE}): {specs}, raster {ras}, low {low}, high {high}: {what}",
                                   [(int(y), int(x), float(got[y, x]), float(want[y, x])) for y, x in bad[:8]])
    finally:
        _host.free(r)
