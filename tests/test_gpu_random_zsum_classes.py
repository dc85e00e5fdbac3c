"""pcq_scan_dev_zsum_raster_batch_classes on drawn cases: 16 seeds (PCQ_TEST_SEED_BASE moves the whole range for a soak run), each
a random number of segments of random sizes up to a few thousand points (0, 1 and sizes around the 512-point step among them), a
random misalignment of every class block, a random raster of at most PCQ_ZSUM_CELLS_MAX cells with random cell widths per segment,
class bytes over all 256 values and a random set of 0 .. 256 classes.  Every word of both arrays, and the 64 behind the launch limit,
against numpy on int64 (tests/_zsum_classes.py).  draw(seed) is a pure function of BASE + PCQ_TEST_SEED_BASE + seed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _zsum_classes as zc  # noqa: E402

pytestmark = pytest.mark.gpu

SEED_BASE = int(os.environ.get("PCQ_TEST_SEED_BASE", "0"))  # a soak run: other seeds than the committed ones
BASE = 7100
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536)


def draw(seed):
    rng = np.random.default_rng(BASE + SEED_BASE + seed)
    S = int(rng.integers(1, 12))
    ns = [int(rng.choice(SIZES)) if rng.random() < 0.5 else int(rng.integers(0, 5000)) for _ in range(S)]
    mis = [int(m) for m in rng.integers(0, 16, S)]
    nx = int(rng.integers(1, 65))
    ny = int(rng.integers(1, zc.CELLS_MAX // nx + 1))
    cws = [(int(rng.integers(1, 700)), int(rng.integers(1, 700))) for _ in range(S)]
    nclasses = int(rng.choice([0, 1, 2, 255, 256, int(rng.integers(0, 257))]))
    classes = tuple(int(c) for c in rng.permutation(256)[:nclasses])
    xyz, cls = zc.draw(rng, ns, nx, ny, cws, classes=range(256), margin=3)
    zs = [(-2**40, 2**40) if rng.random() < 0.3 else None for _ in range(S)]
    boxes = [zc.box_of(k, nx, ny, cws[k], zs[k]) for k in range(S)]
    return ns, mis, nx, ny, cws, classes, xyz, cls, boxes


def test_draw_is_a_pure_function_of_the_seed():
    a, b = draw(3), draw(3)
    assert a[:6] == b[:6] and all(np.array_equal(x, y) for x, y in zip(a[6] + a[7], b[6] + b[7]))
    assert 1 <= a[2] * a[3] <= zc.CELLS_MAX


@pytest.mark.parametrize("seed", range(16))
def test_every_word_is_numpys(gpu_ctx, seed):
    ns, mis, nx, ny, cws, classes, xyz, cls, boxes = draw(seed)
    dev = zc.Dev(gpu_ctx, ns)
    try:
        dev.upload(xyz, cls, mis)
        try:
            dev.check(boxes, cws, nx, ny, classes)
            dev.check(boxes, cws, nx, ny, classes, pre=zc.ZEROS)
        except AssertionError as e:
            raise AssertionError(f"seed {seed} (PCQ_TEST_SEED_BASE {SEED_BASE}): n {ns}, class misalignments {mis}, {nx} x {ny} cells of {cws}, "
                                 f"{len(classes)} classes: {e}") from e
    finally:
        dev.free()
