"""pcq_scan_dev_zmoments_raster_batch: the count, the z sum and the two halves of the sum of z squared per cell of a box over many
resident segments in one pass, every word against numpy on int64 (whose adds wrap modulo 2^64 as the entry's do).

Segments of n = 0, 1, 511, 512, 513, 1535, 4133 points, the sizes of test_gpu_zsum_raster.py (a step of the pipeline is 512
points), positions pieces 16-byte aligned in one buffer.  Every segment has its own origin, its own box and its own cell widths; x,
y and z are drawn independently, so a z taken from the wrong lane or load is another point's.  Every case uploads the positions it
needs.  The call ADDS: every call starts from preset words, PCQ_ZMOMENTS_CELLS_MAX of each of the four arrays and 64 guard words
behind them — counts of 0, 2^32 - 1 and 2^40 + c, sums of 0, -1, 2^62 and -2^62 + c, low words of 0, 2^32 - 1 and 2^33 + c and,
in every other cell that receives a point whose z^2 mod 2^32 is not 0, of 2^64 - 1 (so that the word wraps), high words of 2^32 - 1,
2^64 - 1 - c and 0 — and the test compares all of them with np.add.at of the points pp.in_box keeps into a copy of the presets: the
raster's words grown, the 64 behind them as they were.

What turns it red: a square formed in 32 bits, a low or high half added in 32 bits, a z zero-extended, the halves swapped, a slice
of the partials written or folded at another array's offset, a word touched at or beyond nx * ny, a refusal that writes.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

import _zmoments as zm  # noqa: E402
from _zmoments import CELLS_MAX, EMPTY, I32_MAX, I32_MIN, NAMES, NS, PLANTED, PRE, WORDS, ZEROS, Dev, box_of, draw, four, origin  # noqa: E402,F401

PCQ_ERR_ARG = pkg.PCQ_ERR_ARG


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    d = Dev(gpu_ctx)
    yield d
    d.free()


@pytest.mark.parametrize("k", [3, 4, 5])
def test_one_point_per_cell(dev, k):
    """(a) 32 x 32 = PCQ_ZMOMENTS_CELLS_MAX cells of width 1, a single segment of 512, 513 or 1535 points, point p in cell p (modulo
    1024: the longest segment goes round once, so its first 511 cells hold two points) with a z of its own over the whole i32 range
    and the planted values at points 85 and 170 of both tiles, next to them, and in the leftovers: every position of a step, both
    tiles, the leftover loop.  From zeroed words each array is read back as numpy's four words of that z."""
    n, nx, ny = NS[k], 32, 32
    ox, oy = origin(k)
    rng = np.random.default_rng(1900 + k)
    z = rng.integers(I32_MIN, I32_MAX + 1, n)
    at = [85, 170, 256 + 85, 256 + 170, 0, 63, 64, 255, 256, 511] + ([n - 1] if n > 512 else [])
    for i, p in enumerate(at):
        z[p] = PLANTED[i % len(PLANTED)]
    z[n - 1 - np.arange(len(PLANTED))] = PLANTED  # (and all of them at the segment's end)
    assert set(PLANTED) <= set(z.tolist())
    xyz = [np.full((m, 3), -10**6, dtype=np.int32) for m in NS]
    p = np.arange(n) % 1024
    xyz[k] = np.stack([ox + p % 32, oy + p // 32, z], axis=1).astype(np.int32)
    dev.upload(xyz)
    for zlo, zhi in ((-2**40, 2**40), (I32_MIN, I32_MAX)):  # ... and the i32 limits as the box's z faces: the same answer
        box = ([ox, oy, zlo], [ox + 31, oy + 31, zhi])
        added = dev.check([box], [(1, 1)], nx, ny, [k], pre=ZEROS)
        cnt = np.bincount(p, minlength=1024)
        assert np.array_equal(added[0], cnt) and cnt.max() == (2 if n > 1024 else 1)
        if n <= 1024:
            z64 = z.astype(np.int64)
            got = dev.words()
            for g, v in zip(got, four(z64)):
                assert np.array_equal(g[:n], v) and not g[n:].any()
            assert np.array_equal(got[3][:n] * 2**32 + got[2][:n], z64 * z64)
    dev.check([box], [(1, 1)], nx, ny, [k])  # (the same into the presets: a carry per word, the low words wrapping)
    assert dev.wraps > 200


@pytest.mark.parametrize("name", ["65535", "min", "max", "alternating"])
def test_every_point_in_one_cell(dev, name):
    """(b) A 1 x 1 raster over every segment: all 64 lanes of every slot add into one LDS word of each array.  All z = 65535: z^2 =
    2^32 - 131071 has no high half and the low word passes 2^32 at the second point, so a 32-bit low add is seen.  All INT32_MIN:
    2^30 into the high word per point and nothing into the low one.  All INT32_MAX.  Alternating INT32_MAX and INT32_MIN.  From
    zeroed words, then from each of the presets in word 0."""
    total = sum(NS)
    zs = {"65535": lambda n: np.full(n, 65535), "min": lambda n: np.full(n, I32_MIN), "max": lambda n: np.full(n, I32_MAX),
          "alternating": lambda n: np.where(np.arange(n) % 2 == 0, I32_MAX, I32_MIN)}[name]
    rng = np.random.default_rng(1910)
    xyz, boxes = [], []
    for k, n in enumerate(NS):
        ox, oy = origin(k)
        xyz.append(np.stack([ox + rng.integers(0, 9, n), oy + rng.integers(0, 9, n), zs(n)], axis=1).astype(np.int32))
        boxes.append(([ox, oy, I32_MIN], [ox + 8, oy + 8, I32_MAX]))
    dev.upload(xyz)
    cws = [(9, 9)] * len(NS)
    for pre in [ZEROS, None] + [tuple(np.roll(p, -s) for p in PRE) for s in range(1, 4)]:
        added = dev.check(boxes, cws, 1, 1, pre=pre)
        assert added[0][0] == total
        if name == "65535":
            assert added[1][0] == 65535 * total and added[2][0] == total * (2**32 - 131071) > 2**44 and added[3][0] == 0
        if name == "min":
            assert added[1][0] == -2**31 * total and added[2][0] == 0 and added[3][0] == total * 2**30


@pytest.mark.parametrize("nx,ny", [(1, 1), (8, 8), (37, 27), (1024, 1)])
def test_random_segments(dev, nx, ny):
    """(c) Random segments with their own origins and cell widths, x, y and z independent; the z slab keeps about half the points,
    and dropping it changes the words of many cells"""
    cws = [(2 + k, 9 - k) for k in range(len(NS))] if nx * ny < 999 else [(1 + k % 3, 40 + k) for k in range(len(NS))]
    dev.upload(draw(np.random.default_rng(152 + nx + 100 * ny), nx, ny, cws))
    boxes = [box_of(k, nx, ny, cws[k]) for k in range(len(NS))]
    added = dev.check(boxes, cws, nx, ny)
    # (about half the points of the raster's ground; on a raster of a few lattice steps most points lie in the margin around it)
    assert (sum(NS) // 4 if nx * ny >= 64 else 500) < added[0].sum() < 2 * sum(NS) // 3 and (added[0] > 0).sum() >= min(nx * ny, 900)
    assert dev.wraps >= min(nx * ny, 900) // 2
    every = [([lo[0], lo[1], -2**40], [hi[0], hi[1], 2**40]) for lo, hi in boxes]
    more = dev.check(every, cws, nx, ny)
    assert more[0].sum() > added[0].sum() and (more[3] != added[3]).sum() >= min(nx * ny, 600)


@pytest.mark.parametrize("nx,ny", [(8, 8), (37, 27)])
def test_counts_and_sums_are_the_mean_height_rasters(dev, nx, ny):
    """(d) device_count and device_zsum receive exactly what pcq_scan_dev_zsum_raster_batch adds for the same call"""
    cws = [(2 + k, 9 - k) for k in range(len(NS))]
    dev.upload(draw(np.random.default_rng(152 + nx + 100 * ny), nx, ny, cws))
    boxes = [box_of(k, nx, ny, cws[k]) for k in range(len(NS))]
    added = dev.check(boxes, cws, nx, ny)
    got = dev.words()
    for d, p in zip(dev.d_zsum_words, dev.pre[:2]):
        dev.ctx.to_device(d, np.ascontiguousarray(p, dtype=np.int64))
    dev.ctx.scan_dev_zsum_raster_batch(dev.cols, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], cws, nx, ny, *dev.d_zsum_words)
    other = dev.words(dev.d_zsum_words)
    assert np.array_equal(other[0], got[0]) and np.array_equal(other[1], got[1]) and added[0].sum() > 1000


def test_a_subset_of_segments_and_a_callers_stream(dev):
    """(e) Segments 6, 2 and 4 alone, in that order, on the context's stream and on a caller's; the caller orders its outputs"""
    import torch
    nx, ny = 16, 16
    n = len(NS)
    cws = [(3 + k, 4) for k in range(n)]
    dev.upload(draw(np.random.default_rng(156), nx, ny, cws))
    some = [6, 2, 4]
    boxes = [box_of(k, nx, ny, cws[k]) for k in some]
    part = dev.check(boxes, [cws[k] for k in some], nx, ny, some)
    every = dev.check([box_of(k, nx, ny, cws[k]) for k in range(n)], cws, nx, ny)
    assert 1000 < part[0].sum() < every[0].sum()
    ts = torch.cuda.Stream()
    on_stream = dev.check(boxes, [cws[k] for k in some], nx, ny, some, stream=ts.cuda_stream, sync=ts.synchronize)
    assert all(np.array_equal(a, b) for a, b in zip(on_stream, part))
    dev.check(boxes, [cws[k] for k in some], nx, ny, some)  # (the last call of a test is on the context's own stream)


def test_refusals_leave_the_words_alone(dev):
    """(f) every refusal leaves all four arrays as they were"""
    nx, ny = 6, 7
    n = len(NS)
    cws = [(4 + k, 5) for k in range(n)]
    dev.upload(draw(np.random.default_rng(158), nx, ny, cws))
    boxes = [box_of(k, nx, ny, cws[k]) for k in range(n)]
    dev.check(boxes, cws, nx, ny)
    good = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
    dev.preset(PRE)

    def refused(cols=dev.cols, preds=good, cells=cws, nx=nx, ny=ny, ds=None):
        with pytest.raises(binding.PcqError) as e:
            dev.launch(None, cells, nx, ny, cols=cols, preds=preds, ds=ds)
        assert e.value.code == PCQ_ERR_ARG, e.value
        assert dev.unchanged()
        return str(e.value)

    def swapped(seq, k, v):
        out = list(seq)
        out[k] = v
        return out

    for a in range(4):                                                                       # each null pointer
        assert "null argument" in refused(ds=swapped(dev.d_words, a, 0))
    refused(nx=0), refused(ny=0), refused(nx=0, ny=0)                                        # 0 cells
    refused(nx=1025, ny=1), refused(nx=25, ny=41), refused(nx=33, ny=32), refused(nx=64, ny=32), refused(nx=2**31, ny=2**31)  # 1025 cells and more
    for bad in (pkg.Predicate.classification(2), pkg.Predicate.bounds_class(*boxes[3], 2)):  # any other predicate kind
        refused(preds=swapped(good, 3, bad))
    c = dev.cols[5]
    for bad in (binding.make_columns(xyz=c.xyz, n=100, xyz_stride=20), binding.make_columns(xyz=c.xyz + 4, n=c.n - 1),
                binding.make_columns(xyz=None, n=100)):                                      # stride, alignment, null positions with points
        refused(cols=swapped(dev.cols, 5, bad))
    refused(cells=swapped(cws, 4, (0, 5))), refused(cells=swapped(cws, 4, (8, 0)))           # a cell width of 0 in a non-empty segment
    lo, hi = boxes[2]
    for a in (0, 1):
        refused(preds=swapped(good, 2, pkg.Predicate.bounds(lo, swapped(hi, a, hi[a] + 1)))) # one lattice step beyond the raster
    # the order of the mean-height raster's refusals: a null array before the number of cells, that before a segment's refusal
    assert "null argument" in refused(ds=swapped(dev.d_words, 3, 0), nx=0, preds=swapped(good, 3, pkg.Predicate.classification(2)))
    assert "cells" in refused(nx=1025, ny=1, preds=swapped(good, 3, pkg.Predicate.classification(2)))
    # nsegments == 0 is PCQ_OK with nothing written, after the argument checks
    dev.launch([], [], nx, ny, [])
    assert dev.unchanged()
    assert "null argument" in refused(cols=[], preds=[], cells=[], ds=swapped(dev.d_words, 2, 0))
    assert "cells" in refused(cols=[], preds=[], cells=[], nx=1025, ny=1)
    # 1024 cells are accepted, and the table stored before the refusals serves the next call
    dev.check(boxes, cws, nx, ny)
    dev.check([box_of(k, 32, 32, (1, 1)) for k in range(n)], [(1, 1)] * n, 32, 32)
