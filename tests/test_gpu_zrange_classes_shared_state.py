"""pcq_scan_dev_zrange_raster_batch_classes beside pcq_scan_dev_zsum_raster_batch_classes on ONE context: the two share the segment
table's kind (PCQ_SEGMENTS_RASTER_CLASSES: an upload whose bytes equal the stored table's is skipped, so a table uploaded by one
entry serves the other), the context's partials (one word per cell here, two there) and the scratch stream.

One sequence of calls, every one checked against numpy: the two entries alternating over one byte-identical segment table (boxes and
cell widths A: the boxes are 6 x 7 cells, the launches' rasters 6 x 7, 8 x 8, 16 x 40 and 32 x 32, which changes the cell numbering and
the partials' size but no byte of the table) and over a changed one (boxes and widths B).  Then two calls of the new entry over the
same segments with other sets, back to back, and one on a caller's stream: a set served from a cache folds the earlier set's points.

What turns it red: a table reused although its bytes differ; slices of a larger earlier launch or of the other entry's second word
per cell left in the partials and folded in; partials read at another entry's offsets; a set kept with the cached table.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _canopy as cn  # noqa: E402
import _pipeline_plan as pp  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

NS = (0, 1, 511, 512, 513, 1535, 4133)
MIS = (0, 1, 2, 3, 0, 1, 2)
BX, BY = 6, 7  # the boxes' cells: every launch's raster holds them
A = [(4 + k, 5) for k in range(len(NS))]
B = [(3, 4 + k) for k in range(len(NS))]
LOW, HIGH = (2,), cn.BUT_7_18
SUM_SET = (2, 9)
SEQUENCE = [("canopy", "A", 6, 7), ("zsum", "A", 6, 7), ("canopy", "A", 32, 32), ("zsum", "A", 8, 8), ("canopy", "A", 6, 7),
            ("zsum", "A", 16, 40), ("canopy", "A", 8, 8), ("canopy", "B", 8, 8), ("zsum", "B", 6, 7), ("canopy", "B", 32, 32),
            ("zsum", "B", 32, 32), ("canopy", "A", 6, 7), ("canopy", "B", 16, 40), ("zsum", "A", 32, 32), ("canopy", "A", 16, 40)]


def tables():
    return {name: ([cn.box_of(k, BX, BY, cws[k], slab) for k in range(len(NS))], cws)
            for name, cws, slab in (("A", A, None), ("B", B, (-30, 10)))}


def zsum_entry(dev, d_cnt, d_sum, boxes, cws, nx, ny):
    """One call of the class-filtered mean-height entry from zeroed words, against numpy on int64"""
    ctx = dev.ctx
    cnt, zsum = np.zeros(nx * ny + 16, dtype=np.int64), np.zeros(nx * ny + 16, dtype=np.int64)
    ctx.to_device(d_cnt, cnt), ctx.to_device(d_sum, zsum)
    ctx.scan_dev_zsum_raster_batch_classes(dev.cols, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], cws, nx, ny, SUM_SET, d_cnt, d_sum)
    for k, (lo, hi) in enumerate(boxes):
        p = dev.xyz[k][pp.in_box(dev.xyz[k], lo, hi) & cn.in_set(dev.cls[k], SUM_SET)].astype(np.int64)
        cell = ((p[:, 1] - lo[1]) // cws[k][1]) * nx + (p[:, 0] - lo[0]) // cws[k][0]
        np.add.at(cnt, cell, 1), np.add.at(zsum, cell, p[:, 2])
    for d, w, name in ((d_cnt, cnt, "count"), (d_sum, zsum, "sum")):
        got = np.zeros_like(w)
        ctx.to_host(got, d)  # (waits for the context's stream)
        assert np.array_equal(got, w), (name, nx, ny, int((got != w).sum()))
    return int(cnt.sum())


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    d = cn.Dev(gpu_ctx, NS)
    d.upload(*cn.draw(np.random.default_rng(4200), NS, BX, BY, [(max(a[0], b[0]), max(a[1], b[1])) for a, b in zip(A, B)],
                      classes=(0, 2, 5, 7, 9, 18, 255)), MIS)
    yield d
    d.free()


def test_alternating_entries_on_one_context(dev):
    ctx = dev.ctx
    d_cnt, d_sum = ctx.alloc(8 * (32 * 32 + 16)), ctx.alloc(8 * (32 * 32 + 16))
    try:
        t = tables()
        kept = {}
        for step, (entry, name, nx, ny) in enumerate(SEQUENCE):
            boxes, cws = t[name]
            try:
                if entry == "canopy":
                    zmin, zmax = dev.check(boxes, cws, nx, ny, LOW, HIGH)
                    assert not np.array_equal(zmin, cn.PRE_MIN[:nx * ny]) and not np.array_equal(zmax, cn.PRE_MAX[:nx * ny])
                    if step % 2:
                        dev.check(boxes, cws, nx, ny, LOW, HIGH, pre=cn.SENT)  # (the byte-identical table and cell count again)
                else:
                    n = zsum_entry(dev, d_cnt, d_sum, boxes, cws, nx, ny)
                    assert kept.setdefault(name, n) == n and n > 100  # the entry keeps the same points of a table at every raster
            except AssertionError as e:
                raise AssertionError(f"step {step}: {entry} over table {name} at {nx} x {ny} cells: {e}") from e
        assert kept["A"] != kept["B"]
        pairs = {(a[0], b[0], a[1] == b[1]) for a, b in zip(SEQUENCE, SEQUENCE[1:])}
        assert {("canopy", "zsum", True), ("zsum", "canopy", True), ("canopy", "canopy", False), ("zsum", "canopy", False),
                ("canopy", "zsum", False)} <= pairs
    finally:
        ctx.free(d_cnt), ctx.free(d_sum)


def test_two_pairs_of_sets_in_a_row_and_a_callers_stream(dev):
    """identical columns, predicates, cells and outputs; sets ({2}, {5}) then ({5}, {2}) then ({9}, all): each call folds its own
    sets' points into what the one before left; the third on a caller's torch stream"""
    import torch
    nx, ny = 8, 8
    boxes, cws = tables()["A"]
    calls = [((2,), (5,)), ((5,), (2,)), ((9,), cn.ALL)]
    want = [(cn.SENT[0].copy(), cn.SENT[1].copy())]
    for low, high in calls:
        want.append(dev.want(boxes, cws, nx, ny, low, high, pre=want[-1]))
    stale = dev.want(boxes, cws, nx, ny, *calls[0], pre=want[1])  # (the second call with the first call's sets)
    assert not np.array_equal(stale[0], want[2][0]) and not np.array_equal(stale[1], want[2][1])
    assert not np.array_equal(want[3][1], want[2][1])
    dev.preset(cn.SENT)
    dev.launch(boxes, cws, nx, ny, *calls[0])
    dev.compare(want[1], "first")
    dev.launch(boxes, cws, nx, ny, *calls[1])
    dev.compare(want[2], "second")
    ts = torch.cuda.Stream()
    dev.launch(boxes, cws, nx, ny, *calls[2], stream=ts.cuda_stream)
    ts.synchronize()
    dev.compare(want[3], "stream")
    dev.check(boxes, cws, nx, ny, LOW, HIGH)  # (the last call of a test is on the context's own stream)
