"""pcq_scan_dev_zmoments_raster_batch beside the three other raster entries on ONE context: the four share the segment table's kind
(PCQ_SEGMENTS_RASTER: an upload whose bytes equal the stored table's is skipped), the context's partials (whose size and slice
offsets follow the entry's words per cell — 1, 1, 2 and 4 — and the launch's cell count) and the scratch stream.

One sequence of calls, every one checked against numpy: the height-spread raster alternating with pcq_scan_dev_raster_batch,
pcq_scan_dev_zrange_raster_batch and pcq_scan_dev_zsum_raster_batch over one byte-identical segment table (boxes and cell widths A:
the boxes are 6 x 7 cells, the launches' rasters 6 x 7, 8 x 8, 16 x 40 and 32 x 32, which changes the cell numbering and the partials'
size but no byte of the table) and over a changed one (boxes and widths B).

What turns it red: a table reused although its bytes differ, or another entry's table layout taken for this one's under the shared
kind; slices of a larger earlier launch left in the partials and folded in; a finish that reads the four arrays at offsets of
another cell count or another entry; partials not grown for four words per cell.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402
import _zmoments as zm  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

NS, WORDS = zm.NS, zm.WORDS
BX, BY = 6, 7  # the boxes' cells: every launch's raster holds them
A = [(4 + k, 5) for k in range(len(NS))]
B = [(3, 4 + k) for k in range(len(NS))]
SEQUENCE = [("zmoments", "A", 6, 7), ("raster", "A", 6, 7), ("zmoments", "A", 32, 32), ("zrange", "A", 8, 8), ("zmoments", "A", 6, 7),
            ("zsum", "A", 16, 40), ("zmoments", "A", 8, 8), ("zmoments", "B", 8, 8), ("zsum", "B", 6, 7), ("zmoments", "B", 32, 32),
            ("raster", "B", 32, 32), ("zmoments", "A", 6, 7), ("zrange", "B", 16, 40), ("zmoments", "B", 6, 7), ("zmoments", "B", 16, 40),
            ("zsum", "A", 32, 32), ("zmoments", "A", 16, 40)]


def tables():
    out = {}
    for name, cws, slab in (("A", A, None), ("B", B, (-2**29, 2**31))):
        out[name] = ([zm.box_of(k, BX, BY, cws[k], slab) for k in range(len(NS))], cws)
    return out


def other_entry(dev, entry, boxes, cws, nx, ny):
    """One call of one of the three older entries into d_zsum_words, against numpy"""
    ctx = dev.ctx
    cell, z = dev.cells_and_z(boxes, cws, nx, ny)
    preds = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
    d0, d1 = dev.d_zsum_words
    if entry == "zrange":
        lo, hi = np.full(WORDS, zm.I32_MAX, dtype=np.int32), np.full(WORDS, zm.I32_MIN, dtype=np.int32)
        ctx.to_device(d0, lo), ctx.to_device(d1, hi)
        ctx.scan_dev_zrange_raster_batch(dev.cols, preds, cws, nx, ny, d0, d1)
        np.minimum.at(lo, cell, z.astype(np.int32)), np.maximum.at(hi, cell, z.astype(np.int32))
        want = [lo, hi]
    else:
        want = [zm.PRE[0].copy(), zm.PRE[1].copy()]
        ctx.to_device(d0, want[0]), ctx.to_device(d1, want[1])
        np.add.at(want[0], cell, 1)
        if entry == "raster":
            ctx.scan_dev_raster_batch(dev.cols, preds, cws, nx, ny, d0)
        else:
            ctx.scan_dev_zsum_raster_batch(dev.cols, preds, cws, nx, ny, d0, d1)
            np.add.at(want[1], cell, z)
    for d, w in zip((d0, d1), want):
        got = np.zeros_like(w)
        ctx.to_host(got, d)  # (waits for the context's stream)
        assert np.array_equal(got, w), (entry, nx, ny, int((got != w).sum()))
    return len(cell)


def test_alternating_entries_on_one_context(gpu_ctx):
    dev = zm.Dev(gpu_ctx)
    try:
        dev.upload(zm.draw(np.random.default_rng(4100), BX, BY, [(max(a[0], b[0]), max(a[1], b[1])) for a, b in zip(A, B)]))
        t = tables()
        kept = {}
        for step, (entry, name, nx, ny) in enumerate(SEQUENCE):
            boxes, cws = t[name]
            try:
                if entry == "zmoments":
                    n = int(dev.check(boxes, cws, nx, ny)[0].sum())
                    if step % 2:
                        dev.check(boxes, cws, nx, ny, pre=zm.ZEROS)  # (the byte-identical table and cell count again)
                else:
                    n = other_entry(dev, entry, boxes, cws, nx, ny)
            except AssertionError as e:
                raise AssertionError(f"step {step}: {entry} over table {name} at {nx} x {ny} cells: {e}") from e
            assert kept.setdefault(name, n) == n and n > 1000  # every entry keeps the same points of a table
        assert kept["A"] != kept["B"]
        # every neighbour pair the docstring names is in the sequence
        pairs = {(a[0], b[0], a[1] == b[1]) for a, b in zip(SEQUENCE, SEQUENCE[1:])}
        for older in ("raster", "zrange", "zsum"):
            assert (older, "zmoments", True) in pairs and ("zmoments", older, True) in pairs, older
        assert ("zmoments", "zmoments", False) in pairs and ("raster", "zmoments", False) in pairs
    finally:
        dev.free()
