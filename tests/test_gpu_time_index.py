"""pcq_scan_dev_indexed_time: PCQ_PRED_TIME through the time part of the chunk index (minimum, maximum and NaN count per 4096
GPS times), against numpy, pcq_scan_dev on the same columns and the numpy model of the chunk states (_time_index_model.py),
which gives the exact skipped / whole / scanned of every pruned scan.

Covered: the seams of the chunking (n around one chunk, a ragged tail, many chunks; ranges cut at chunk boundaries and inside
chunks), the IEEE corners of the state table (one NaN in a contained chunk, a chunk of NaNs, extremes equal to a bound, signed
zeros, infinities, empty / reversed / NaN ranges), the layouts that fall through to pcq_scan_dev, the independence of the three
parts of one index object, collectors that hold something already, a caller's stream, and the refusals.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _time_images as ti  # noqa: E402
import _time_index_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
POINT_DTYPE = binding.POINT_DTYPE
CH = tm.CHUNK
SC = dict(scale=list(ti.SCALE), offset=list(ti.OFFSET))
NMAX = 300_001
INF = np.inf


class Dev:
    """Device copies of host arrays, freed together."""

    def __init__(self, ctx):
        self.ctx, self.blocks = ctx, []

    def put(self, arr, pad=0):
        arr = np.ascontiguousarray(arr)
        base = self.ctx.alloc(arr.nbytes + 64 + pad)
        self.blocks.append(base)
        self.ctx.to_device(base + pad, arr)
        return base + pad

    def free(self):
        for b in self.blocks:
            self.ctx.free(b)
        self.blocks = []


@pytest.fixture(scope="module")
def data():
    """Positions and sorted (acquisition order) times of NMAX points; every test takes a prefix."""
    xyz, cls, _, t = ti.points(NMAX, 4242)
    assert len(np.unique(t)) == NMAX
    return xyz, cls, t


def stats3(st):
    return st["skipped"], st["whole"], st["scanned"]


def run(ctx, cols, pred, kind, ix=None, stream=None, old_entry=False):
    """The count, or the records as bytes, of one scan into a fresh collector: plain (ix None) or through the index."""
    g = ctx.count_collector() if kind == "count" else ctx.buffer_collector()
    try:
        if ix is None:
            ctx.scan_dev(cols, pred, g, stream)
        elif old_entry:
            ctx.scan_dev_indexed(cols, pred, ix, g, stream)
        else:
            ctx.scan_dev_indexed_time(cols, pred, ix, g, stream)
        return g.point_count() if kind == "count" else g.points().tobytes()
    finally:
        g.free()


def expected(xyz, t, start, end, kind):
    sel = ti.select(t, start, end)
    return int(sel.sum()) if kind == "count" else ti.expect_records(xyz, sel, POINT_DTYPE).tobytes()


def check_pruned(ctx, cols, ix, xyz, t, ranges, what=""):
    """Every range, count and records, through an index whose time part exists: results, and statistics equal to the model."""
    n = len(t)
    for start, end in ranges:
        pred = pkg.Predicate.time_range(start, end)
        for kind in ("count", "buffer"):
            got = run(ctx, cols, pred, kind, ix)
            st = ctx.index_stats(ix)
            w = (what, start, end, kind, st)
            assert got == expected(xyz, t, start, end, kind), w
            assert got == run(ctx, cols, pred, kind), w
            assert st["built"] == 0 and st["chunks"] == n // CH, w
            assert stats3(st) == tm.classify(t, start, end), w


def seam_ranges(t):
    n = len(t)

    def at(i):
        return float(t[min(i, n - 1)])

    return [(at(CH), at(2 * CH)),                      # cut at two chunk boundaries: chunk 1 exactly
            (at(100), at(CH + 904)),                   # both cuts inside chunks
            (at(0), at(CH - 1)),                       # chunk 0 without its last time
            (at(2 * CH), np.nextafter(at(n - 1), INF)),  # from a boundary to the end, the tail included
            (at(6000), at(6100)), (at(150_000), at(153_000)),
            (-INF, INF), (1500.0, 1500.0), (1600.0, 1400.0)]


@pytest.mark.parametrize("n", [4095, 4096, 4097, 3 * 4096 + 1, NMAX])
def test_seams_of_the_chunking(gpu_ctx, data, n):
    ctx = gpu_ctx
    xyz, t = data[0][:n], data[2][:n]
    dev, ix, ix2 = Dev(ctx), ctx.index_new(), ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(t), n=n, cls_stride=8, **SC)
        ranges = seam_ranges(t)
        if n < CH:  # no whole chunk: the plain scan, statistics that claim nothing
            for start, end in ranges:
                for kind in ("count", "buffer"):
                    pred = pkg.Predicate.time_range(start, end)
                    assert run(ctx, cols, pred, kind, ix) == expected(xyz, t, start, end, kind) == run(ctx, cols, pred, kind)
                    assert not any(ctx.index_stats(ix).values())
            return
        # the building call: a count on one index, a buffer scan on the other; both answer and report the build
        start, end = ranges[1]
        pred = pkg.Predicate.time_range(start, end)
        for which, kind in ((ix, "count"), (ix2, "buffer")):
            assert run(ctx, cols, pred, kind, which) == expected(xyz, t, start, end, kind), kind
            st = ctx.index_stats(which)
            assert st == dict(chunks=n // CH, skipped=0, whole=0, scanned=n // CH, built=1), (kind, st)
        check_pruned(ctx, cols, ix, xyz, t, ranges, "built by a count")
        check_pruned(ctx, cols, ix2, xyz, t, ranges[:4], "built by a buffer scan")
        if n // CH >= 3:
            assert tm.classify(t, *ranges[0]) == (n // CH - 1, 1, 0)      # the model says: everything but chunk 1 is skipped
            assert tm.classify(t, *ranges[1])[0] == n // CH - 2 > 0
        # a count needs no positions
        count_cols = binding.make_columns(cls=cols.cls, n=n, cls_stride=8)
        assert run(ctx, count_cols, pred, "count", ix) == expected(xyz, t, start, end, "count")
        assert ctx.index_stats(ix)["built"] == 0
    finally:
        ctx.index_free(ix)
        ctx.index_free(ix2)
        dev.free()


def corner_times():
    """Seven chunks and a tail, one for every line of the state table."""
    rng = np.random.default_rng(31)
    inside = rng.uniform(0.25, 0.75, CH)
    one_nan = inside.copy()
    one_nan[2345] = np.nan
    exact = rng.permutation(np.linspace(0.25, 0.75, CH))         # min == 0.25 and max == 0.75 exactly
    zeros = np.where(rng.integers(0, 2, CH) == 0, 0.0, -0.0)
    infs = np.where(rng.integers(0, 2, CH) == 0, INF, -INF)
    tail = ti.adversarial_times(77, 0.25, 0.75, 5)
    t = np.concatenate([one_nan, np.full(CH, np.nan), exact, zeros, np.full(CH, INF), np.full(CH, -INF), infs, tail])
    return t


CORNER_RANGES = [(0.25, 0.76), (0.0, 0.75), (0.0, 0.25), (0.75, 2.0), (-0.0, 5e-324), (0.0, 1.0), (-INF, INF), (1.0, INF)]


def test_ieee_corners_of_the_state_table(gpu_ctx):
    ctx = gpu_ctx
    t = corner_times()
    n = len(t)
    xyz = ti.points(n, 77)[0]
    S, N, A = tm.SCAN, tm.NONE, tm.ALL
    # what the table says, chunk by chunk (one NaN, NaNs, exact, zeros, +inf, -inf, both infinities)
    assert tm.states(t, 0.25, 0.76) == [S, N, A, N, N, N, S]     # one NaN: read, not whole; the NaN chunk: skipped
    assert int(ti.select(t[:CH], 0.25, 0.76).sum()) == CH - 1
    assert tm.states(t, 0.0, 0.75)[2] == S                        # max == end: not whole
    assert tm.states(t, 0.0, 0.25)[2] == N                        # min == end: skipped
    assert tm.states(t, 0.75, 2.0)[2] == S                        # max == start: read
    assert tm.states(t, -0.0, 5e-324)[3] == A and tm.states(t, 0.0, 1.0)[3] == A
    assert tm.states(t, -INF, INF) == [S, N, A, A, N, A, S]
    assert tm.states(t, 1.0, INF)[4:] == [N, N, S]
    dev, ix = Dev(ctx), ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(t), n=n, cls_stride=8, **SC)
        pred = pkg.Predicate.time_range(0.25, 0.76)
        assert run(ctx, cols, pred, "count", ix) == expected(xyz, t, 0.25, 0.76, "count")
        assert ctx.index_stats(ix)["built"] == 1
        check_pruned(ctx, cols, ix, xyz, t, CORNER_RANGES + ti.RANGES, "corners")
    finally:
        ctx.index_free(ix)
        dev.free()


def test_adversarial_times_for_every_pair_of_bounds(gpu_ctx):
    """Times on and around both bounds and the IEEE special values, over 5 chunks and a tail; chunk 1 is all NaN, chunk 2 sorted
    below the start where that is finite, chunk 3 holds only the start bound itself."""
    ctx = gpu_ctx
    n = 5 * CH + 77
    xyz = ti.points(n, 78)[0]
    dev, ix = Dev(ctx), ctx.index_new()
    try:
        d_xyz = dev.put(xyz)
        for k, (start, end) in enumerate(ti.RANGES):
            t = ti.adversarial_times(n, start, end, 900 + k)
            t[CH:2 * CH] = np.nan
            if np.isfinite(start):
                t[2 * CH:3 * CH] = start - np.abs(t[2 * CH:3 * CH]) - 1.0
                t[3 * CH:4 * CH] = start
            if k % 2:  # (chunk 0 with and without NaNs)
                t[:CH] = np.where(np.isnan(t[:CH]), 0.0, t[:CH])
            cols = binding.make_columns(xyz=d_xyz, cls=dev.put(t), n=n, cls_stride=8, **SC)  # another column: the part is rebuilt
            pred = pkg.Predicate.time_range(start, end)
            assert run(ctx, cols, pred, "buffer", ix) == expected(xyz, t, start, end, "buffer"), (start, end)
            assert ctx.index_stats(ix) == dict(chunks=5, skipped=0, whole=0, scanned=5, built=1)
            check_pruned(ctx, cols, ix, xyz, t, [(start, end)] + ti.RANGES[:3], "adversarial")
    finally:
        ctx.index_free(ix)
        dev.free()


def test_layouts_the_index_does_not_cover_fall_through_and_leave_it_alone(gpu_ctx, data):
    ctx = gpu_ctx
    n = 3 * CH + 1
    xyz, cls, t = data[0][:n], data[1][:n], data[2][:n]
    dev = Dev(ctx)
    ix, fresh = ctx.index_new(), ctx.index_new()
    try:
        d_xyz = dev.put(xyz)
        cols = binding.make_columns(xyz=d_xyz, cls=dev.put(t), n=n, cls_stride=8, **SC)
        start, end = float(t[100]), float(t[CH + 904])
        pred = pkg.Predicate.time_range(start, end)
        run(ctx, cols, pred, "count", ix)
        assert run(ctx, cols, pred, "count", ix) == expected(xyz, t, start, end, "count")
        before = ctx.index_stats(ix)
        assert before["built"] == 0 and before["chunks"] == 3 and before["skipped"] > 0
        rec = ti.records(1, xyz, cls, np.zeros((n, 3), dtype=np.uint16), t)  # LAS format 1: 28-byte records, the time at +20
        p = dev.put(rec)
        uncovered = [(binding.make_columns(xyz=d_xyz, cls=dev.put(t, pad=8), n=n, cls_stride=8, **SC), n),  # 8 bytes off a 16-byte boundary
                     (binding.make_columns(xyz=p, cls=p + 20, n=n, xyz_stride=28, cls_stride=28, **SC), n),   # strided records
                     (binding.make_columns(xyz=d_xyz, cls=cols.cls, n=CH - 1, cls_stride=8, **SC), CH - 1)]    # no whole chunk
        for which in (ix, fresh):
            for c, m in uncovered:
                for kind in ("count", "buffer"):
                    assert run(ctx, c, pred, kind, which) == expected(xyz[:m], t[:m], start, end, kind) == run(ctx, c, pred, kind)
                    assert not any(ctx.index_stats(which).values())
        assert run(ctx, cols, pred, "count", ix) == expected(xyz, t, start, end, "count")
        assert ctx.index_stats(ix) == before           # still the part it had
        assert run(ctx, cols, pred, "count", fresh) == expected(xyz, t, start, end, "count")
        assert ctx.index_stats(fresh)["built"] == 1    # nothing had been built into it
    finally:
        ctx.index_free(ix)
        ctx.index_free(fresh)
        dev.free()


def test_the_three_parts_of_an_index_stay_apart(gpu_ctx, data):
    ctx = gpu_ctx
    n = 70_001
    xyz, cls, t = data[0][:n], data[1][:n], data[2][:n]
    lo, hi = [-100, -5000, -1000], [100, 5000, 1000]
    inside = int(np.all((xyz >= np.asarray(lo)) & (xyz <= np.asarray(hi)), axis=1).sum())
    dev, ix = Dev(ctx), ctx.index_new()
    try:
        d_xyz, d_t = dev.put(xyz), dev.put(t)
        ccols = binding.make_columns(xyz=d_xyz, cls=dev.put(cls), n=n, **SC)
        tcols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, **SC)
        bpred, cpred = pkg.Predicate.bounds(lo, hi), pkg.Predicate.classification(6)
        start, end = float(t[5000]), float(t[9000])
        tpred = pkg.Predicate.time_range(start, end)

        def old():
            assert run(ctx, ccols, bpred, "count", ix, old_entry=True) == inside
            b = ctx.index_stats(ix)
            assert run(ctx, ccols, cpred, "count", ix, old_entry=True) == int((cls == 6).sum())
            return b, ctx.index_stats(ix)

        b0, c0 = old()
        assert b0["built"] == 1 and c0["built"] == 1
        b1, c1 = old()
        assert b1["built"] == 0 and c1["built"] == 0 and b1["chunks"] == n // CH and c1["whole"] == c1["chunks"] == (n + 65535) // 65536
        # the time part arrives beside them
        want = expected(xyz, t, start, end, "count")
        assert run(ctx, tcols, tpred, "count", ix) == want and ctx.index_stats(ix)["built"] == 1
        assert old() == (b1, c1)                       # pruned as before, nothing rebuilt
        assert run(ctx, tcols, tpred, "count", ix) == want
        pruned = ctx.index_stats(ix)
        assert pruned["built"] == 0 and stats3(pruned) == tm.classify(t, start, end) and pruned["skipped"] > 0
        # the old entry with a time predicate: the plain scan and statistics that claim nothing, the part exists or not
        for kind in ("count", "buffer"):
            assert run(ctx, tcols, tpred, kind, ix, old_entry=True) == expected(xyz, t, start, end, kind)
            assert not any(ctx.index_stats(ix).values())
        assert run(ctx, tcols, tpred, "buffer", ix) == expected(xyz, t, start, end, "buffer")
        assert ctx.index_stats(ix) == pruned           # ... and it did not touch the part
        # other columns, or the same pointer with another n: the part is rebuilt
        other = binding.make_columns(xyz=d_xyz, cls=dev.put(t), n=n, cls_stride=8, **SC)
        assert run(ctx, other, tpred, "count", ix) == want and ctx.index_stats(ix)["built"] == 1
        assert run(ctx, other, tpred, "count", ix) == want and ctx.index_stats(ix)["built"] == 0
        m = n - 5000
        shorter = binding.make_columns(xyz=d_xyz, cls=other.cls, n=m, cls_stride=8, **SC)
        assert run(ctx, shorter, tpred, "count", ix) == expected(xyz[:m], t[:m], start, end, "count")
        st = ctx.index_stats(ix)
        assert st["built"] == 1 and st["chunks"] == m // CH
        assert run(ctx, other, tpred, "count", ix) == want and ctx.index_stats(ix)["built"] == 1
        assert old() == (b1, c1)
    finally:
        ctx.index_free(ix)
        dev.free()


def test_collectors_that_hold_something_and_a_callers_stream(gpu_ctx, data):
    import torch
    ctx = gpu_ctx
    n = 5 * CH + 123
    xyz, t = data[0][:n], data[2][:n]
    dev, ix = Dev(ctx), ctx.index_new()
    ts = torch.cuda.Stream()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(t), n=n, cls_stride=8, **SC)
        a, b = (float(t[3000]), float(t[9000])), (float(t[CH]), float(t[n - 1]))
        ra, rb = expected(xyz, t, *a, "buffer"), expected(xyz, t, *b, "buffer")
        pa, pb = pkg.Predicate.time_range(*a), pkg.Predicate.time_range(*b)
        gb = ctx.buffer_collector()
        ctx.scan_dev(cols, pa, gb)                       # records of a plain scan first
        ctx.scan_dev_indexed_time(cols, pb, ix, gb)      # the building call appends
        later = binding.make_columns(xyz=cols.xyz, cls=cols.cls, n=n, cls_stride=8, first_index=n, **SC)
        ctx.scan_dev_indexed_time(later, pa, ix, gb)     # a pruned call, as the second file of a query
        assert ctx.index_stats(ix)["built"] == 0
        ctx.scan_dev_indexed_time(later, pb, ix, gb, ts.cuda_stream)  # ... and on the caller's stream
        assert stats3(ctx.index_stats(ix)) == tm.classify(t, *b)
        assert gb.points().tobytes() == ra + rb + ra + rb
        gb.free()
        cc = ctx.count_collector()
        ctx.scan_dev_indexed_time(cols, pa, ix, cc)
        ctx.scan_dev_indexed_time(cols, pb, ix, cc, ts.cuda_stream)
        assert stats3(ctx.index_stats(ix)) == tm.classify(t, *b)
        ctx.scan_dev(cols, pa, cc)
        assert cc.point_count() == (2 * len(ra) + len(rb)) // 31
        cc.free()
    finally:
        ctx.index_free(ix)
        dev.free()


def test_refusals(gpu_ctx, data):
    ctx = gpu_ctx
    n = 2 * CH + 5
    xyz, cls, t = data[0][:n], data[1][:n], data[2][:n]
    dev, ix = Dev(ctx), ctx.index_new()
    try:
        d_xyz = dev.put(xyz)
        tcols = binding.make_columns(xyz=d_xyz, cls=dev.put(t), n=n, cls_stride=8, **SC)
        ccols = binding.make_columns(xyz=d_xyz, cls=dev.put(cls), n=n, **SC)
        tpred = pkg.Predicate.time_range(float(t[10]), float(t[5000]))
        lo, hi = [-100] * 3, [100] * 3
        cc, gb = ctx.count_collector(), ctx.buffer_collector()
        gg = ctx.grid_collector([-1000.0] * 3, [1000.0] * 3, 10.0)
        bad = [(ccols, pkg.Predicate.bounds(lo, hi), cc), (ccols, pkg.Predicate.classification(6), cc),
               (ccols, pkg.Predicate.bounds_class(lo, hi, 6), gb), (tcols, pkg.Predicate.bounds_time(lo, hi, 0.0, 1.0), cc),
               (ccols, pkg.Predicate.bounds_f64([-1.0] * 3, [1.0] * 3), gb), (tcols, tpred, gg)]
        for cols, pred, coll in bad:
            with pytest.raises(binding.PcqError) as e:
                ctx.scan_dev_indexed_time(cols, pred, ix, coll)
            assert e.value.code == -8, pred.kind
        import ctypes as C
        lib = ctx.lib
        args = [ctx.handle, C.byref(tcols), C.byref(tpred), C.c_void_p(ix), cc.handle, None]
        for k in range(5):
            a = list(args)
            a[k] = None
            assert lib.pcq_scan_dev_indexed_time(*a) == -8, k
        # a buffer collector needs positions: refused by the validation, before the index or the collector is touched
        nopos = binding.make_columns(cls=tcols.cls, n=n, cls_stride=8)
        with pytest.raises(binding.PcqError) as e:
            ctx.scan_dev_indexed_time(nopos, tpred, ix, gb)
        assert e.value.code == -8
        assert cc.point_count() == 0 and gb.point_count() == 0 and gg.point_count() == 0
        assert not any(ctx.index_stats(ix).values())
        assert run(ctx, tcols, tpred, "count", ix) == 4990 and ctx.index_stats(ix)["built"] == 1  # nothing had been built
        cc.free(), gb.free(), gg.free()
    finally:
        ctx.index_free(ix)
        dev.free()
