"""pcq_scan_dev_indexed_combined: PCQ_PRED_BOUNDS_CLASS through both parts of the chunk index (an integer AABB per 4096
points, a class histogram per 65536), against numpy and pcq_scan_dev.

One file of 2 x 65536 + 3 x 4096 + 1234 points in which all nine pairs of (box state, class state) occur among the 35 bounds
chunks: x ascends inside every class chunk (x = i mod 65536), so the box's x range [2000, 8191] straddles the first bounds
chunk of each class chunk, contains the second and is disjoint from the rest; class chunk 0 is entirely the queried class,
class chunk 1 has none of it, the partial class chunk 2 is mixed.  The last 1234 points (the ragged tail, never indexed) lie
inside the box, some of the queried class and some not: a tail scanned without its class bytes, or with the file's first
ones, counts wrong.
"""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
N = 2 * 65536 + 3 * 4096 + 1234
CHUNKS = N // 4096
Q = 6  # the queried class
LO, HI = [2000, -1000, -1000], [8191, 1000, 1000]
SC = dict(scale=[0.01, 0.01, 0.01], offset=[5.0, -7.0, 1.0])
NONE, ALL, SCAN = 1, 2, 0


class Dev:
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


def inside(xyz, lo=LO, hi=HI):
    x = xyz.astype(np.int64)
    return np.all((x >= np.asarray(lo, dtype=np.int64)) & (x <= np.asarray(hi, dtype=np.int64)), axis=1)


def classify(xyz, cls, n, lo=LO, hi=HI, c=Q):
    """(skipped, whole, scanned) by the definition: box state of bounds chunk ch with the class state of class chunk ch >> 4."""
    k = {NONE: 0, ALL: 0, SCAN: 0}
    states = set()
    for ch in range(n // 4096):
        p = xyz[4096 * ch: 4096 * (ch + 1)].astype(np.int64)
        mn, mx = p.min(axis=0), p.max(axis=0)
        if np.any(mx < np.asarray(lo)) or np.any(mn > np.asarray(hi)):
            b = NONE
        else:
            b = ALL if np.all(mn >= np.asarray(lo)) and np.all(mx <= np.asarray(hi)) else SCAN
        first = (ch >> 4) * 65536
        points = min(65536, n - first)  # the last class chunk may be partial
        cnt = int((cls[first: first + points] == c).sum())
        s = NONE if cnt == 0 else (ALL if cnt == points else SCAN)
        states.add((b, s))
        k[NONE if NONE in (b, s) else (ALL if b == ALL and s == ALL else SCAN)] += 1
    return (k[NONE], k[ALL], k[SCAN]), states


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(77)
    i = np.arange(N)
    xyz = np.stack([i % 65536, rng.integers(-100, 100, N), rng.integers(-100, 100, N)], axis=1).astype(np.int32)
    cls = np.empty(N, dtype=np.uint8)
    cls[:65536] = Q
    cls[65536:131072] = rng.choice(np.array([1, 2, 9], dtype=np.uint8), 65536)
    cls[131072:] = rng.choice(np.array([1, Q, Q, 9], dtype=np.uint8), N - 131072)
    tail = CHUNKS * 4096
    xyz[tail:, 0] = rng.integers(LO[0], HI[0] + 1, N - tail)  # the tail inside the box, of the queried class and of others
    rgb = rng.integers(0, 65536, (N, 3)).astype(np.uint16)
    sel = inside(xyz) & (cls == Q)
    assert 0 < int(sel[tail:].sum()) < int(inside(xyz[tail:]).sum()) == N - tail
    stats, states = classify(xyz, cls, N)
    assert len(states) == 9 and stats == (31, 1, 3), (stats, states)
    return xyz, cls, rgb, sel


def stats3(st):
    return st["skipped"], st["whole"], st["scanned"]


def count(ctx, cols, pred, ix=None, combined=True):
    cc = ctx.count_collector()
    if ix is None:
        ctx.scan_dev(cols, pred, cc)
    elif combined:
        ctx.scan_dev_indexed_combined(cols, pred, ix, cc)
    else:
        ctx.scan_dev_indexed(cols, pred, ix, cc)
    out = cc.point_count()
    cc.free()
    return out


def records(ctx, cols, pred, ix=None):
    gb = ctx.buffer_collector()
    if ix is None:
        ctx.scan_dev(cols, pred, gb)
    else:
        ctx.scan_dev_indexed_combined(cols, pred, ix, gb)
    out = gb.points().tobytes()
    gb.free()
    return out


@pytest.mark.parametrize("cls_pad", [0, 1, 2, 3])
def test_count_on_the_building_call_and_later(gpu_ctx, data, cls_pad):
    ctx = gpu_ctx
    xyz, cls, _, sel = data
    want, want_stats = int(sel.sum()), classify(xyz, cls, N)[0]
    dev, ix = Dev(ctx), ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(cls, pad=cls_pad), n=N, **SC)
        pred = pkg.Predicate.bounds_class(LO, HI, Q)
        assert count(ctx, cols, pred) == want
        for k in range(3):
            assert count(ctx, cols, pred, ix) == want, k
            st = ctx.index_stats(ix)
            assert st["built"] == (1 if k == 0 else 0) and st["chunks"] == CHUNKS, st
            assert stats3(st) == want_stats and sum(stats3(st)) == CHUNKS, st
        # other boxes and classes through the same index: an empty box, everything, a class no point has, a thin slab
        for lo, hi, c in [([2**31, 0, 0], [2**31 + 5, 1, 1], Q), ([-2**31] * 3, [2**31 - 1] * 3, Q), (LO, HI, 77), (LO, HI, 9),
                          ([4000, -50, -1000], [4100, 50, 1000], Q), ([0, -1000, -1000], [65535, 1000, 1000], 1)]:
            p = pkg.Predicate.bounds_class(lo, hi, c)
            got, st = count(ctx, cols, p, ix), ctx.index_stats(ix)
            assert got == int((inside(xyz, lo, hi) & (cls == c)).sum()) == count(ctx, cols, p), (lo, hi, c)
            assert st["built"] == 0 and stats3(st) == classify(xyz, cls, N, lo, hi, c)[0], (lo, hi, c, st)
    finally:
        ctx.index_free(ix)
        dev.free()


@pytest.mark.parametrize("colours", [True, False])
def test_records_equal_the_plain_scan_and_follow_what_the_collector_holds(gpu_ctx, data, colours):
    ctx = gpu_ctx
    xyz, cls, rgb, sel = data
    want_stats = classify(xyz, cls, N)[0]
    dev, ix = Dev(ctx), ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(cls, pad=1), rgb=dev.put(rgb) if colours else None, n=N, **SC)
        pred = pkg.Predicate.bounds_class(LO, HI, Q)
        plain = records(ctx, cols, pred)
        assert len(plain) == 31 * int(sel.sum())
        for k in range(2):
            assert records(ctx, cols, pred, ix) == plain, k
            st = ctx.index_stats(ix)
            assert st["built"] == (1 if k == 0 else 0) and st["chunks"] == CHUNKS and stats3(st) == want_stats, st
        # behind records the collector already holds (of another query, unindexed), and once more behind those
        other = pkg.Predicate.bounds_class([0, -1000, -1000], [65535, 1000, 1000], 9)
        first = records(ctx, cols, other)
        assert len(first) == 31 * int((cls == 9).sum())
        gb = ctx.buffer_collector()
        ctx.scan_dev(cols, other, gb)
        ctx.scan_dev_indexed_combined(cols, pred, ix, gb)
        ctx.scan_dev_indexed_combined(cols, other, ix, gb)
        assert gb.points().tobytes() == first + plain + first
        gb.free()
        assert count(ctx, cols, pred, ix) == int(sel.sum())  # a count through the index the buffer scan built
        assert stats3(ctx.index_stats(ix)) == want_stats
    finally:
        ctx.index_free(ix)
        dev.free()


def test_the_index_is_shared_with_the_bounds_and_class_scans_in_both_directions(gpu_ctx, data):
    ctx = gpu_ctx
    xyz, cls, _, sel = data
    dev = Dev(ctx)
    a, b = ctx.index_new(), ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(cls), n=N, **SC)
        pred, bpred, cpred = pkg.Predicate.bounds_class(LO, HI, Q), pkg.Predicate.bounds(LO, HI), pkg.Predicate.classification(Q)
        want_b, want_c = int(inside(xyz).sum()), int((cls == Q).sum())
        # built by pcq_scan_dev_indexed, used by the combined entry
        assert count(ctx, cols, bpred, a, combined=False) == want_b and ctx.index_stats(a)["built"] == 1
        assert count(ctx, cols, cpred, a, combined=False) == want_c and ctx.index_stats(a)["built"] == 1
        assert count(ctx, cols, pred, a) == int(sel.sum())
        st = ctx.index_stats(a)
        assert st["built"] == 0 and stats3(st) == classify(xyz, cls, N)[0], st
        # built by the combined entry, used by pcq_scan_dev_indexed
        assert count(ctx, cols, pred, b) == int(sel.sum()) and ctx.index_stats(b)["built"] == 1
        assert count(ctx, cols, bpred, b, combined=False) == want_b
        st = ctx.index_stats(b)
        assert st["built"] == 0 and st["skipped"] + st["whole"] + st["scanned"] == CHUNKS and st["skipped"] > 0, st
        assert count(ctx, cols, cpred, b, combined=False) == want_c
        assert ctx.index_stats(b)["built"] == 0
        # half an index: only the boxes exist -> the combined entry builds the histograms
        c = ctx.index_new()
        assert count(ctx, cols, bpred, c, combined=False) == want_b
        assert count(ctx, cols, pred, c) == int(sel.sum()) and ctx.index_stats(c)["built"] == 1
        assert count(ctx, cols, cpred, c, combined=False) == want_c and ctx.index_stats(c)["built"] == 0
        ctx.index_free(c)
    finally:
        ctx.index_free(a)
        ctx.index_free(b)
        dev.free()


def test_layouts_the_index_does_not_cover_fall_through_and_leave_it_alone(gpu_ctx, data):
    ctx = gpu_ctx
    xyz, cls, rgb, sel = data
    dev = Dev(ctx)
    ix, fresh = ctx.index_new(), ctx.index_new()
    try:
        d_cls = dev.put(cls, pad=2)
        cols = binding.make_columns(xyz=dev.put(xyz), cls=d_cls, n=N, **SC)
        pred = pkg.Predicate.bounds_class(LO, HI, Q)
        count(ctx, cols, pred, ix)
        assert count(ctx, cols, pred, ix) == int(sel.sum())
        before = ctx.index_stats(ix)
        assert before["built"] == 0 and before["chunks"] == CHUNKS
        rec = np.zeros((N, 34), dtype=np.uint8)  # LAS-like records of 34 bytes
        rec[:, 0:12] = xyz.view(np.uint8).reshape(N, 12)
        rec[:, 15] = cls
        rec[:, 28:34] = rgb.view(np.uint8).reshape(N, 6)
        p = dev.put(rec)
        uncovered = [(binding.make_columns(xyz=cols.xyz, cls=d_cls, n=4095, **SC), int(sel[:4095].sum())),
                     (binding.make_columns(xyz=dev.put(xyz, pad=4), cls=d_cls, n=N, **SC), int(sel.sum())),
                     (binding.make_columns(xyz=p, cls=p + 15, rgb=p + 28, n=N, xyz_stride=34, cls_stride=34, rgb_stride=34, **SC), int(sel.sum()))]
        for which in (ix, fresh):
            for c, want in uncovered:
                assert count(ctx, c, pred, which) == want == count(ctx, c, pred)
                assert not any(ctx.index_stats(which).values())
                assert records(ctx, c, pred, which) == records(ctx, c, pred)
                assert not any(ctx.index_stats(which).values())
        assert count(ctx, cols, pred, ix) == int(sel.sum())
        assert ctx.index_stats(ix) == before          # still the index it had
        assert count(ctx, cols, pred, fresh) == int(sel.sum())
        assert ctx.index_stats(fresh)["built"] == 1   # nothing had been built into it
    finally:
        ctx.index_free(ix)
        ctx.index_free(fresh)
        dev.free()


def test_refusals(gpu_ctx, data):
    ctx = gpu_ctx
    xyz, cls, _, _ = data
    dev, ix = Dev(ctx), ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(cls), n=N, **SC)
        gg = ctx.grid_collector([-1000.0] * 3, [1000.0] * 3, 10.0)
        cc = ctx.count_collector()
        for pred, coll in [(pkg.Predicate.bounds_class(LO, HI, Q), gg), (pkg.Predicate.bounds(LO, HI), cc),
                           (pkg.Predicate.classification(Q), cc)]:
            with pytest.raises(binding.PcqError) as e:
                ctx.scan_dev_indexed_combined(cols, pred, ix, coll)
            assert e.value.code == -8
        assert cc.point_count() == 0
        gg.free(), cc.free()
    finally:
        ctx.index_free(ix)
        dev.free()
