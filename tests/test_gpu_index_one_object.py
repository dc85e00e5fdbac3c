"""The four indexed entries share one driver and one index object holds three parts (csrc/chunk_index.hip, csrc/index_plan.h):
all five predicate kinds on ONE pcq_index, in an order that holds every ordered pair of kinds, with count and buffer collectors
alternating — every result against pcq_scan_dev on a fresh collector, every call's statistics against a numpy model of the parts
and of the chunk states.  And the one behaviour that the shared driver changed: an uncovered BOUNDS / CLASS scan through
pcq_scan_dev_indexed leaves all-zero statistics, as the newer entries always did.

One column set of n = 65536 + 4096 + 17 points: seventeen bounds / time chunks of 4096, two class chunks (65536 and 4113 points),
a ragged tail of 17.
  positions  x = the point's number (sorted by x), y and z small and random
  times      1000 + 0.01 x, ascending; chunk 13 all NaN, one NaN in chunk 12, one in the tail
  classes    class chunk 0 all class 2; class chunk 1 (with the tail) classes 2 and 5 mixed
The box is x >= 60000 (chunk 14 straddles, 15 and 16 and the tail are inside), the range [t(40000), 1e9) (chunk 9 straddles, 12
has its NaN, 13 is NaN, the rest behind are inside).  A class scan has two chunks only, which cannot show three states at once:
it asks for class 2 (ALL, SCAN) and class 5 (NONE, SCAN) in turn.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _bounds_time_index_model as bm  # noqa: E402
import _time_index_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
CH, CLASS_CH = 4096, 65536
NONE, SCAN, ALL = bm.NONE, bm.SCAN, bm.ALL
N = CLASS_CH + CH + 17
CHUNKS, CLASS_CHUNKS = N // CH, (N + CLASS_CH - 1) // CLASS_CH
LO, HI = [60000, -2**31, -2**31], [2**31 - 1, 2**31 - 1, 2**31 - 1]
T0, T1 = 1000.0 + 0.01 * 40000, 1e9
BOUNDS, CLASS, BOUNDS_CLASS, TIME, BOUNDS_TIME = range(5)
PARTS = {BOUNDS: {"boxes"}, CLASS: {"hist"}, BOUNDS_CLASS: {"boxes", "hist"}, TIME: {"times"}, BOUNDS_TIME: {"boxes", "times"}}
ORDER = [0, 0, 1, 0, 2, 0, 3, 0, 4, 1, 1, 2, 1, 3, 1, 4, 2, 2, 3, 2, 4, 3, 3, 4, 4, 0]


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


def build():
    rng = np.random.default_rng(20261019)
    i = np.arange(N)
    xyz = np.stack([i, rng.integers(-100, 101, N), rng.integers(-100, 101, N)], axis=1).astype(np.int32)
    t = 1000.0 + 0.01 * i
    t[13 * CH: 14 * CH] = np.nan
    t[12 * CH + 1234] = np.nan
    t[CHUNKS * CH + 5] = np.nan
    cls = np.full(N, 2, dtype=np.uint8)
    cls[CLASS_CH:] = np.where(rng.integers(0, 2, N - CLASS_CH) == 1, 5, 2)
    return xyz, t, cls


def class_states(cls, c):
    out = []
    for k in range(CLASS_CHUNKS):
        part = cls[CLASS_CH * k: CLASS_CH * (k + 1)]
        hits = int((part == c).sum())
        out.append(NONE if hits == 0 else (ALL if hits == len(part) else SCAN))
    return out


def states(kind, data, c):
    """The chunk states of one kind's query: per class chunk for CLASS, per 4096-point chunk for the others."""
    xyz, t, cls = data
    box = [bm.box_state(xyz[CH * k: CH * (k + 1)], LO, HI) for k in range(CHUNKS)]
    if kind == BOUNDS:
        return box
    if kind == CLASS:
        return class_states(cls, c)
    if kind == BOUNDS_CLASS:
        cs = class_states(cls, c)
        return [bm.combined(box[k], cs[k * CH // CLASS_CH]) for k in range(CHUNKS)]
    if kind == TIME:
        return tm.states(t, T0, T1)
    return bm.states(xyz, t, LO, HI, T0, T1)


def counts3(s):
    return s.count(NONE), s.count(ALL), s.count(SCAN)


def checked_data():
    """The column set, with the construction asserted on the model alone, before any GPU call."""
    data = build()
    xyz, t, cls = data
    assert len(xyz) == len(t) == len(cls) == N and CHUNKS == 17 and CLASS_CHUNKS == 2 and N - CHUNKS * CH == 17
    assert np.all(np.diff(xyz[:, 0]) > 0)
    ok = ~np.isnan(t)
    assert np.all(np.diff(t[ok]) > 0) and np.isnan(t[13 * CH: 14 * CH]).all() and int(np.isnan(t[12 * CH: 13 * CH]).sum()) == 1
    assert int(np.isnan(t[CHUNKS * CH:]).sum()) == 1 and int(np.isnan(t).sum()) == CH + 2
    assert class_states(cls, 2) == [ALL, SCAN] and class_states(cls, 5) == [NONE, SCAN]
    # every kind's query meets all three chunk states (CLASS: its two queries between them)
    for kind in (BOUNDS, BOUNDS_CLASS, TIME, BOUNDS_TIME):
        assert set(states(kind, data, 2)) == {NONE, SCAN, ALL}, kind
    assert set(states(CLASS, data, 2)) | set(states(CLASS, data, 5)) == {NONE, SCAN, ALL}
    assert states(BOUNDS, data, 2)[13:] == [NONE, SCAN, ALL, ALL]
    assert states(BOUNDS_CLASS, data, 2)[13:] == [NONE, SCAN, ALL, SCAN]       # chunk 16 lies in the mixed class chunk
    assert states(TIME, data, 2)[8:] == [NONE, SCAN, ALL, ALL, SCAN, NONE, ALL, ALL, ALL]
    assert states(BOUNDS_TIME, data, 2)[12:] == [NONE, NONE, SCAN, ALL, ALL]
    # the tail has matches of its own, and not all of its points match
    tail = slice(CHUNKS * CH, N)
    assert 0 < int((cls[tail] == 2).sum()) < 17 and 0 < int((cls[tail] == 5).sum()) < 17
    assert int(bm.select(xyz[tail], t[tail], LO, HI, T0, T1).sum()) == 16
    return data


@pytest.fixture(scope="module")
def data():
    return checked_data()


def test_the_order_holds_every_ordered_pair_of_kinds():
    assert len(ORDER) == 26 and {(a, b) for a, b in zip(ORDER, ORDER[1:])} == {(a, b) for a in range(5) for b in range(5)}


def predicate(kind, c):
    return [pkg.Predicate.bounds(LO, HI), pkg.Predicate.classification(c), pkg.Predicate.bounds_class(LO, HI, c),
            pkg.Predicate.time_range(T0, T1), pkg.Predicate.bounds_time(LO, HI, T0, T1)][kind]


def result(g, coll):
    return g.point_count() if coll == "count" else g.points().tobytes()


@pytest.mark.parametrize("first", ["count", "buffer"])
def test_all_five_kinds_on_one_index_object(gpu_ctx, data, first):
    """first = count: the 1st, 3rd, ... calls count and the others collect records; first = buffer: the other way round, so that
    every kind meets its building call and its later calls with both collectors between the two cases."""
    ctx = gpu_ctx
    xyz, t, cls = data
    dev, ix = Dev(ctx), ctx.index_new()
    try:
        d_xyz = dev.put(xyz)
        ccols = binding.make_columns(xyz=d_xyz, cls=dev.put(cls, pad=3), n=N)  # (class bytes at any alignment)
        tcols = binding.make_columns(xyz=d_xyz, cls=dev.put(t), n=N, cls_stride=8)
        entries = [ctx.scan_dev_indexed, ctx.scan_dev_indexed, ctx.scan_dev_indexed_combined, ctx.scan_dev_indexed_time,
                   ctx.scan_dev_indexed_bounds_time]
        plain = {}  # pcq_scan_dev on a fresh collector, once per (kind, class, collector)
        have = set()
        class_calls = 0
        for call, kind in enumerate(ORDER):
            coll = ("count", "buffer")[(call + (first == "buffer")) % 2]
            c = 2
            if kind == CLASS:
                c = (2, 5)[class_calls % 2]
                class_calls += 1
            cols, pred = (tcols if kind in (TIME, BOUNDS_TIME) else ccols), predicate(kind, c)
            if (kind, c, coll) not in plain:
                g = ctx.count_collector() if coll == "count" else ctx.buffer_collector()
                ctx.scan_dev(cols, pred, g)
                plain[(kind, c, coll)] = result(g, coll)
                g.free()
            g = ctx.count_collector() if coll == "count" else ctx.buffer_collector()
            entries[kind](cols, pred, ix, g)
            got = result(g, coll)
            g.free()
            st = ctx.index_stats(ix)
            what = (call, kind, coll, c, st)
            assert got == plain[(kind, c, coll)], what
            assert (got if coll == "count" else len(got)) > 0, what
            # the model: which parts exist, and the states of the chunks
            missing = not PARTS[kind] <= have
            have |= PARTS[kind]
            chunks = CLASS_CHUNKS if kind == CLASS else CHUNKS
            if missing and len(PARTS[kind]) == 1:       # the build of the one part read every chunk
                want = (0, 0, chunks)
            elif kind == CLASS and coll == "count":     # answered from the histograms
                want = (0, chunks, 0)
            else:
                want = counts3(states(kind, data, c))
            assert st == dict(chunks=chunks, skipped=want[0], whole=want[1], scanned=want[2], built=int(missing)), (what, want)
        assert have == {"boxes", "hist", "times"} and class_calls == ORDER.count(CLASS) >= 2
    finally:
        ctx.index_free(ix)
        dev.free()


def test_an_uncovered_bounds_or_class_scan_zeroes_the_statistics_and_leaves_the_parts(gpu_ctx, data):
    ctx = gpu_ctx
    xyz, t, cls = data
    dev, ix = Dev(ctx), ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(cls), n=N)
        bpred, cpred = pkg.Predicate.bounds(LO, HI), pkg.Predicate.classification(5)
        want_b = int(np.all((xyz >= np.asarray(LO, dtype=np.int64)) & (xyz <= np.asarray(HI, dtype=np.int64)), axis=1).sum())
        want_c = int((cls == 5).sum())
        box3 = counts3(states(BOUNDS, data, 2))

        def count(c, p):
            g = ctx.count_collector()
            ctx.scan_dev_indexed(c, p, ix, g)
            got = g.point_count()
            g.free()
            return got

        def covered(built):  # a covered bounds count: statistics that are not zero, of parts that were there
            assert count(cols, bpred) == want_b
            st = ctx.index_stats(ix)
            want = (0, 0, CHUNKS) if built else box3
            assert st == dict(chunks=CHUNKS, skipped=want[0], whole=want[1], scanned=want[2], built=built), st

        covered(1)
        covered(0)
        assert count(cols, cpred) == want_c and ctx.index_stats(ix)["built"] == 1   # the histograms exist as well
        covered(0)
        # positions 4 bytes off alignment
        off = binding.make_columns(xyz=dev.put(xyz, pad=4), cls=cols.cls, n=N)
        assert count(off, bpred) == want_b
        assert not any(ctx.index_stats(ix).values())
        covered(0)
        # fewer points than one chunk
        few = binding.make_columns(xyz=cols.xyz, cls=cols.cls, n=100)
        assert count(few, pkg.Predicate.bounds([0, -2**31, -2**31], [49, 2**31 - 1, 2**31 - 1])) == 50
        assert not any(ctx.index_stats(ix).values())
        covered(0)
        # class bytes inside 34-byte records
        rec = np.zeros((N, 34), dtype=np.uint8)
        rec[:, 15] = cls
        p = dev.put(rec)
        las = binding.make_columns(xyz=p, cls=p + 15, n=N, xyz_stride=34, cls_stride=34)
        assert count(las, cpred) == want_c
        assert not any(ctx.index_stats(ix).values())
        covered(0)
        assert count(cols, cpred) == want_c
        assert ctx.index_stats(ix) == dict(chunks=CLASS_CHUNKS, skipped=0, whole=CLASS_CHUNKS, scanned=0, built=0)
    finally:
        ctx.index_free(ix)
        dev.free()
