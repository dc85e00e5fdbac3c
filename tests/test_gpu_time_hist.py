"""pcq_scan_dev_time_hist_batch: the time histogram of a box over many resident segments in one pass, every bin against numpy.

Segments of n = 0, 1, 511, 512, 513, 1535, 4133 points, the sizes of test_gpu_class_hist.py (a step of the pipeline is 512 points),
positions pieces 16-byte aligned in one buffer, time pieces carved at 8-byte offsets so that both 0 and 8 modulo 16 occur among the
non-empty segments.  Every segment has a box of its own.  Two points at (INT32_MIN,)*3 and two at (INT32_MAX,)*3 are planted, one
of each inside a whole step and one among a segment's leftover points.  The 512-point segment carries its point index in x (20
where index % 5 == 0, 70 elsewhere, from a numpy table), so that a box is a stride test.  The positions stay; each case uploads
the times it needs.  Expected values are plain numpy compares per bin: in_box & (t >= e[b]) & (t < e[b + 1]).  The counts are ADDED:
every call starts from PCQ_TIME_BINS_MAX + 8 distinct non-zero device words, and the test looks at the difference and at the words
from nbins on, which must be unchanged.
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

NS = (0, 1, 511, 512, 513, 1535, 4133)
TIME_PHASES = (0, 8, 0, 8, 0, 8, 0)  # byte phases of the time pieces in a 16-byte line
STRIDE_SEG = 3                        # the 512-point segment whose x encodes the point index
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
I32_MIN, I32_MAX = -2**31, 2**31 - 1
BINS_MAX = 1024                       # include/pcq.h: PCQ_TIME_BINS_MAX
WORDS = BINS_MAX + 8
PRESET = np.asarray([1000 + 7 * c for c in range(WORDS)], dtype=np.uint64)
EMPTY = ([5, 5, 5], [4, 4, 4])
FULL = ([-2**40] * 3, [2**40] * 3)
FAR = ([2**31, 0, 0], [2**40, 99, 99])  # outside the i32 range on one axis
NAN, INF = float("nan"), float("inf")
DENORMAL = 5e-324


def numpy_hist(t, edges):
    """Per bin: (t >= e[b]) & (t < e[b + 1]), counted.  No histogram or search routine."""
    e = np.asarray(edges, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.asarray([int(((t >= e[b]) & (t < e[b + 1])).sum()) for b in range(len(e) - 1)], dtype=np.int64)


class Segments:
    def __init__(self, ctx):
        self.ctx = ctx
        rng = np.random.default_rng(2411)
        self.xyz = [rng.integers(0, 100, size=(n, 3), dtype=np.int32) for n in NS]
        self.keep5 = np.arange(NS[STRIDE_SEG]) % 5 == 0
        self.xyz[STRIDE_SEG][:, 0] = np.where(self.keep5, 20, 70)
        self.xyz[6][100] = I32_MIN   # inside a whole step
        self.xyz[4][512] = I32_MIN   # the one leftover point of a segment of 513
        self.xyz[6][3000] = I32_MAX  # inside a whole step
        self.xyz[5][1530] = I32_MAX  # among the 511 leftover points
        poff, psize = pp.carve(NS, [0] * len(NS), 12)
        self.toff, self.tsize = pp.carve(NS, TIME_PHASES, 8)
        self.blocks = [ctx.alloc(psize + 64), ctx.alloc(self.tsize + 64), ctx.alloc(8 * WORDS), ctx.alloc(64)]
        d_pos, self.d_t, self.d_hist, self.d_total = self.blocks
        assert all(p % 16 == 0 for p in self.blocks) and all(o % 16 == 0 for o in poff)
        phases = {(self.d_t + o) % 16 for o, n in zip(self.toff, NS) if n}
        assert phases == {0, 8}, phases
        img = np.zeros(psize, dtype=np.uint8)
        for o, a in zip(poff, self.xyz):
            img[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
        ctx.to_device(d_pos, img)
        self.cols = [binding.make_columns(xyz=d_pos + p, cls=self.d_t + c, n=n, cls_stride=8) for p, c, n in zip(poff, self.toff, NS)]
        self.t = None

    def set_times(self, t):
        """t[k]: the times of segment k; the gaps between the pieces hold 12345.0"""
        assert [len(a) for a in t] == list(NS)
        img = np.full(self.tsize // 8 + 2, 12345.0, dtype=np.float64).view(np.uint8)[:self.tsize].copy()
        for o, a in zip(self.toff, t):
            a = np.ascontiguousarray(a, dtype=np.float64)
            img[o:o + a.nbytes] = a.view(np.uint8)
        self.ctx.to_device(self.d_t, img)
        self.t = [np.asarray(a, dtype=np.float64) for a in t]

    def box(self, k):
        return [10 + k, 5, 2 * k], [60 + k, 90, 99 - k]

    def passing(self, boxes, segments=None):
        """The times of the points inside each segment's box, in one array"""
        ks = range(len(NS)) if segments is None else segments
        return np.concatenate([self.t[k][pp.in_box(self.xyz[k], lo, hi)] for k, (lo, hi) in zip(ks, boxes)] + [np.zeros(0)])

    def want(self, boxes, edges, segments=None):
        return numpy_hist(self.passing(boxes, segments), edges)

    def words(self):
        out = np.zeros(WORDS, dtype=np.uint64)
        self.ctx.to_host(out, self.d_hist)  # (waits for the context's stream)
        return out

    def added(self, boxes, edges, segments=None):
        """One call from the preset words: what it ADDED to each of the nbins words; the words behind them are unchanged"""
        cols = self.cols if segments is None else [self.cols[k] for k in segments]
        self.ctx.to_device(self.d_hist, PRESET)
        self.ctx.scan_dev_time_hist_batch(cols, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], edges, self.d_hist)
        got = self.words()
        nbins = len(edges) - 1
        assert np.array_equal(got[nbins:], PRESET[nbins:]), np.flatnonzero(got != PRESET)[-8:]
        return got[:nbins].astype(np.int64) - PRESET[:nbins].astype(np.int64)

    def check(self, boxes, edges, segments=None):
        got, want = self.added(boxes, edges, segments), self.want(boxes, edges, segments)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, [(int(b), int(got[b]), int(want[b])) for b in bad[:12]]
        return want

    def range_count(self, boxes, start, end):
        """pcq_scan_dev_count_batch_bounds_time on the same columns"""
        self.ctx.memset(self.d_total, 0, 8)
        self.ctx.scan_dev_count_batch_bounds_time(self.cols, [pkg.Predicate.bounds_time(lo, hi, start, end) for lo, hi in boxes], self.d_total)
        out = np.zeros(1, dtype=np.uint64)
        self.ctx.to_host(out, self.d_total)
        return int(out[0])

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


@pytest.fixture(scope="module")
def segs(gpu_ctx):
    s = Segments(gpu_ctx)
    yield s
    s.free()


def own_boxes(segs):
    return [segs.box(k) for k in range(len(NS))]


def random_times(seed, lo=900.0, hi=2100.0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(lo, hi, n) for n in NS]


def random_edges(seed, nbins, lo=1000.0, hi=2000.0):
    return np.sort(np.random.default_rng(seed).uniform(lo, hi, nbins + 1))


@pytest.mark.parametrize("nbins", [1, 2, 3, 63, 64, 65, 1023, 1024])
def test_random_sorted_edges(segs, nbins):
    """Times in [900, 2100), edges in [1000, 2000): points below the first edge and at or above the last one among them."""
    segs.set_times(random_times(20 + nbins))
    edges = random_edges(40 + nbins, nbins)
    want = segs.check(own_boxes(segs), edges)
    every = segs.passing(own_boxes(segs))
    assert 0 < want.sum() < len(every) < sum(NS) and (every < edges[0]).any() and (every >= edges[-1]).any()
    # with the full range every point is looked at, the planted extremes among them
    want = segs.check([FULL] * len(NS), edges)
    assert len(segs.passing([FULL] * len(NS))) == sum(NS) and want.sum() > 0
    if nbins >= 63:
        assert np.count_nonzero(want) > nbins // 2 and want[0] + want[-1] > 0


def test_every_passing_point_of_a_large_segment_shares_one_time(segs):
    """All lanes add to one bin (the LDS contention case), in whole steps and among the leftovers."""
    t = random_times(61)
    t[6] = np.full(NS[6], 1500.0)
    segs.set_times(t)
    for edges in (np.asarray([1000.0, 1400.0, 1500.0, 1600.0]), np.linspace(1000.0, 2000.0, 1025), np.asarray([1500.0, np.nextafter(1500.0, INF)])):
        want = segs.check([FULL], edges, [6])
        assert want.sum() == NS[6] and np.count_nonzero(want) == 1
        assert edges[np.flatnonzero(want)[0]] == 1500.0  # the bin that STARTS at the shared time
        segs.check(own_boxes(segs), edges)
    assert not segs.check([FULL], np.asarray([1000.0, 1500.0]), [6]).any()  # the bin that ENDS there


def special_pool(edges):
    e = np.asarray(edges, dtype=np.float64)
    pool = [NAN, INF, -INF, -0.0, 0.0, DENORMAL, -DENORMAL]
    pool += list(e) + list(np.nextafter(e, -INF)) + list(np.nextafter(e, INF))
    finite = e[np.isfinite(e)]
    if len(finite):
        pool += [finite.min() - 1.0, finite.min() - 1e9, finite.max() + 1.0, finite.max() + 1e9]
    return np.asarray(pool, dtype=np.float64)


EDGE_TABLES = {
    "plain": [1.0, 2.0, 3.0, 5.0, 8.0],
    "equal_neighbours": [1.0, 2.0, 2.0, 3.0, 4.0, 4.0, 4.0, 5.0],       # a pair and a run of three
    "all_equal": [7.0, 7.0, 7.0],
    "inf_first_and_last": [-INF, -1.0, 0.0, 1.0, INF],
    "inf_in_the_middle": [0.0, 1.0, INF, INF],
    "inf_only": [-INF, INF],
    "both_zeros": [-0.0, 0.0, 1.0],
    "zeros_reversed": [-1.0, 0.0, -0.0, 1.0],                              # (0.0 <= -0.0 under IEEE compares: non-decreasing)
    "denormals": [-DENORMAL, 0.0, DENORMAL, 1.0],
    "negative_first": [-INF, -INF, -5.0, -0.0],
}


@pytest.mark.parametrize("name", list(EDGE_TABLES))
def test_special_times_and_edge_tables(segs, name):
    """Times drawn from NaN, the infinities, both zeros, denormals, every edge, the doubles next to every edge, and values
    outside the table.  Every bin is numpy's compare, and the definition's corollaries are pinned one by one."""
    edges = np.asarray(EDGE_TABLES[name], dtype=np.float64)
    nbins = len(edges) - 1
    pool = special_pool(edges)
    rng = np.random.default_rng(70 + len(name))
    t = [rng.choice(pool, n) for n in NS]
    for k in (2, 6):  # every pool value at least once in a segment with leftovers only and in one with whole steps
        t[k][:len(pool)] = pool
    segs.set_times(t)
    boxes = [FULL] * len(NS)
    got = segs.added(boxes, edges)
    every = segs.passing(boxes)
    assert np.array_equal(got, segs.want(boxes, edges))
    with np.errstate(invalid="ignore"):
        # a NaN time, a time below e[0] and a time at or above e[nbins] land in no bin: the sum is the others
        assert got.sum() == int(((every >= edges[0]) & (every < edges[-1])).sum())
        assert np.isnan(every).sum() > 0 and (every == INF).sum() > 0 and (every == -INF).sum() > 0
        for b in range(nbins):
            if edges[b] == edges[b + 1]:
                assert got[b] == 0, (b, "a bin with equal edges stays empty")
            elif np.isfinite(edges[b]) or edges[b] == -INF:
                # a time equal to an edge belongs to the bin that starts there (the last such bin where edges repeat)
                assert got[b] >= int((every == edges[b]).sum()) > 0, b
        if edges[-1] == INF:
            assert (every == INF).sum() > 0  # ... and +inf is in no bin whose end is +inf: covered by the sum above
    if name == "both_zeros":
        zeros = int((every == 0.0).sum())  # (-0.0 == 0.0)
        assert np.signbit(every[every == 0.0]).any() and not np.signbit(every[every == 0.0]).all()
        assert got[0] == 0 and got[1] >= zeros > 0
    if name == "inf_only":
        assert got[0] == int(np.isfinite(every).sum()) + int((every == -INF).sum())
    # the own boxes as well
    segs.check(own_boxes(segs), edges)


@pytest.mark.parametrize("nbins", [1, 2, 3, 8])
def test_every_bin_against_the_box_and_time_count(segs, nbins):
    segs.set_times(random_times(80 + nbins))
    edges = random_edges(90 + nbins, nbins)
    boxes = own_boxes(segs)
    want = segs.check(boxes, edges)
    for b in range(nbins):
        assert segs.range_count(boxes, float(edges[b]), float(edges[b + 1])) == int(want[b]), b
    edges = np.asarray(EDGE_TABLES["equal_neighbours"])
    want = segs.check(boxes, edges)
    for b in range(len(edges) - 1):
        assert segs.range_count(boxes, float(edges[b]), float(edges[b + 1])) == int(want[b]), b


def test_verdict_to_lane(segs):
    """One 512-point segment, time = point index, one bin per index, and a box that keeps exactly the points with index % 5 == 0
    (x is 20 there and 70 elsewhere): a verdict taken from the wrong load, source lane or dword lands in another bin."""
    k = STRIDE_SEG
    t = [np.zeros(n) for n in NS]
    t[k] = np.arange(NS[k], dtype=np.float64)
    segs.set_times(t)
    edges = np.arange(NS[k] + 1, dtype=np.float64)
    box = ([0, -10, -10], [50, 200, 200])
    assert np.array_equal(pp.in_box(segs.xyz[k], *box), segs.keep5)
    want = segs.check([box], edges, [k])
    assert np.array_equal(want, segs.keep5.astype(np.int64)) and want.sum() == 103
    want = segs.check([([60, -10, -10], [80, 200, 200])], edges, [k])  # the complement
    assert np.array_equal(want, (~segs.keep5).astype(np.int64))
    # the same in every segment, whole steps and leftovers: time = index mod 512, own boxes
    segs.set_times([(np.arange(n) % 512).astype(np.float64) for n in NS])
    want = segs.check(own_boxes(segs), edges)
    assert 0 < want.sum() < sum(NS) and len(set(want.tolist())) > 2


def test_empty_and_out_of_range_boxes_and_subsets(segs):
    segs.set_times(random_times(101))
    edges = random_edges(102, 16)
    n = len(NS)
    odd = [EMPTY if k % 2 else segs.box(k) for k in range(n)]
    want = segs.check(odd, edges)
    assert 0 < want.sum() < segs.want(own_boxes(segs), edges).sum()  # (the odd segments would have matched)
    far = [FAR if k == 6 else FULL for k in range(n)]
    want_far = segs.check(far, edges)
    assert 0 < want_far.sum() < segs.want([FULL] * n, edges).sum()
    assert not segs.added([EMPTY] * n, edges).any()
    assert not segs.added([FAR] * n, edges).any()
    assert not segs.added([], edges, []).any()  # nsegments == 0
    for subset in ([6], [5], [1], [0], [2, 4], [6, 3, 1], [0, 1, 2], list(range(n))[::-1]):
        segs.check([segs.box(k) for k in subset], edges, subset)


def test_new_edges_in_the_same_host_buffer(gpu_ctx, segs):
    """Two calls in a row with the same segments and the same host buffer holding other edges: a cache keyed on the buffer's
    address, or on the segment table alone, answers the second call with the first call's bins.  Then other batches on the same
    context in between."""
    segs.set_times(random_times(111))
    boxes = own_boxes(segs)
    edges = random_edges(112, 8)
    first = segs.check(boxes, edges)
    edges[:] = random_edges(113, 8)  # in place
    second = segs.check(boxes, edges)
    assert not np.array_equal(first, second)
    assert np.array_equal(segs.check(boxes, edges), second)  # unchanged edges: the stored table serves
    edges[3] = np.nextafter(edges[3], INF)  # one bit of one edge
    segs.check(boxes, edges)
    # fewer and more bins over the same segments, in both orders
    for nbins in (4, 8, 1024, 5, 1023, 8):
        segs.check(boxes, random_edges(114, nbins))
    for _ in range(2):
        assert segs.range_count(boxes, 1000.0, 2000.0) == int(segs.want(boxes, [1000.0, 2000.0])[0])
        segs.check(boxes, edges)


def test_refusals_leave_the_words_alone(gpu_ctx, segs):
    segs.set_times(random_times(121))
    n = len(NS)
    boxes = own_boxes(segs)
    edges = random_edges(122, 8)
    segs.check(boxes, edges)
    good = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
    gpu_ctx.to_device(segs.d_hist, PRESET)

    def refused(cols, preds, e):
        with pytest.raises(binding.PcqError) as err:
            gpu_ctx.scan_dev_time_hist_batch(cols, preds, e, segs.d_hist)
        assert err.value.code == PCQ_ERR_ARG, err.value
        assert np.array_equal(segs.words(), PRESET)

    refused(segs.cols, good, np.asarray([1.0]))                              # nbins == 0
    refused(segs.cols, good, np.arange(BINS_MAX + 2, dtype=np.float64))      # PCQ_TIME_BINS_MAX + 1
    refused([], [], np.asarray([1.0]))                                       # ... also without segments
    refused([], [], np.asarray([1.0, NAN]))
    for bad in ([NAN, 2.0, 3.0], [1.0, NAN, 3.0], [1.0, 2.0, NAN], [2.0, 1.0, 3.0], [1.0, 3.0, 2.0], [INF, -INF]):
        refused(segs.cols, good, np.asarray(bad))
    for bad in (pkg.Predicate.bounds_time(*boxes[3], 1000.0, 2000.0), pkg.Predicate.time_range(1000.0, 2000.0)):
        preds = list(good)
        preds[3] = bad
        refused(segs.cols, preds, edges)
    c = segs.cols[5]
    for bad in (binding.make_columns(xyz=c.xyz, cls=c.cls, n=100, cls_stride=1),
                binding.make_columns(xyz=c.xyz, cls=c.cls + 4, n=100, cls_stride=8),
                binding.make_columns(xyz=c.xyz, cls=None, n=100, cls_stride=8),
                binding.make_columns(xyz=c.xyz + 4, cls=c.cls, n=c.n - 1, cls_stride=8),
                binding.make_columns(xyz=c.xyz, cls=c.cls, n=100, cls_stride=8, xyz_stride=20)):
        cols = list(segs.cols)
        cols[5] = bad
        refused(cols, good, edges)
    # the table stored before the refusals serves the next good call
    segs.check(boxes, edges)
