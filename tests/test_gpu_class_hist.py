"""pcq_scan_dev_class_hist_batch: the class histogram of a box over many resident segments in one pass, every bin against numpy.

Segments of n = 0, 1, 511, 512, 513, 1535, 4133 points, the sizes of test_gpu_batch_multi.py (a step of the pipeline is 512
points), positions pieces 16-byte aligned in one buffer, class pieces carved at explicit byte phases so that 0, 1, 2 and 3 modulo
4 all occur among the non-empty segments.  Every segment has a box of its own.  Two points at (INT32_MIN,)*3 and two at
(INT32_MAX,)*3 are planted, one of each inside a whole step and one among a segment's leftover points.  The 512-point segment
carries its point index in x (20 where index % 5 == 0, 70 elsewhere, from a numpy table), so that a box is a stride test.  The
positions stay; each case uploads the class bytes it needs.  The counts are ADDED: every call starts from 256 distinct non-zero
device words and the test looks at the difference.
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
CLASS_PHASES = (0, 5, 2, 7, 8, 13, 3)  # byte phases of the class pieces in a 16-byte line: 1, 2, 3, 0, 1, 3 modulo 4 for the six non-empty segments
STRIDE_SEG = 3                          # the 512-point segment whose x encodes the point index
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
I32_MIN, I32_MAX = -2**31, 2**31 - 1
BINS = 256
PRESET = np.asarray([1000 + 7 * c for c in range(BINS)], dtype=np.uint64)
EMPTY = ([5, 5, 5], [4, 4, 4])
FULL = ([-2**40] * 3, [2**40] * 3)
FAR = ([2**31, 0, 0], [2**40, 99, 99])  # outside the i32 range on one axis


class Segments:
    def __init__(self, ctx):
        self.ctx = ctx
        rng = np.random.default_rng(2407)
        self.xyz = [rng.integers(0, 100, size=(n, 3), dtype=np.int32) for n in NS]
        self.keep5 = np.arange(NS[STRIDE_SEG]) % 5 == 0
        self.xyz[STRIDE_SEG][:, 0] = np.where(self.keep5, 20, 70)
        self.xyz[6][100] = I32_MIN   # inside a whole step
        self.xyz[4][512] = I32_MIN   # the one leftover point of a segment of 513
        self.xyz[6][3000] = I32_MAX  # inside a whole step
        self.xyz[5][1530] = I32_MAX  # among the 511 leftover points
        poff, psize = pp.carve(NS, [0] * len(NS), 12)
        self.coff, self.csize = pp.carve(NS, CLASS_PHASES)
        self.blocks = [ctx.alloc(psize + 64), ctx.alloc(self.csize + 64), ctx.alloc(8 * BINS)]
        d_pos, self.d_cls, self.d_hist = self.blocks
        assert all(p % 16 == 0 for p in self.blocks) and all(o % 16 == 0 for o in poff)
        phases = {(self.d_cls + o) % 4 for o, n in zip(self.coff, NS) if n}
        assert phases == {0, 1, 2, 3}, phases
        img = np.zeros(psize, dtype=np.uint8)
        for o, a in zip(poff, self.xyz):
            img[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
        ctx.to_device(d_pos, img)
        self.cols = [binding.make_columns(xyz=d_pos + p, cls=self.d_cls + c, n=n) for p, c, n in zip(poff, self.coff, NS)]
        self.cols_plain = [binding.make_columns(xyz=d_pos + p, n=n) for p, n in zip(poff, NS)]
        self.cls = None

    def set_classes(self, cls):
        """cls[k]: the class bytes of segment k; the gaps between the pieces hold 255 - a byte no case leaves unasserted"""
        assert [len(c) for c in cls] == list(NS)
        img = np.full(self.csize, 255, dtype=np.uint8)
        for o, c in zip(self.coff, cls):
            img[o:o + len(c)] = c
        self.ctx.to_device(self.d_cls, img)
        self.cls = [np.asarray(c, dtype=np.uint8) for c in cls]

    def box(self, k, visit=0):
        """The box of segment k.  Only segment 6 depends on the visit."""
        v = visit if k == 6 else 0
        return [10 + k, 5, 2 * k], [60 + k + 13 * v, 90, 99 - k]

    def want(self, boxes, segments=None):
        """numpy's histogram: bincount of the class bytes of the points inside each segment's box, summed over the segments"""
        h = np.zeros(BINS, dtype=np.int64)
        for k, (lo, hi) in zip(range(len(NS)) if segments is None else segments, boxes):
            h += np.bincount(self.cls[k][pp.in_box(self.xyz[k], lo, hi)], minlength=BINS)
        return h

    def preset(self):
        self.ctx.to_device(self.d_hist, PRESET)

    def words(self):
        out = np.zeros(BINS, dtype=np.uint64)
        self.ctx.to_host(out, self.d_hist)  # (waits for the context's stream)
        return out

    def added(self, boxes, segments=None):
        """One call from the preset words: what it ADDED to each of the 256 words"""
        cols = self.cols if segments is None else [self.cols[k] for k in segments]
        self.preset()
        self.ctx.scan_dev_class_hist_batch(cols, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], self.d_hist)
        return self.words().astype(np.int64) - PRESET.astype(np.int64)

    def check(self, boxes, segments=None):
        got, want = self.added(boxes, segments), self.want(boxes, segments)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, [(int(c), int(got[c]), int(want[c])) for c in bad[:12]]
        return want

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


@pytest.fixture(scope="module")
def segs(gpu_ctx):
    s = Segments(gpu_ctx)
    yield s
    s.free()


def random_classes(seed, values=None):
    rng = np.random.default_rng(seed)
    if values is None:
        return [rng.integers(0, 256, size=n, dtype=np.uint8) for n in NS]
    return [rng.choice(np.asarray(values, dtype=np.uint8), n) for n in NS]


def test_random_classes_over_all_bins(segs):
    segs.set_classes(random_classes(11))
    boxes = [segs.box(k) for k in range(len(NS))]
    want = segs.check(boxes)
    assert want[0] > 0 and want[255] > 0 and 0 < want.sum() < sum(NS)
    # with the full range every point is binned, the planted extremes among them
    want = segs.check([FULL] * len(NS))
    assert want.sum() == sum(NS)


def test_against_the_existing_batch_kernels(gpu_ctx, segs):
    few = (0, 1, 2, 5, 6, 9, 17, 255)
    segs.set_classes(random_classes(12, few))
    boxes = [segs.box(k) for k in range(len(NS))]
    hist = segs.added(boxes)
    assert np.array_equal(hist, segs.want(boxes))
    occur = [c for c in range(BINS) if hist[c]]
    assert occur == sorted(few)
    total = np.zeros(1, dtype=np.uint64)
    for c in occur + [3, 100, 254]:
        gpu_ctx.memset(segs.d_hist, 0, 8)
        gpu_ctx.scan_dev_count_batch_combined(segs.cols, [pkg.Predicate.bounds_class(lo, hi, c) for lo, hi in boxes], segs.d_hist)
        gpu_ctx.to_host(total, segs.d_hist)
        assert int(total[0]) == int(hist[c]), c
    gpu_ctx.memset(segs.d_hist, 0, 8)
    gpu_ctx.scan_dev_count_batch(segs.cols_plain, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], segs.d_hist)
    gpu_ctx.to_host(total, segs.d_hist)
    assert int(total[0]) == int(hist.sum()) > 0


def test_skewed_classes(segs):
    """Every lane adds to one bin (the LDS contention case), then three lanes of four."""
    segs.set_classes([np.full(n, 2, dtype=np.uint8) for n in NS])
    got = segs.added([FULL] * len(NS))
    assert got[2] == sum(NS) and not np.delete(got, 2).any(), (int(got[2]), np.flatnonzero(got).tolist())
    along, at = np.tile(np.asarray([2, 2, 2, 7], dtype=np.uint8), sum(NS) // 4 + 1), np.cumsum((0,) + NS)
    segs.set_classes([along[at[k]:at[k + 1]] for k in range(len(NS))])  # 2, 2, 2, 7 along the file
    want = segs.check([FULL] * len(NS))
    assert want[2] + want[7] == sum(NS) and want[7] == sum(NS) // 4


def test_position_inside_the_dword(segs):
    """class = point index mod 4 + 10 in every segment (so at every byte phase) and boxes that keep every point: bins 10..13 are
    exact, for the batch and for single segments with whole steps and leftover points.  A verdict brought to the wrong byte of a
    lane shows only where neighbouring points' verdicts differ, so a last call keeps a slab of y."""
    segs.set_classes([(np.arange(n) % 4 + 10).astype(np.uint8) for n in NS])
    want = segs.check([FULL] * len(NS))
    assert want[10:14].sum() == sum(NS) and list(want[10:14]) == [sum((n + 3 - i) // 4 for n in NS) for i in range(4)]
    for k in (4, 5, 6):
        want = segs.check([FULL], [k])
        assert list(want[10:14]) == [(NS[k] + 3 - i) // 4 for i in range(4)]
    want = segs.check([([0, 30, 0], [99, 60, 99])], [6])
    assert 0 < want.sum() < NS[6] and len({int(w) for w in want[10:14]}) > 1


def test_verdict_to_lane(segs):
    """One 512-point segment, class = point index mod 256, and a box that keeps exactly the points with index % 5 == 0 (x is 20
    there and 70 elsewhere): a verdict taken from the wrong load k or source lane lands in another bin."""
    k = STRIDE_SEG
    cls = [np.zeros(n, dtype=np.uint8) for n in NS]
    cls[k] = (np.arange(NS[k]) % 256).astype(np.uint8)
    segs.set_classes(cls)
    box = ([0, -10, -10], [50, 200, 200])
    assert np.array_equal(pp.in_box(segs.xyz[k], *box), segs.keep5)
    want = segs.check([box], [k])
    assert want.sum() == int(segs.keep5.sum()) == 103 and set(want.tolist()) == {0, 1}
    # the complement as well: every point with index % 5 != 0
    want = segs.check([([60, -10, -10], [80, 200, 200])], [k])
    assert want.sum() == NS[k] - 103


def test_empty_and_out_of_range_boxes(segs):
    segs.set_classes(random_classes(13))
    n = len(NS)
    odd = [EMPTY if k % 2 else segs.box(k) for k in range(n)]
    want = segs.check(odd)
    assert 0 < want.sum() < segs.want([segs.box(k) for k in range(n)]).sum()  # (the odd segments would have matched)
    far = [FAR if k == 6 else FULL for k in range(n)]
    want = segs.check(far)
    assert want.sum() == sum(NS) - NS[6]
    assert not segs.added([EMPTY] * n).any()
    assert not segs.added([FAR] * n).any()
    assert not segs.added([], []).any()  # nsegments == 0


def test_refusals_leave_the_histogram_alone(gpu_ctx, segs):
    segs.set_classes(random_classes(14))
    n = len(NS)
    boxes = [segs.box(k) for k in range(n)]
    segs.check(boxes)
    good = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
    segs.preset()

    def refused(cols, preds):
        with pytest.raises(binding.PcqError) as e:
            gpu_ctx.scan_dev_class_hist_batch(cols, preds, segs.d_hist)
        assert e.value.code == PCQ_ERR_ARG, e.value
        assert np.array_equal(segs.words(), PRESET)

    for bad in (pkg.Predicate.classification(2), pkg.Predicate.bounds_class(*boxes[3], 2)):
        preds = list(good)
        preds[3] = bad
        refused(segs.cols, preds)
    c = segs.cols[5]
    for bad in (binding.make_columns(xyz=c.xyz, cls=c.cls, n=100, xyz_stride=20),
                binding.make_columns(xyz=c.xyz + 4, cls=c.cls, n=c.n - 1),
                binding.make_columns(xyz=c.xyz, cls=None, n=100),
                binding.make_columns(xyz=c.xyz, cls=c.cls, n=100, cls_stride=2)):
        cols = list(segs.cols)
        cols[5] = bad
        refused(cols, good)
    # the table stored before the refusals serves the next good call
    segs.check(boxes)


def test_table_reuse_and_the_other_batches_in_between(gpu_ctx, segs):
    """Two calls in a row with one box changed (the table is uploaded only when it differs), then a box AND class batch — the
    same segment struct under another kind — and a multi-box batch on the same context, then the histogram again."""
    segs.set_classes(random_classes(15, (1, 2, 3, 200)))
    n = len(NS)
    sums = []
    for visit in (0, 1, 1, 0):
        sums.append(int(segs.check([segs.box(k, visit) for k in range(n)]).sum()))
    assert sums[0] == sums[3] != sums[1] == sums[2]
    boxes = [segs.box(k) for k in range(n)]
    total = np.zeros(2, dtype=np.uint64)

    def combined():
        gpu_ctx.memset(segs.d_hist, 0, 16)
        gpu_ctx.scan_dev_count_batch_combined(segs.cols, [pkg.Predicate.bounds_class(lo, hi, 2) for lo, hi in boxes], segs.d_hist)
        gpu_ctx.to_host(total, segs.d_hist)
        assert int(total[0]) == int(segs.want(boxes)[2]) > 0

    def multi():
        gpu_ctx.memset(segs.d_hist, 0, 16)
        rows = [[pkg.Predicate.bounds(lo, hi), pkg.Predicate.bounds(*FULL)] for lo, hi in boxes]
        gpu_ctx.scan_dev_count_batch_multi(segs.cols_plain, rows, segs.d_hist)
        gpu_ctx.to_host(total, segs.d_hist)
        assert [int(t) for t in total] == [int(segs.want(boxes).sum()), sum(NS)]

    for step in (combined, None, multi, None, combined, multi, None):
        if step is None:
            segs.check(boxes)
        else:
            step()
