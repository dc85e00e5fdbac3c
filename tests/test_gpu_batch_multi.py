"""pcq_scan_dev_count_batch_multi: up to eight boxes asked of many resident segments in one pass, every per-query total against
numpy int64 compares.

Segments of n = 0, 1, 511, 512, 513, 1535, 4133 points, the sizes of test_gpu_batch_kinds.py (a step of the pipeline is 512
points), positions pieces 16-byte aligned in one buffer.  Every (segment, query) pair has a box of its own, derived from k and
q.  Two points at (INT32_MIN,)*3 and two at (INT32_MAX,)*3 are planted, one of each inside a whole step and one among a
segment's leftover points.  The totals are ADDED: every call starts from distinct non-zero device words.
"""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

NS = (0, 1, 511, 512, 513, 1535, 4133)
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
I32_MIN, I32_MAX = -2**31, 2**31 - 1
VARIED = (6, 2)  # the (segment, query) whose box changes from one call to the next
PRESET = [1000 + 7 * q for q in range(8)]
EMPTY = ([5, 5, 5], [4, 4, 4])
FULL = ([-2**40] * 3, [2**40] * 3)


def in_box(xyz, lo, hi):
    x = xyz.astype(np.int64)
    return np.all((x >= np.asarray(lo, dtype=np.int64)) & (x <= np.asarray(hi, dtype=np.int64)), axis=1)


class Segments:
    def __init__(self, ctx):
        self.ctx = ctx
        rng = np.random.default_rng(2203)
        self.xyz = [rng.integers(0, 100, size=(n, 3), dtype=np.int32) for n in NS]
        self.cls = [rng.integers(1, 4, size=n, dtype=np.uint8) for n in NS]
        self.xyz[6][100] = I32_MIN   # inside a whole step
        self.xyz[4][512] = I32_MIN   # the one leftover point of a segment of 513
        self.xyz[6][3000] = I32_MAX  # inside a whole step
        self.xyz[5][1530] = I32_MAX  # among the 511 leftover points
        poff, at = [], 0
        for n in NS:
            poff.append(at)
            at += (12 * n + 64 + 15) // 16 * 16
        self.blocks = [ctx.alloc(at + 64), ctx.alloc(sum(NS) + 64), ctx.alloc(128)]
        d_pos, d_cls, self.d_totals = self.blocks
        assert all(p % 16 == 0 for p in self.blocks) and all(o % 16 == 0 for o in poff)
        img = np.zeros(at, dtype=np.uint8)
        for o, a in zip(poff, self.xyz):
            img[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
        ctx.to_device(d_pos, img)
        ctx.to_device(d_cls, np.concatenate(self.cls))
        coff = np.cumsum((0,) + NS[:-1])
        self.cols = [binding.make_columns(xyz=d_pos + p, n=n) for p, n in zip(poff, NS)]
        self.cols_class = [binding.make_columns(xyz=d_pos + p, cls=d_cls + int(c), n=n) for p, c, n in zip(poff, coff, NS)]

    def box(self, k, q, visit=0):
        """The box of segment k under query q.  Only VARIED depends on the visit."""
        v = visit if (k, q) == VARIED else 0
        return [10 + k + q, 5, 2 * q], [60 + k - 3 * q + 13 * v, 90, 99 - q]

    def rows(self, boxes):
        """boxes[k][q] -> the predicate rows and numpy's per-query totals"""
        rows = [[pkg.Predicate.bounds(lo, hi) for lo, hi in row] for row in boxes]
        nq = len(boxes[0])
        want = [sum(int(in_box(self.xyz[k], *boxes[k][q]).sum()) for k in range(len(NS))) for q in range(nq)]
        return rows, want

    def preset(self):
        self.ctx.to_device(self.d_totals, np.asarray(PRESET, dtype=np.uint64))

    def totals(self):
        out = np.zeros(8, dtype=np.uint64)
        self.ctx.to_host(out, self.d_totals)  # (waits for the context's stream)
        return [int(x) for x in out]

    def multi(self, boxes):
        """One call from the preset words: what it ADDED to each of the eight words, and numpy's answer"""
        rows, want = self.rows(boxes)
        self.preset()
        self.ctx.scan_dev_count_batch_multi(self.cols, rows, self.d_totals)
        got = [t - p for t, p in zip(self.totals(), PRESET)]
        return got, want + [0] * (8 - len(want))

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


@pytest.fixture(scope="module")
def segs(gpu_ctx):
    s = Segments(gpu_ctx)
    yield s
    s.free()


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 7, 8])
def test_every_pair_has_its_own_box(segs, nq):
    boxes = [[segs.box(k, q) for q in range(nq)] for k in range(len(NS))]
    got, want = segs.multi(boxes)
    assert all(w > 0 for w in want[:nq]) and len(set(want[:nq])) == nq, want
    assert got == want, f"nqueries {nq}: got - want = {[g - w for g, w in zip(got, want)]}"


def test_empty_identical_full_and_one_point_boxes(segs):
    """q0 empty everywhere, q1 empty in the odd segments, q2 == q3, q4 the full i32 range, q5 / q6 one point at INT32_MIN /
    INT32_MAX, q7 an ordinary box."""
    boxes = []
    for k in range(len(NS)):
        same = segs.box(k, 2)
        boxes.append([EMPTY, EMPTY if k % 2 else segs.box(k, 1), same, same, FULL, ([I32_MIN] * 3, [I32_MIN] * 3), ([I32_MAX] * 3, [I32_MAX] * 3),
                      segs.box(k, 7)])
    got, want = segs.multi(boxes)
    assert want[0] == 0 and want[1] > 0 and want[2] == want[3] > 0 and want[4] == sum(NS) and want[5] == 2 and want[6] == 2 and want[7] > 0
    assert want[1] < segs.rows([[segs.box(k, 1)] for k in range(len(NS))])[1][0]  # (the odd segments would have matched)
    assert got == want, [g - w for g, w in zip(got, want)]
    # the same boxes outside the i32 range on one axis: empty as well
    far = [[([2**31, 0, 0], [2**40, 99, 99]), FULL] for _ in NS]
    got, want = segs.multi(far)
    assert want[:2] == [0, sum(NS)] and got == want


def test_table_reuse_and_the_other_batches_in_between(gpu_ctx, segs):
    """Two calls in a row with one predicate changed (the table is uploaded only when it differs), then a plain box batch and a
    box AND class batch on the same context, then multi again."""
    for visit in (0, 1, 1, 0):
        boxes = [[segs.box(k, q, visit) for q in range(4)] for k in range(len(NS))]
        got, want = segs.multi(boxes)
        assert got == want, (visit, [g - w for g, w in zip(got, want)])
    a = segs.rows([[segs.box(k, q, 0) for q in range(4)] for k in range(len(NS))])[1]
    b = segs.rows([[segs.box(k, q, 1) for q in range(4)] for k in range(len(NS))])[1]
    assert a[VARIED[1]] != b[VARIED[1]] and a[:2] == b[:2]

    def plain(kind):
        want, preds = 0, []
        for k in range(len(NS)):
            lo, hi = segs.box(k, 3)
            sel = in_box(segs.xyz[k], lo, hi)
            if kind == "class":
                sel &= segs.cls[k] == 2
            preds.append(pkg.Predicate.bounds_class(lo, hi, 2) if kind == "class" else pkg.Predicate.bounds(lo, hi))
            want += int(sel.sum())
        segs.preset()
        if kind == "class":
            gpu_ctx.scan_dev_count_batch_combined(segs.cols_class, preds, segs.d_totals)
        else:
            gpu_ctx.scan_dev_count_batch(segs.cols, preds, segs.d_totals)
        assert want > 0 and segs.totals() == [PRESET[0] + want] + PRESET[1:], kind

    for kind in ("box", "multi", "class", "multi", "box", "class"):
        if kind == "multi":
            boxes = [[segs.box(k, q) for q in range(8)] for k in range(len(NS))]
            got, want = segs.multi(boxes)
            assert got == want, [g - w for g, w in zip(got, want)]
        else:
            plain(kind)


def test_refusals_leave_the_totals_alone(gpu_ctx, segs):
    segs.preset()

    def refused(cols, rows, **kw):
        with pytest.raises(binding.PcqError) as e:
            gpu_ctx.scan_dev_count_batch_multi(cols, rows, segs.d_totals, **kw)
        assert e.value.code == PCQ_ERR_ARG, e.value
        assert segs.totals() == PRESET

    def rows(nq):
        return [[pkg.Predicate.bounds(*segs.box(k, q % 8)) for q in range(nq)] for k in range(len(NS))]

    refused(segs.cols, rows(0))
    refused(segs.cols, rows(9))
    refused([], [], nqueries=0)
    refused([], [], nqueries=9)
    for nq in (1, 4):
        r = rows(nq)
        r[3][nq // 2] = pkg.Predicate.classification(2)
        refused(segs.cols, r)
        c = segs.cols[5]
        for bad in (binding.make_columns(xyz=c.xyz + 4, n=c.n - 1), binding.make_columns(xyz=c.xyz, n=100, xyz_stride=20),
                    binding.make_columns(xyz=None, n=100)):
            cols = list(segs.cols)
            cols[5] = bad
            refused(cols, rows(nq))
    # no segments: nothing to do, nothing written
    gpu_ctx.scan_dev_count_batch_multi([], [], segs.d_totals, nqueries=3)
    assert segs.totals() == PRESET
