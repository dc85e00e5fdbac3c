"""pcq_scan_dev_count_batch_bounds_time: box AND GPS time range over many resident segments in one launch, against numpy.

The design of test_gpu_batch_combined.py: the batch kernel's step is 512 points and its grid num_cus x 3 one-wave workgroups; a
workgroup changes segment only when the batch holds more steps than workgroups, and turns both register sets inside its loop
only from three steps per workgroup.  So: one batch of 1.4 M points (> 3 x 3 x CUs steps) in sixteen segments of unequal size —
n in {1, 255, 256, 511, 512, 513, 1027} (no step, exactly one, leftovers of every kind), several of tens of thousands of points,
one large — each with its own box AND its own range.  Segment k's times lie around 1000 k and rise along the segment, so a stale
cursor's range or time base, or leftover times taken from a block's start, change the count.  The time blocks are carved out of
one device buffer at 8-byte offsets of both residues modulo 16.
"""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
I32_MAX = 2**31 - 1

SIZES = [30_011, 1, 255, 1_100_003, 256, 511, 50_000, 512, 513, 70_003, 1027, 41_999, 20_001, 33_333, 12_345, 60_001]
EVERYTHING = ([-5000, -5000, -1000], [5000, 5000, 1000])
ALL_MATCH, EMPTY_BOX, ABSENT_RANGE, NAN_BOUND = 6, 9, 11, 13  # every point matches · box outside the i32 range · a range nobody is in · start = NaN


def inside(xyz, lmin, lmax):
    x = xyz.astype(np.int64)
    return np.all((x >= np.asarray(lmin, dtype=np.int64)) & (x <= np.asarray(lmax, dtype=np.int64)), axis=1)


def in_range(t, a, b):
    with np.errstate(invalid="ignore"):
        return (t >= a) & (t < b)


class Batch:
    """The segments on the host and in HBM, and numpy's answers."""

    def __init__(self, ctx):
        self.ctx = ctx
        rng = np.random.default_rng(2025)
        self.xyz, self.t, self.box, self.rng = [], [], [], []
        for k, n in enumerate(SIZES):
            xyz = np.stack([rng.integers(-5000, 5000, n), rng.integers(-5000, 5000, n), rng.integers(-1000, 1000, n)], axis=1).astype(np.int32)
            # around 1000 k, rising along the segment with noise, a NaN now and then
            t = 1000.0 * k + 100.0 * np.arange(n) / max(n, 1) + rng.uniform(-10.0, 10.0, n)
            t[rng.random(n) < 0.01] = np.nan
            lo = [-4000 + 300 * k, -3000 + 100 * k, -800 + 20 * k]
            hi = [1000 + 200 * k, 4500 - 150 * k, 900 - 30 * k]
            r = (1000.0 * k + 40.0 + 2.0 * (k % 5), 1000.0 * k + 200.0)  # the later part of the segment: its end, not its start
            if n < 600:
                r = (1000.0 * k - 20.0, 1000.0 * k + 60.0)
            if k == ALL_MATCH:
                t = np.where(np.isnan(t), 1000.0 * k, t)
                lo, hi, r = EVERYTHING[0], EVERYTHING[1], (-np.inf, np.inf)
            elif k == EMPTY_BOX:
                lo, hi = [I32_MAX + 1, -5000, -1000], [I32_MAX + 9, 5000, 1000]
            elif k == ABSENT_RANGE:
                r = (5e6, 6e6)
            elif k == NAN_BOUND:
                r = (np.nan, 1000.0 * k + 50.0)
            self.xyz.append(xyz), self.t.append(t), self.box.append((lo, hi)), self.rng.append(r)
        self.want = [int((inside(x, *bx) & in_range(t, *r)).sum()) for x, t, bx, r in zip(self.xyz, self.t, self.box, self.rng)]
        self.want_bounds = [int(inside(x, *bx).sum()) for x, bx in zip(self.xyz, self.box)]
        # positions: 16-byte aligned pieces of one buffer; time blocks: pieces of another at 8-byte offsets, 0 and 8 modulo 16
        pos_off, t_off, p, q = [], [], 0, 0
        for k, n in enumerate(SIZES):
            pos_off.append(p)
            p += (12 * n + 15) // 16 * 16
            q = (q + 15) // 16 * 16 + 8 * (k % 2)
            t_off.append(q)
            q += 8 * n
        self.d_pos, self.d_t = ctx.alloc(p + 64), ctx.alloc(q + 64)
        self.d_total = ctx.alloc(64)
        assert self.d_pos % 16 == 0 and self.d_t % 16 == 0
        assert [(self.d_t + o) % 16 for o in t_off] == [0, 8] * 8
        pos_img, t_img = np.zeros(p, dtype=np.uint8), np.zeros(q, dtype=np.uint8)
        for k, n in enumerate(SIZES):
            pos_img[pos_off[k]:pos_off[k] + 12 * n] = self.xyz[k].view(np.uint8).reshape(-1)
            t_img[t_off[k]:t_off[k] + 8 * n] = np.ascontiguousarray(self.t[k]).view(np.uint8).reshape(-1)
        ctx.to_device(self.d_pos, pos_img)
        ctx.to_device(self.d_t, t_img)
        self.cols = [binding.make_columns(xyz=self.d_pos + pos_off[k], cls=self.d_t + t_off[k], n=n, cls_stride=8) for k, n in enumerate(SIZES)]
        self.preds = [pkg.Predicate.bounds_time(bx[0], bx[1], r[0], r[1]) for bx, r in zip(self.box, self.rng)]

    def total(self):
        out = np.zeros(1, dtype=np.uint64)
        self.ctx.to_host(out, self.d_total)  # (waits for the context's stream)
        return int(out[0])

    def zero(self):
        self.ctx.memset(self.d_total, 0, 8)

    def free(self):
        for p in (self.d_pos, self.d_t, self.d_total):
            self.ctx.free(p)


@pytest.fixture(scope="module")
def batch(gpu_ctx):
    b = Batch(gpu_ctx)
    yield b
    b.free()


def test_the_batch_is_large_enough_to_turn_every_pipeline(gpu_ctx, batch):
    steps = sum(n // 512 for n in SIZES)
    assert steps >= 3 * 3 * gpu_ctx.device_info()["compute_units"], (steps, gpu_ctx.device_info())
    special = (EMPTY_BOX, ABSENT_RANGE, NAN_BOUND)
    assert batch.want[ALL_MATCH] == SIZES[ALL_MATCH] and all(batch.want[k] == 0 for k in special)
    assert all(batch.want_bounds[k] > 0 for k in (ABSENT_RANGE, NAN_BOUND))
    assert all(w > 0 for k, w in enumerate(batch.want) if k not in special and SIZES[k] > 1)
    for k, n in enumerate(SIZES):  # the answer differs from what the box alone, the range alone, or a neighbour's range gives
        if k in special or k == ALL_MATCH or n < 600:
            continue
        sel_t = in_range(batch.t[k], *batch.rng[k])
        assert batch.want[k] < min(batch.want_bounds[k], int(sel_t.sum())), k
        assert not in_range(batch.t[k], *batch.rng[k - 1]).any() or k - 1 == ALL_MATCH, k
        # leftover points (behind the last whole step) with their own times: other than with the block's first times
        rest = n - n // 512 * 512
        own = inside(batch.xyz[k][n - rest:], *batch.box[k]) & sel_t[n - rest:]
        first = inside(batch.xyz[k][n - rest:], *batch.box[k]) & sel_t[:rest]
        assert int(own.sum()) != int(first.sum()) or rest < 50, k


def test_whole_batch_and_accumulation(gpu_ctx, batch):
    batch.zero()
    gpu_ctx.scan_dev_count_batch_bounds_time(batch.cols, batch.preds, batch.d_total)
    assert batch.total() == sum(batch.want)
    gpu_ctx.scan_dev_count_batch_bounds_time(batch.cols, batch.preds, batch.d_total)  # the entry ADDS, to a non-zero total too
    assert batch.total() == 2 * sum(batch.want)
    gpu_ctx.scan_dev_count_batch_bounds_time([], [], batch.d_total)  # no segment: PCQ_OK, nothing added
    assert batch.total() == 2 * sum(batch.want)


def test_every_segment_alone_and_every_prefix(gpu_ctx, batch):
    """Each segment alone (a wrong time base, range or leftover shows in its own number), and growing batches (the segment
    a workgroup crosses into changes with the steps in front of it)."""
    for k in range(len(SIZES)):
        batch.zero()
        gpu_ctx.scan_dev_count_batch_bounds_time(batch.cols[k:k + 1], batch.preds[k:k + 1], batch.d_total)
        assert batch.total() == batch.want[k], (k, SIZES[k])
    for m in range(2, len(SIZES) + 1):
        batch.zero()
        gpu_ctx.scan_dev_count_batch_bounds_time(batch.cols[:m], batch.preds[:m], batch.d_total)
        assert batch.total() == sum(batch.want[:m]), m
    batch.zero()
    gpu_ctx.scan_dev_count_batch_bounds_time(batch.cols[::-1], batch.preds[::-1], batch.d_total)
    assert batch.total() == sum(batch.want)


def test_matches_the_per_file_scan(gpu_ctx, batch):
    """The answer the parent could give: one pcq_scan_dev with PCQ_PRED_BOUNDS_TIME per segment into one counter."""
    cc = gpu_ctx.count_collector()
    for cols, pred in zip(batch.cols, batch.preds):
        gpu_ctx.scan_dev(cols, pred, cc)
    assert cc.point_count() == sum(batch.want)
    cc.free()


def test_refusals_leave_the_counter_alone(gpu_ctx, batch):
    batch.zero()
    gpu_ctx.scan_dev_count_batch_bounds_time(batch.cols[:3], batch.preds[:3], batch.d_total)
    before = batch.total()
    assert before == sum(batch.want[:3])
    lo, hi = batch.box[0]

    def refused(cols, preds):
        with pytest.raises(binding.PcqError) as e:
            gpu_ctx.scan_dev_count_batch_bounds_time(cols, preds, batch.d_total)
        assert e.value.code == PCQ_ERR_ARG, e.value
        assert batch.total() == before

    for other in (pkg.Predicate.bounds(lo, hi), pkg.Predicate.classification(2), pkg.Predicate.time_range(0.0, 1.0),
                  pkg.Predicate.bounds_class(lo, hi, 2)):
        for at in (0, 2):
            preds = list(batch.preds[:3])
            preds[at] = other
            refused(batch.cols[:3], preds)
    c0 = batch.cols[0]
    for bad in (binding.make_columns(xyz=c0.xyz, cls=c0.cls, n=1000, xyz_stride=16, cls_stride=8),
                binding.make_columns(xyz=c0.xyz, cls=c0.cls, n=1000, cls_stride=16),
                binding.make_columns(xyz=c0.xyz, cls=c0.cls, n=1000),               # class bytes, not times
                binding.make_columns(xyz=c0.xyz, cls=None, n=1000, cls_stride=8),
                binding.make_columns(xyz=c0.xyz, cls=c0.cls + 4, n=1000, cls_stride=8),
                binding.make_columns(xyz=c0.xyz + 4, cls=c0.cls, n=1000, cls_stride=8)):
        refused([batch.cols[1], bad], batch.preds[:2])
        refused([bad], batch.preds[:1])
    # the table in HBM is still the one of the first call: the same batch again needs no upload and is right
    gpu_ctx.scan_dev_count_batch_bounds_time(batch.cols[:3], batch.preds[:3], batch.d_total)
    assert batch.total() == 2 * before


def test_segment_table_cache_tells_the_tables_apart(gpu_ctx, batch):
    """The table is uploaded only when it differs from the one in HBM.  Same files, same number of segments: two box AND time
    batches that differ in their ranges alone, then a plain bounds batch (another kind and pitch, the same count of segments
    and the same positions) and the box AND time batches around it, in two orders — every answer right.  This catches a cache
    keyed on the number of segments alone.  It cannot tell whether the kind is part of the key: tables of two kinds never have
    the same bytes, so the byte compare already separates them."""
    cols = batch.cols
    other_rng = [(1000.0 * k + 20.0, 1000.0 * k + 70.0) for k in range(len(SIZES))]
    other = [pkg.Predicate.bounds_time(bx[0], bx[1], r[0], r[1]) for bx, r in zip(batch.box, other_rng)]
    want_other = sum(int((inside(x, *bx) & in_range(t, *r)).sum()) for x, t, bx, r in zip(batch.xyz, batch.t, batch.box, other_rng))
    assert want_other != sum(batch.want)

    def run(kind):
        batch.zero()
        if kind == "bt":
            gpu_ctx.scan_dev_count_batch_bounds_time(cols, batch.preds, batch.d_total)
            return batch.total(), sum(batch.want)
        if kind == "bt2":
            gpu_ctx.scan_dev_count_batch_bounds_time(cols, other, batch.d_total)
            return batch.total(), want_other
        gpu_ctx.scan_dev_count_batch(cols, [pkg.Predicate.bounds(*bx) for bx in batch.box], batch.d_total)
        return batch.total(), sum(batch.want_bounds)

    for kind in ("bt", "bt2", "bt", "bt",                       # same kind and count, other bytes
                 "bounds", "bt", "bounds", "bt2",               # order one
                 "bt2", "bounds", "bounds", "bt", "bt", "bounds"):  # order two
        got, want = run(kind)
        assert got == want, kind
