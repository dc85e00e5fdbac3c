"""pcq_scan_dev_count_batch_combined: box AND class over many resident segments in one launch, against numpy.

The batch kernel's shape dictates the sizes: a step is 512 points, the grid is num_cus x 3 one-wave workgroups (768 on an
MI355X); a workgroup changes segment only when the batch holds more steps than workgroups, and turns both register sets
inside its loop only from three steps per workgroup.  So: one batch of 1.4 M points (> 3 x 768 steps) in sixteen segments of
unequal size — n in {1, 255, 256, 511, 512, 513, 1027} (no step, exactly one, leftovers of every kind), several of tens of
thousands of points, one large — each with its own box and class byte, the class blocks carved out of one device buffer at
byte offsets 0..15 (every dword misalignment, lane 63's second dword), the queried class falling unevenly along each segment.
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
ALL_MATCH, EMPTY_BOX, ABSENT_CLASS = 6, 9, 11  # segments: every point matches · box outside the i32 range · a class no point has


def inside(xyz, lmin, lmax):
    x = xyz.astype(np.int64)
    return np.all((x >= np.asarray(lmin, dtype=np.int64)) & (x <= np.asarray(lmax, dtype=np.int64)), axis=1)


class Batch:
    """The segments on the host and in HBM, and numpy's answers."""

    def __init__(self, ctx):
        self.ctx = ctx
        rng = np.random.default_rng(2024)
        self.xyz, self.cls, self.box, self.c = [], [], [], []
        for k, n in enumerate(SIZES):
            xyz = np.stack([rng.integers(-5000, 5000, n), rng.integers(-5000, 5000, n), rng.integers(-1000, 1000, n)], axis=1).astype(np.int32)
            a, b = (1, 2, 6, 9)[k % 4], (2, 6, 9, 1)[k % 4]
            # class a grows rarer along the segment, in bursts: a wrong segment's class byte or base changes the count
            ramp = np.arange(n) / max(n, 1)
            cls = np.where((rng.random(n) > ramp) & ((np.arange(n) // 97 + k) % 3 != 0), a, b).astype(np.uint8)
            lo = [-4000 + 300 * k, -3000 + 100 * k, -800 + 20 * k]
            hi = [1000 + 200 * k, 4500 - 150 * k, 900 - 30 * k]
            c = a
            if k == ALL_MATCH:
                cls[:] = 5
                lo, hi, c = EVERYTHING[0], EVERYTHING[1], 5
            elif k == EMPTY_BOX:
                lo, hi = [I32_MAX + 1, -5000, -1000], [I32_MAX + 9, 5000, 1000]
            elif k == ABSENT_CLASS:
                c = 77
            self.xyz.append(xyz), self.cls.append(cls), self.box.append((lo, hi)), self.c.append(c)
        self.want = [int((inside(x, *bx) & (cl == c)).sum()) for x, cl, bx, c in zip(self.xyz, self.cls, self.box, self.c)]
        self.want_bounds = [int(inside(x, *bx).sum()) for x, bx in zip(self.xyz, self.box)]
        self.want_class = [int((cl == c).sum()) for cl, c in zip(self.cls, self.c)]
        # positions: 16-byte aligned pieces of one buffer; class blocks: pieces of another at byte offsets 0..15
        pos_off, cls_off, p, q = [], [], 0, 0
        for k, n in enumerate(SIZES):
            pos_off.append(p)
            p += (12 * n + 15) // 16 * 16
            q = (q + 15) // 16 * 16 + k % 16
            cls_off.append(q)
            q += n
        self.d_pos, self.d_cls = ctx.alloc(p + 64), ctx.alloc(q + 64)
        self.d_total = ctx.alloc(64)
        assert self.d_pos % 16 == 0 and self.d_cls % 16 == 0
        assert sorted((self.d_cls + o) % 16 for o in cls_off) == list(range(16))
        pos_img, cls_img = np.zeros(p, dtype=np.uint8), np.full(q, 255, dtype=np.uint8)
        for k, n in enumerate(SIZES):
            pos_img[pos_off[k]:pos_off[k] + 12 * n] = self.xyz[k].view(np.uint8).reshape(-1)
            cls_img[cls_off[k]:cls_off[k] + n] = self.cls[k]
        ctx.to_device(self.d_pos, pos_img)
        ctx.to_device(self.d_cls, cls_img)
        self.cols = [binding.make_columns(xyz=self.d_pos + pos_off[k], cls=self.d_cls + cls_off[k], n=n) for k, n in enumerate(SIZES)]
        self.preds = [pkg.Predicate.bounds_class(bx[0], bx[1], c) for bx, c in zip(self.box, self.c)]

    def total(self):
        out = np.zeros(1, dtype=np.uint64)
        self.ctx.to_host(out, self.d_total)  # (waits for the context's stream)
        return int(out[0])

    def zero(self):
        self.ctx.memset(self.d_total, 0, 8)

    def free(self):
        for p in (self.d_pos, self.d_cls, self.d_total):
            self.ctx.free(p)


@pytest.fixture(scope="module")
def batch(gpu_ctx):
    b = Batch(gpu_ctx)
    yield b
    b.free()


def test_the_batch_is_large_enough_to_turn_every_pipeline(gpu_ctx, batch):
    steps = sum(n // 512 for n in SIZES)
    assert steps >= 3 * 3 * gpu_ctx.device_info()["compute_units"], (steps, gpu_ctx.device_info())
    assert batch.want[ALL_MATCH] == SIZES[ALL_MATCH] and batch.want[EMPTY_BOX] == 0 and batch.want[ABSENT_CLASS] == 0
    assert batch.want_bounds[ABSENT_CLASS] > 0 and all(w > 0 for k, w in enumerate(batch.want) if k not in (EMPTY_BOX, ABSENT_CLASS) and SIZES[k] > 1)


def test_whole_batch_and_accumulation(gpu_ctx, batch):
    batch.zero()
    gpu_ctx.scan_dev_count_batch_combined(batch.cols, batch.preds, batch.d_total)
    assert batch.total() == sum(batch.want)
    gpu_ctx.scan_dev_count_batch_combined(batch.cols, batch.preds, batch.d_total)  # the entry ADDS
    assert batch.total() == 2 * sum(batch.want)
    gpu_ctx.scan_dev_count_batch_combined([], [], batch.d_total)  # no segment: PCQ_OK, nothing added
    assert batch.total() == 2 * sum(batch.want)


def test_every_segment_alone_and_every_prefix(gpu_ctx, batch):
    """Each segment alone (a wrong class base, shift or leftover shows in its own number), and growing batches (the segment
    a workgroup crosses into changes with the steps in front of it)."""
    for k in range(len(SIZES)):
        batch.zero()
        gpu_ctx.scan_dev_count_batch_combined(batch.cols[k:k + 1], batch.preds[k:k + 1], batch.d_total)
        assert batch.total() == batch.want[k], (k, SIZES[k])
    for m in (2, 5, 9, 13):
        batch.zero()
        gpu_ctx.scan_dev_count_batch_combined(batch.cols[:m], batch.preds[:m], batch.d_total)
        assert batch.total() == sum(batch.want[:m]), m
    batch.zero()
    gpu_ctx.scan_dev_count_batch_combined(batch.cols[::-1], batch.preds[::-1], batch.d_total)
    assert batch.total() == sum(batch.want)


def test_matches_the_per_file_scan(gpu_ctx, batch):
    """The answer the parent could give: one pcq_scan_dev with PCQ_PRED_BOUNDS_CLASS per segment into one counter."""
    cc = gpu_ctx.count_collector()
    for cols, pred in zip(batch.cols, batch.preds):
        gpu_ctx.scan_dev(cols, pred, cc)
    assert cc.point_count() == sum(batch.want)
    cc.free()


def test_refusals_leave_the_counter_alone(gpu_ctx, batch):
    batch.zero()
    gpu_ctx.scan_dev_count_batch_combined(batch.cols[:3], batch.preds[:3], batch.d_total)
    before = batch.total()
    assert before == sum(batch.want[:3])
    lo, hi = batch.box[0]

    def refused(cols, preds):
        with pytest.raises(binding.PcqError) as e:
            gpu_ctx.scan_dev_count_batch_combined(cols, preds, batch.d_total)
        assert e.value.code == PCQ_ERR_ARG, e.value
        assert batch.total() == before

    for other in (pkg.Predicate.bounds(lo, hi), pkg.Predicate.classification(2), pkg.Predicate.time_range(0.0, 1.0)):
        for at in (0, 2):
            preds = list(batch.preds[:3])
            preds[at] = other
            refused(batch.cols[:3], preds)
    c0 = batch.cols[0]
    for bad in (binding.make_columns(xyz=c0.xyz, cls=c0.cls, n=1000, xyz_stride=16),
                binding.make_columns(xyz=c0.xyz, cls=c0.cls, n=1000, cls_stride=2),
                binding.make_columns(xyz=c0.xyz, cls=None, n=1000),
                binding.make_columns(xyz=c0.xyz + 4, cls=c0.cls, n=1000)):
        refused([batch.cols[1], bad], batch.preds[:2])
        refused([bad], batch.preds[:1])


def test_segment_table_cache_tells_the_tables_apart(gpu_ctx, batch):
    """The table is uploaded only when it differs from the one in HBM.  Same files, same number of segments: two combined
    batches that differ in their predicates alone, then a plain bounds batch, a combined batch and a class batch in two
    orders — every answer right."""
    cols = batch.cols
    other = [pkg.Predicate.bounds_class(bx[0], bx[1], 2) for bx in batch.box]
    want_other = sum(int((inside(x, *bx) & (cl == 2)).sum()) for x, cl, bx in zip(batch.xyz, batch.cls, batch.box))
    assert want_other != sum(batch.want)

    def run(kind):
        batch.zero()
        if kind == "combined":
            gpu_ctx.scan_dev_count_batch_combined(cols, batch.preds, batch.d_total)
            return batch.total(), sum(batch.want)
        if kind == "combined2":
            gpu_ctx.scan_dev_count_batch_combined(cols, other, batch.d_total)
            return batch.total(), want_other
        if kind == "bounds":
            gpu_ctx.scan_dev_count_batch(cols, [pkg.Predicate.bounds(*bx) for bx in batch.box], batch.d_total)
            return batch.total(), sum(batch.want_bounds)
        gpu_ctx.scan_dev_count_batch(cols, [pkg.Predicate.classification(c) for c in batch.c], batch.d_total)
        return batch.total(), sum(batch.want_class)

    for kind in ("combined", "combined2", "combined", "combined",                 # same kind and count, other bytes
                 "bounds", "combined", "class", "combined2",                      # order one
                 "class", "combined", "bounds", "bounds", "combined", "class"):   # order two
        got, want = run(kind)
        assert got == want, kind
