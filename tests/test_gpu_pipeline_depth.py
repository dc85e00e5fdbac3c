"""The count kernels' software pipelines beyond their second step, on step-coded data, against numpy.

Sizes come from the device's compute units through tests/_pipeline_plan.py (whose CPU test shows what they reach): per file
5g + g // 3 steps (depths 6 and 5: the loop-back taken twice, both exits out of the steady state) and 4g - 1 steps (depths 4
and 3: each register set reloaded once while the other is in flight), each with a head, leftover vectors or a leftover tile,
and a tail; the batches one plan of seventeen segments, at least 5g + g // 3 steps, in which workgroups change segment when
either cursor seeks and jump over segments with a few steps, none, and no element.  In step s the data hold m(s) matches of
query value s mod 3, m distinct along every workgroup's list, on a background no query matches (_pipeline_plan.py): a step
counted twice, dropped or read from the wrong place moves a total by an amount no other single error cancels.  On an MI355X
(256 CUs) the largest input is 25 MB of positions; the class batch is 26 MB.
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
I32_MAX = 2**31 - 1

SIZES = {"deep": pp.deep_steps, "shallow": pp.shallow_steps}
DEPTHS = {"deep": {5, 6}, "shallow": {3, 4}}
CLASSES, FILLER, ABSENT = (2, 6, 9), 1, 77
RANGES = ((100.0, 200.0), (300.0, 400.0), (500.0, 600.0))


class Dev:
    """Device copies of host arrays at a byte phase of a 16-byte line, freed together."""

    def __init__(self, ctx):
        self.ctx, self.blocks = ctx, []

    def put(self, arr, phase=0):
        arr = np.ascontiguousarray(arr)
        base = self.ctx.alloc(arr.nbytes + 64 + phase)
        self.blocks.append(base)
        assert base % 16 == 0
        if arr.nbytes:
            self.ctx.to_device(base + phase, arr)
        return base + phase

    def free(self):
        for b in self.blocks:
            self.ctx.free(b)
        self.blocks = []


@pytest.fixture(scope="module")
def cus(gpu_ctx):
    return gpu_ctx.device_info()["compute_units"]


def count(ctx, cols, pred):
    cc = ctx.count_collector()
    try:
        ctx.scan_dev(cols, pred, cc)
        return cc.point_count()
    finally:
        cc.free()


def reaches(fam, cus, steps, size):
    """The depth claim, with the real compute-unit count."""
    rep = pp.depth_report(pp.schedule(pp.per_file_grid(fam, cus, steps), steps))
    assert set(rep["depths"]) == DEPTHS[size] and rep["both_exits_deep"] == (size == "deep"), rep
    return pp.full_grid(fam, cus)


# ---------------------------------------------------------------------------------------------------------------------
# per-file kernels through pcq_scan_dev with count collectors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["deep", "shallow"])
@pytest.mark.parametrize("phase", [0, 1, 9, 15])
def test_class_count_k2(gpu_ctx, cus, phase, size):
    """k_class_count_pipe<4>: the three planted classes, the filler (everything else) and an absent class."""
    g = pp.full_grid(pp.K2, cus)
    steps = SIZES[size](g)
    reaches(pp.K2, cus, steps, size)
    head = (16 - phase) % 16
    a = pp.class_file(np.random.default_rng(100 + phase), g, steps, head, 16 * 21 + 11, CLASSES, (FILLER,))
    dev = Dev(gpu_ctx)
    try:
        d = dev.put(a, phase)
        assert pp.class_layout(d, len(a)) == (head, 256 * steps + 21, steps)
        cols = binding.make_columns(cls=d, n=len(a))
        for c in CLASSES + (FILLER, ABSENT):
            got, want = count(gpu_ctx, cols, pkg.Predicate.classification(c)), pp.class_count(a, c)
            assert got == want, f"K2 phase {phase} S={steps} g={g} class {c}: got - want = {got - want}"
    finally:
        dev.free()


def time_queries(t):
    qs = list(RANGES) + [(-np.inf, np.inf), (300.0, 300.0), (400.0, 300.0), (100.0, 600.0)]
    return [(a, b, pp.time_count(t, a, b)) for a, b in qs]


@pytest.mark.parametrize("size", ["deep", "shallow"])
@pytest.mark.parametrize("phase", [0, 8])
def test_time_count_k3(gpu_ctx, cus, phase, size):
    """k_time_count_pipe<4>: planted times on each range's start, just below its end and in its middle; its end, NaN and
    the infinities in the background; every time but NaN and +inf, and two empty ranges."""
    g = pp.full_grid(pp.K3, cus)
    steps = SIZES[size](g)
    reaches(pp.K3, cus, steps, size)
    head = phase // 8
    t = pp.time_file(np.random.default_rng(200 + phase), g, steps, head, 2 * 37 + 1, RANGES)
    dev = Dev(gpu_ctx)
    try:
        d = dev.put(t, phase)
        assert pp.time_layout(d, len(t)) == (head, 256 * steps + 37, steps)
        cols = binding.make_columns(cls=d, n=len(t), cls_stride=8)
        for a, b, want in time_queries(t):
            got = count(gpu_ctx, cols, pkg.Predicate.time_range(a, b))
            assert got == want, f"K3 phase {phase} S={steps} g={g} [{a}, {b}): got - want = {got - want}"
    finally:
        dev.free()


def test_time_count_strided_kernel_agrees(gpu_ctx, cus):
    """The same step-coded column only 4-byte aligned: k_generic_count<PCQ_PRED_TIME>, the cross-check kernel."""
    g = pp.full_grid(pp.K3, cus)
    steps = pp.shallow_steps(g)
    t = pp.time_file(np.random.default_rng(204), g, steps, 1, 2 * 37 + 1, RANGES)
    dev = Dev(gpu_ctx)
    try:
        cols = binding.make_columns(cls=dev.put(t, 4), n=len(t), cls_stride=8)
        for a, b, want in time_queries(t):
            got = count(gpu_ctx, cols, pkg.Predicate.time_range(a, b))
            assert got == want, f"strided time count phase 4 S={steps} g={g} [{a}, {b}): got - want = {got - want}"
    finally:
        dev.free()


@pytest.mark.parametrize("size", ["deep", "shallow"])
@pytest.mark.parametrize("peel", [0, 1])
def test_bounds_count_k1_plain_class_and_time(gpu_ctx, cus, peel, size):
    """k_bounds_count_w1_pipe<2> plain, + ClassBytes (class phases 0 and 3), + GpsTimes (time phases 0 and 8), behind a
    head peel of 0 and 1 point: one leftover tile and 13 tail points.  The combined queries' matches are the planted points;
    half the background passes the box alone, half the column alone."""
    g = pp.full_grid(pp.K1, cus)
    steps = SIZES[size](g)
    reaches(pp.K1, cus, steps, size)
    q = pp.PointQueries(classes=CLASSES, other_classes=(FILLER, 7), ranges=RANGES)
    xyz, cls, t = pp.points_file(np.random.default_rng(300 + peel), g, steps, peel, 256 + 13, q)
    n, x64 = len(xyz), xyz.astype(np.int64)
    where = f"peel {peel} S={steps} g={g}"
    dev = Dev(gpu_ctx)
    try:
        d_xyz = dev.put(xyz, 4 * peel)
        assert pp.k1_layout(d_xyz, n) == (peel, 2 * steps + 1, steps)
        cols = binding.make_columns(xyz=d_xyz, n=n)
        for lo, hi in q.sub + [q.box, q.inside, ([5, 5, 5], [4, 4, 4])]:
            got, want = count(gpu_ctx, cols, pkg.Predicate.bounds(lo, hi)), pp.box_count(x64, lo, hi)
            assert got == want, f"K1 {where} box {lo}..{hi}: got - want = {got - want}"
        for cph in (0, 3):
            cols = binding.make_columns(xyz=d_xyz, cls=dev.put(cls, cph), n=n)
            for lo, hi, c in [q.box + (c,) for c in CLASSES + (FILLER, ABSENT)] + [q.sub[1] + (CLASSES[1],), q.sub[1] + (CLASSES[0],)]:
                got = count(gpu_ctx, cols, pkg.Predicate.bounds_class(lo, hi, c))
                want = int((pp.in_box(x64, lo, hi) & (cls == c)).sum())
                assert got == want, f"K1+class {where} class phase {cph} box {lo}..{hi} class {c}: got - want = {got - want}"
        for tph in (0, 8):
            cols = binding.make_columns(xyz=d_xyz, cls=dev.put(t, tph), n=n, cls_stride=8)
            for lo, hi, a, b in [q.box + r for r in RANGES + ((-np.inf, np.inf), (300.0, 300.0))] + [q.sub[2] + RANGES[2], q.sub[2] + RANGES[0]]:
                got = count(gpu_ctx, cols, pkg.Predicate.bounds_time(lo, hi, a, b))
                want = int((pp.in_box(x64, lo, hi) & pp.in_range(t, a, b)).sum())
                assert got == want, f"K1+time {where} time phase {tph} box {lo}..{hi} [{a}, {b}): got - want = {got - want}"
    finally:
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# batched kernels through pcq_scan_dev_count_batch and pcq_scan_dev_count_batch_combined
# ---------------------------------------------------------------------------------------------------------------------
class Batch:
    """Segments in HBM with their predicates, numpy's answer for each, and the device total."""

    def __init__(self, ctx, name, g, run):
        self.ctx, self.name, self.g, self.run = ctx, name, g, run
        self.cols, self.preds, self.want, self.blocks = [], [], [], []
        self.d_total = self.alloc(64)

    def alloc(self, nbytes):
        p = self.ctx.alloc(nbytes + 64)
        assert p % 16 == 0
        self.blocks.append(p)
        return p

    def total(self):
        out = np.zeros(1, dtype=np.uint64)
        self.ctx.to_host(out, self.d_total)  # (waits for the context's stream)
        return int(out[0])

    def of(self, cols, preds):
        self.ctx.memset(self.d_total, 0, 8)
        self.run(cols, preds, self.d_total)
        return self.total()

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


def check_batch(b):
    """The whole batch and a second call that adds to it; every segment alone; prefixes; the reversed order."""
    n, want = len(b.cols), sum(b.want)
    got = b.of(b.cols, b.preds)
    assert got == want, f"{b.name} batch g={b.g}: got - want = {got - want}"
    b.run(b.cols, b.preds, b.d_total)
    assert b.total() == 2 * want, f"{b.name} batch g={b.g}, second call: got - want = {b.total() - 2 * want}"
    for k in range(n):
        got = b.of(b.cols[k:k + 1], b.preds[k:k + 1])
        assert got == b.want[k], f"{b.name} segment {k} alone g={b.g}: got - want = {got - b.want[k]}"
    for m in (2, 3, 5, 6, 9, 10, 12, 14, 16):
        got = b.of(b.cols[:m], b.preds[:m])
        assert got == sum(b.want[:m]), f"{b.name} first {m} segments g={b.g}: got - want = {got - sum(b.want[:m])}"
    got = b.of(b.cols[::-1], b.preds[::-1])
    assert got == want, f"{b.name} batch reversed g={b.g}: got - want = {got - want}"


def batch_reaches(fam, cus, plan, ns, steps):
    """Every crossing kind, with the real compute-unit count."""
    g = pp.full_grid(fam, cus)
    assert steps == [s.steps for s in plan]
    rep = pp.depth_report(pp.schedule(pp.batch_grid(fam, cus, sum(steps), len(plan)), sum(steps), steps, ns))
    assert sum(steps) >= pp.deep_steps(g) and min(rep["depths"]) >= 5 and rep["both_exits_deep"], rep["depths"]
    assert rep["cross_into_a"] and rep["cross_into_b"] and rep["skips_stepped"] and rep["skips_zero_step"] and rep["skips_empty"], rep
    s = np.arange(sum(steps))
    pp.check_counts(s, pp.planted(s, g), g, 1, fam.step)


@pytest.fixture(scope="module")
def class_batch(gpu_ctx, cus):
    """Segment k asks for class 10 + k; its background is classes 9 + k and 11 + k, what its neighbours ask for."""
    g = pp.full_grid(pp.K2, cus)
    plan = pp.batch_plan(g)
    ns = [pp.class_segment_bytes(s) for s in plan]
    off, size = pp.carve(ns, [s.phase for s in plan])
    b = Batch(gpu_ctx, "class", g, gpu_ctx.scan_dev_count_batch)
    base = b.alloc(size)
    layouts = [pp.class_layout(base + o, n) for o, n in zip(off, ns)]
    batch_reaches(pp.K2, cus, plan, ns, [lay[2] for lay in layouts])
    assert sorted({lay[0] for lay in layouts}) == list(range(16))
    begin = pp.tile_begin([s.steps for s in plan])
    rng = np.random.default_rng(400)
    img = np.full(size, 255, dtype=np.uint8)
    b.host = []
    for k, (seg, lay) in enumerate(zip(plan, layouts)):
        a = pp.class_file(rng, g, seg.steps, lay[0], ns[k] - lay[0] - pp.K2.step * seg.steps, (10 + k,), (9 + k, 11 + k), int(begin[k]))
        img[off[k]:off[k] + ns[k]] = a
        b.host.append(a)
        b.cols.append(binding.make_columns(cls=base + off[k], n=ns[k]))
        b.preds.append(pkg.Predicate.classification(10 + k))
        b.want.append(pp.class_count(a, 10 + k))
    gpu_ctx.to_device(base, img)
    yield b
    b.free()


def test_class_batch(class_batch):
    check_batch(class_batch)


def test_class_batch_one_block_listed_twice_with_two_classes(class_batch):
    b = class_batch
    for k in (4, 9):  # large segments: the second listing asks for a class of the first one's background
        got = b.of([b.cols[k], b.cols[k]], [b.preds[k], pkg.Predicate.classification(9 + k)])
        want = b.want[k] + pp.class_count(b.host[k], 9 + k)
        assert got == want, f"class segment {k} listed twice g={b.g}: got - want = {got - want}"
        got = b.of([b.cols[k], b.cols[k + 1], b.cols[k]], [pkg.Predicate.classification(11 + k), b.preds[k + 1], b.preds[k]])
        want = pp.class_count(b.host[k], 11 + k) + b.want[k + 1] + b.want[k]
        assert got == want, f"class segment {k} around segment {k + 1} g={b.g}: got - want = {got - want}"


class PointSegments:
    """The plan's sizes as positions (16-byte aligned) and class blocks (byte phases 0..15) in two device buffers.  Segment
    k: its boxes shifted by 10 000 k along x, class 20 + k planted; the background inside its box carries its neighbours'
    classes, the background outside it its own class, part of it inside its neighbours' boxes."""

    def __init__(self, ctx, cus):
        g = self.g = pp.full_grid(pp.K1, cus)
        plan = pp.batch_plan(g)
        ns = [pp.point_segment_points(s) for s in plan]
        batch_reaches(pp.K1, cus, plan, ns, [n // pp.K1.step for n in ns])
        poff, psize = pp.carve(ns, [0] * len(ns), 12)
        coff, csize = pp.carve(ns, [s.phase for s in plan])
        self.keep = Batch(ctx, "", g, None)
        d_pos, d_cls = self.keep.alloc(psize), self.keep.alloc(csize)
        begin = pp.tile_begin([s.steps for s in plan])
        rng = np.random.default_rng(500)
        pos_img, cls_img = np.zeros(psize, dtype=np.uint8), np.full(csize, 255, dtype=np.uint8)
        self.cols, self.q, self.xyz, self.cls = [], [], [], []
        for k, seg in enumerate(plan):
            near = [pp.PointQueries(10_000 * j, classes=(0,), other_classes=(1,)).sub[0] for j in (k - 1, k + 1)]
            q = pp.PointQueries(10_000 * k, classes=(20 + k,), other_classes=(19 + k, 21 + k), ranges=RANGES[:1], more_outside=near)
            xyz, cls, _ = pp.points_file(rng, g, seg.steps, 0, ns[k] - pp.K1.step * seg.steps, q, int(begin[k]))
            pos_img[poff[k]:poff[k] + 12 * ns[k]] = xyz.view(np.uint8).reshape(-1)
            cls_img[coff[k]:coff[k] + ns[k]] = cls
            self.cols.append(binding.make_columns(xyz=d_pos + poff[k], cls=d_cls + coff[k], n=ns[k]))
            self.q.append(q), self.xyz.append(xyz), self.cls.append(cls)
        ctx.to_device(d_pos, pos_img)
        ctx.to_device(d_cls, cls_img)

    def batch(self, ctx, name, run, boxes, classes=None):
        b = Batch(ctx, name, self.g, run)
        b.cols = self.cols
        for k, (lo, hi) in enumerate(boxes):
            sel = pp.in_box(self.xyz[k], lo, hi)
            if classes is None:
                b.preds.append(pkg.Predicate.bounds(lo, hi))
            else:
                b.preds.append(pkg.Predicate.bounds_class(lo, hi, classes[k]))
                sel &= self.cls[k] == classes[k]
            b.want.append(int(sel.sum()))
        assert b.want[pp.EMPTY_BOX_SEGMENT] == 0 and all(w > 0 for k, w in enumerate(b.want) if k != pp.EMPTY_BOX_SEGMENT and self.cols[k].n)
        return b


@pytest.fixture(scope="module")
def point_segments(gpu_ctx, cus):
    p = PointSegments(gpu_ctx, cus)
    yield p
    p.keep.free()


def test_bounds_batch(gpu_ctx, point_segments):
    """k_bounds_count_batch_pipe<2>: every segment's own small box, in which only its planted points lie (its neighbours'
    small boxes hold part of its background); one box outside the i32 range between two large segments."""
    boxes = [q.sub[0] for q in point_segments.q]
    boxes[pp.EMPTY_BOX_SEGMENT] = ([I32_MAX + 1, -1000, -1000], [I32_MAX + 9, 1000, 1000])
    b = point_segments.batch(gpu_ctx, "bounds", gpu_ctx.scan_dev_count_batch, boxes)
    try:
        check_batch(b)
    finally:
        b.free()


def test_combined_batch(gpu_ctx, point_segments):
    """k_bounds_count_batch_pipe<2, ClassBytes>: every segment's large box and class; one box with lmin > lmax."""
    boxes = [q.box for q in point_segments.q]
    boxes[pp.EMPTY_BOX_SEGMENT] = ([5, 5, 5], [4, 4, 4])
    b = point_segments.batch(gpu_ctx, "combined", gpu_ctx.scan_dev_count_batch_combined, boxes, [q.classes[0] for q in point_segments.q])
    try:
        check_batch(b)
    finally:
        b.free()
