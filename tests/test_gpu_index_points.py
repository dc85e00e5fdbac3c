"""The chunk index serving the buffer collector (pcq_scan_dev_indexed with a buffer collector): the emit's count pass takes
each 2048-point tile's state from the index (disjoint: not read, contained: not read, straddling: counted), and the records
are exactly those of pcq_scan_dev — byte for byte, in file order, after whatever the collector already held — and those of
numpy on the same columns.  On spatially coherent data most chunks are skipped."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")

POINT_DTYPE = binding.POINT_DTYPE
I32MIN, I32MAX = -(2 ** 31), 2 ** 31 - 1
SCALE, OFFSET = (0.01, 0.02, 0.5), (10.0, -20.0, 3.0)


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


def expect_records(xyz, cls, rgb, sel):
    idx = np.flatnonzero(sel)
    out = np.zeros(len(idx), dtype=POINT_DTYPE)
    for a, k in enumerate("xyz"):
        out[k] = xyz[idx, a].astype(np.float64) * SCALE[a] + OFFSET[a]
    if rgb is not None:
        out["r"], out["g"], out["b"] = rgb[idx, 0], rgb[idx, 1], rgb[idx, 2]
    out["classification"] = cls[idx]
    return out


def in_box(xyz, lo, hi):
    v = xyz.astype(np.int64)
    return np.all((v >= np.array(lo, dtype=np.int64)) & (v <= np.array(hi, dtype=np.int64)), axis=1)


def scan_records(ctx, cols, pred, ix=None):
    gb = ctx.buffer_collector()
    try:
        if ix is None:
            ctx.scan_dev(cols, pred, gb)
        else:
            ctx.scan_dev_indexed(cols, pred, ix, gb)
        pts = gb.points()
        assert gb.point_count() == len(pts)
        return pts
    finally:
        gb.free()


def make_data(oracle, n, coherent, seed):
    spec = specs._spec(777 + seed, n, 1, (0.01,) * 3, (0.0,) * 3, (-50000, -50000, -1000), (100001, 100001, 2001),
                       classes=[(1, 0.5), (2, 0.3), (6, 0.2)])
    xyz, cls = oracle.synth_columns(spec)
    if coherent:  # scan-line like order: sorted by x, so a chunk covers a thin x slab
        order = np.argsort(xyz[:, 0], kind="stable")
        xyz, cls = xyz[order], cls[order]
    rgb = np.random.default_rng(seed).integers(0, 65536, (n, 3), dtype=np.uint16)
    return np.ascontiguousarray(xyz), np.ascontiguousarray(cls), rgb


def bounds_boxes(xyz, n, seed):
    boxes = [("everything", [I32MIN] * 3, [I32MAX] * 3),
             ("nothing", [10 ** 9] * 3, [2 * 10 ** 9] * 3),
             ("clamps_to_full", [-(2 ** 40)] * 3, [2 ** 40] * 3),
             ("max_point", [I32MAX] * 3, [I32MAX] * 3),
             ("min_point", [I32MIN] * 3, [I32MIN] * 3),
             ("empty_by_clamp", [2 ** 31, I32MIN, I32MIN], [2 ** 40, I32MAX, I32MAX])]
    if n >= 4096:
        c0 = xyz[:4096].astype(np.int64)
        mn, mx = c0.min(axis=0), c0.max(axis=0)
        boxes.append(("chunk0_box", list(mn), list(mx)))
        boxes.append(("chunk0_box_minus_face", list(mn), [int(mx[0]) - 1] + list(mx[1:])))
        boxes.append(("chunk0_box_plus_one", list(mn - 1), list(mx + 1)))
    if n >= 8192:
        c1 = xyz[4096:8192].astype(np.int64)
        boxes.append(("face_at_chunk1_min_x", [int(c1[:, 0].min()), I32MIN, I32MIN], [I32MAX] * 3))
        boxes.append(("face_at_chunk1_max_x", [I32MIN] * 3, [int(c1[:, 0].max()), I32MAX, I32MAX]))
    rng = np.random.default_rng(seed)
    for k in range(10):
        lo = rng.integers(-50000, 50000, 3)
        hi = lo + rng.integers(0, 60000, 3)
        boxes.append((f"random{k}", list(lo), list(hi)))
    return boxes


@pytest.mark.parametrize("n", [4095, 4096, 4097, 6144, 1_000_003])
@pytest.mark.parametrize("coherent", [False, True])
@pytest.mark.parametrize("colours", [False, True])
def test_indexed_bounds_records_equal_plain_and_numpy(oracle, gpu_ctx, n, coherent, colours):
    ctx = gpu_ctx
    xyz, cls, rgb = make_data(oracle, n, coherent, n)
    dev = Dev(ctx)
    ix = ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(cls, pad=3), rgb=dev.put(rgb, pad=2) if colours else None, n=n,
                                    scale=SCALE, offset=OFFSET)
        for k, (name, lo, hi) in enumerate(bounds_boxes(xyz, n, n)):
            pred = pkg.Predicate.bounds(lo, hi)
            want = expect_records(xyz, cls, rgb if colours else None, in_box(xyz, lo, hi)).tobytes()
            plain = scan_records(ctx, cols, pred).tobytes()
            got = scan_records(ctx, cols, pred, ix).tobytes()
            what = (name, n, coherent, colours)
            assert plain == want, what
            assert got == want, what
            st = ctx.index_stats(ix)
            if n >= 4096:
                assert st["chunks"] == n // 4096, (what, st)
                assert st["built"] == (1 if k == 0 else 0), (what, st)
                assert st["skipped"] + st["whole"] + st["scanned"] == st["chunks"], (what, st)
                if k == 0:  # the build read every chunk
                    assert st["scanned"] == st["chunks"], (what, st)
                elif name in ("nothing", "empty_by_clamp"):
                    assert st["skipped"] == st["chunks"], (what, st)
                elif name in ("everything", "clamps_to_full"):
                    assert st["whole"] == st["chunks"], (what, st)
                elif name == "chunk0_box":
                    assert st["whole"] >= 1, (what, st)
    finally:
        ctx.index_free(ix)
        dev.free()


def test_repeated_query_reuses_the_index_and_appends_after_existing_records(oracle, gpu_ctx):
    ctx = gpu_ctx
    n = 300_007
    xyz, cls, rgb = make_data(oracle, n, True, 5)
    dev = Dev(ctx)
    ix = ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(cls), rgb=dev.put(rgb), n=n, scale=SCALE, offset=OFFSET)
        lo, hi = [-20000, -40000, -1000], [-5000, 40000, 1000]
        pred = pkg.Predicate.bounds(lo, hi)
        one = expect_records(xyz, cls, rgb, in_box(xyz, lo, hi))
        for k in range(3):
            assert scan_records(ctx, cols, pred, ix).tobytes() == one.tobytes()
            assert ctx.index_stats(ix)["built"] == (1 if k == 0 else 0)
        # two scans into one collector: a plain one, then an indexed one (and the other way round) — the second's records follow
        other = pkg.Predicate.bounds([I32MIN] * 3, [-30000, I32MAX, I32MAX])
        two = expect_records(xyz, cls, rgb, in_box(xyz, [I32MIN] * 3, [-30000, I32MAX, I32MAX]))
        for first_indexed in (False, True):
            gb = ctx.buffer_collector()
            if first_indexed:
                ctx.scan_dev_indexed(cols, pred, ix, gb)
            else:
                ctx.scan_dev(cols, pred, gb)
            ctx.scan_dev_indexed(cols, other, ix, gb)
            ctx.scan_dev_indexed(cols, pred, ix, gb)
            assert gb.points().tobytes() == one.tobytes() + two.tobytes() + one.tobytes(), first_indexed
            gb.free()
    finally:
        ctx.index_free(ix)
        dev.free()


@pytest.mark.parametrize("park,sparse", [(256, 64), (0, 0), (0, 2048), (256, 0)])
def test_indexed_records_with_and_without_the_parked_and_sparse_writers(oracle, gpu_ctx, park, sparse):
    ctx = gpu_ctx
    n = 1_000_003
    before = (ctx.get_option("emit_park_max"), ctx.get_option("emit_sparse_max"))
    dev = Dev(ctx)
    ix = ctx.index_new()
    try:
        ctx.set_option("emit_park_max", park)
        ctx.set_option("emit_sparse_max", sparse)
        for coherent in (False, True):
            xyz, cls, rgb = make_data(oracle, n, coherent, 11)
            cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(cls), rgb=dev.put(rgb), n=n, scale=SCALE, offset=OFFSET)
            boxes = [([I32MIN] * 3, [I32MAX] * 3), ([-49000, -50000, -1000], [-48000, 50000, 1000]),
                     ([-30000, -30000, -900], [30000, 30000, 900]), ([0, 0, 0], [2000, 2000, 100]), ([-40000, 0, -1000], [-20000, 100, 1000])]
            for lo, hi in boxes:
                pred = pkg.Predicate.bounds(lo, hi)
                want = expect_records(xyz, cls, rgb, in_box(xyz, lo, hi)).tobytes()
                assert scan_records(ctx, cols, pred).tobytes() == want, (park, sparse, coherent, lo, hi)
                assert scan_records(ctx, cols, pred, ix).tobytes() == want, (park, sparse, coherent, lo, hi)
    finally:
        ctx.set_option("emit_park_max", before[0])
        ctx.set_option("emit_sparse_max", before[1])
        ctx.index_free(ix)
        dev.free()


@pytest.mark.parametrize("n", [1, 65_535, 65_536, 65_537, 500_009])
def test_indexed_class_records(oracle, gpu_ctx, n):
    ctx = gpu_ctx
    xyz, cls, rgb = make_data(oracle, n, False, 3 * n)
    if n >= 65_536:
        cls[:65_536] = 200   # a class that fills a whole chunk (and is absent from the others)
    if n >= 200_000:
        cls[131_072:196_608] = 6
    dev = Dev(ctx)
    ix = ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz, pad=4), cls=dev.put(cls, pad=3), rgb=dev.put(rgb), n=n, scale=SCALE, offset=OFFSET)
        for k, c in enumerate([6, 1, 2, 200, 19, 0, 255, 6]):
            pred = pkg.Predicate.classification(c)
            want = expect_records(xyz, cls, rgb, cls == c).tobytes()
            assert scan_records(ctx, cols, pred).tobytes() == want, (n, c)
            assert scan_records(ctx, cols, pred, ix).tobytes() == want, (n, c)
            st = ctx.index_stats(ix)
            assert st["chunks"] == (n + 65_535) // 65_536 and st["built"] == (1 if k == 0 else 0), (n, c, st)
            if k > 0:
                assert st["skipped"] + st["whole"] + st["scanned"] == st["chunks"], (n, c, st)
                if c in (19, 255):  # absent: every chunk is skipped
                    assert st["skipped"] == st["chunks"], (n, c, st)
                if c == 200 and n >= 65_536:
                    assert st["whole"] >= 1, (n, c, st)
                    assert st["skipped"] == st["chunks"] - 1, (n, c, st)
    finally:
        ctx.index_free(ix)
        dev.free()


def test_thin_slab_on_coherent_data_skips_most_chunks(oracle, gpu_ctx):
    ctx = gpu_ctx
    n = 1_000_003
    xyz, cls, rgb = make_data(oracle, n, True, 21)
    dev = Dev(ctx)
    ix = ctx.index_new()
    try:
        cols = binding.make_columns(xyz=dev.put(xyz), cls=dev.put(cls), n=n, scale=SCALE, offset=OFFSET)
        lo, hi = [1000, I32MIN, I32MIN], [2000, I32MAX, I32MAX]
        pred = pkg.Predicate.bounds(lo, hi)
        want = expect_records(xyz, cls, None, in_box(xyz, lo, hi)).tobytes()
        for k in range(2):
            assert scan_records(ctx, cols, pred, ix).tobytes() == want
        st = ctx.index_stats(ix)
        assert st["built"] == 0 and st["chunks"] == n // 4096
        assert st["skipped"] + st["whole"] + st["scanned"] == st["chunks"]
        assert st["skipped"] >= 0.9 * st["chunks"], st
        assert st["scanned"] <= 2 and st["whole"] >= 1, st
    finally:
        ctx.index_free(ix)
        dev.free()


def test_layouts_the_index_does_not_cover_fall_through_to_the_plain_scan(oracle, gpu_ctx):
    ctx = gpu_ctx
    n = 20_011
    xyz, cls, rgb = make_data(oracle, n, True, 8)
    lo, hi = [-30000, -40000, -1000], [10000, 40000, 1000]
    pred = pkg.Predicate.bounds(lo, hi)
    sel = in_box(xyz, lo, hi)
    dev = Dev(ctx)
    ix = ctx.index_new()
    try:
        pc, pr = dev.put(cls), dev.put(rgb)
        # unaligned positions
        cols = binding.make_columns(xyz=dev.put(xyz, pad=4), cls=pc, rgb=pr, n=n, scale=SCALE, offset=OFFSET)
        assert scan_records(ctx, cols, pred, ix).tobytes() == expect_records(xyz, cls, rgb, sel).tobytes()
        # fewer than 4096 points
        small = binding.make_columns(xyz=dev.put(xyz[:100]), cls=pc, rgb=pr, n=100, scale=SCALE, offset=OFFSET)
        assert scan_records(ctx, small, pred, ix).tobytes() == expect_records(xyz[:100], cls, rgb, sel[:100]).tobytes()
        # strided (LAS-like records of 34 bytes)
        rec = np.zeros((n, 34), dtype=np.uint8)
        rec[:, 0:12] = xyz.view(np.uint8).reshape(n, 12)
        rec[:, 15] = cls
        rec[:, 28:34] = rgb.view(np.uint8).reshape(n, 6)
        p = dev.put(rec)
        scols = binding.make_columns(xyz=p, cls=p + 15, rgb=p + 28, n=n, xyz_stride=34, cls_stride=34, rgb_stride=34, scale=SCALE, offset=OFFSET)
        want = expect_records(xyz, cls, rgb, sel).tobytes()
        assert scan_records(ctx, scols, pred, ix).tobytes() == want
        cpred = pkg.Predicate.classification(2)
        assert scan_records(ctx, scols, cpred, ix).tobytes() == expect_records(xyz, cls, rgb, cls == 2).tobytes()
        # the aligned block builds the index after all of that
        cols = binding.make_columns(xyz=dev.put(xyz), cls=pc, rgb=pr, n=n, scale=SCALE, offset=OFFSET)
        for k in range(2):
            assert scan_records(ctx, cols, pred, ix).tobytes() == want
            assert ctx.index_stats(ix)["built"] == (1 if k == 0 else 0)
        # grid collectors are not served by the index
        gg = ctx.grid_collector([-1000.0] * 3, [1000.0] * 3, 10.0)
        with pytest.raises(pkg.PcqError) as e:
            ctx.scan_dev_indexed(cols, pred, ix, gg)
        assert e.value.code == -8
        gg.free()
    finally:
        ctx.index_free(ix)
        dev.free()
