"""The combined searches (PCQ_PRED_BOUNDS_CLASS, PCQ_PRED_BOUNDS_TIME) on the GPU: counts, records and grids against numpy,
the oracle's SparseGrid and the oracle's bounds search filtered by class.

Expected results: inside = lmin <= (x, y, z) <= lmax per axis in i64, and (cls == C) or (start <= t < end) on float64
(NaN -> False).  A match's record is the attribute search's: position, class byte and colour for BOUNDS_CLASS; position,
class 0 and colour (0, 0, 0) for BOUNDS_TIME.  Covered: the fast count (K1 with a second column) at every byte phase of
the positions and of the class / time column, strided LAS records (class at +15 / +16), empty boxes, boxes outside the
i32 range, i32 extremes and box faces, absent classes and full matches, NaN and empty ranges, host and file scans across
staging-chunk seams, two files into one buffer and grid, the chunk index's fall-through and the batch refusal, the CLI,
the C view, and one full-size resident count.
"""
import ctypes as C
import importlib
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _time_images as ti  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")
POINT_DTYPE = binding.POINT_DTYPE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY = os.path.join(ROOT, "adhoc-queries-pointclouds_amd", "host", "query")
GRID_BOX = ((-60.0, -400.0, -50.0), (160.0, 0.0, 60.0))
CELL = 2.5
I32_MIN, I32_MAX = -2**31, 2**31 - 1


class Dev:
    """Device copies of host arrays, freed together."""

    def __init__(self, ctx):
        self.ctx, self.blocks = ctx, []

    def put(self, arr, pad=0):
        arr = np.ascontiguousarray(arr)
        base = self.ctx.alloc(arr.nbytes + 64 + pad)
        self.blocks.append(base)
        if arr.nbytes:
            self.ctx.to_device(base + pad, arr)
        return base + pad

    def free(self):
        for b in self.blocks:
            self.ctx.free(b)
        self.blocks = []


def inside(xyz, lmin, lmax):
    x = xyz.astype(np.int64)
    return np.all((x >= np.asarray(lmin, dtype=np.int64)) & (x <= np.asarray(lmax, dtype=np.int64)), axis=1)


class Query:
    """One combined predicate and its numpy restatement."""

    def __init__(self, lmin, lmax, cls=None, start=None, end=None):
        self.lmin, self.lmax, self.cls, self.start, self.end = list(lmin), list(lmax), cls, start, end

    def pred(self):
        if self.cls is not None:
            return pkg.Predicate.bounds_class(self.lmin, self.lmax, self.cls)
        return pkg.Predicate.bounds_time(self.lmin, self.lmax, self.start, self.end)

    def select(self, xyz, cls, t):
        attr = (cls == self.cls) if self.cls is not None else ti.select(t, self.start, self.end)
        return inside(xyz, self.lmin, self.lmax) & attr

    def records(self, xyz, cls, rgb, sel):
        """The attribute search's records, in file order (rgb None: a file without colour)."""
        idx = np.flatnonzero(sel)
        out = np.zeros(len(idx), dtype=POINT_DTYPE)
        w = ti.world(xyz[idx])
        out["x"], out["y"], out["z"] = w[:, 0], w[:, 1], w[:, 2]
        if self.cls is not None:
            out["classification"] = cls[idx]
            if rgb is not None:
                out["r"], out["g"], out["b"] = rgb[idx, 0], rgb[idx, 1], rgb[idx, 2]
        return out

    def __repr__(self):
        return f"Query({self.lmin}, {self.lmax}, cls={self.cls}, t=[{self.start}, {self.end}))"


def oracle_grid(oracle, q, xyz, cls, rgb, sel, og=None):
    og = og or oracle.grid_collector(GRID_BOX[0], GRID_BOX[1], CELL)
    w = ti.world(xyz)
    for i in np.flatnonzero(sel):
        if q.cls is not None and rgb is not None:
            og.collect_one(float(w[i, 0]), float(w[i, 1]), float(w[i, 2]), int(rgb[i, 0]), int(rgb[i, 1]), int(rgb[i, 2]), int(cls[i]))
        elif q.cls is not None:
            og.collect_one(float(w[i, 0]), float(w[i, 1]), float(w[i, 2]), 0, 0, 0, int(cls[i]))
        else:
            og.collect_one(float(w[i, 0]), float(w[i, 1]), float(w[i, 2]), 0, 0, 0, 0)
    return og


def assert_same_grid(gg, og, what=""):
    assert gg.grid_params() == og.grid_params(), what
    assert gg.point_count() == og.point_count(), what
    gp, gk = gg.points(), gg.grid_cells()
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], og.grid_cells()), what
    assert gp[order].tobytes() == og.points().tobytes(), what


def run_all(ctx, scan, queries, xyz, cls, rgb, t, oracle=None, kinds=("count", "buffer", "grid")):
    """scan(pred, collector) for every query and collector kind, each against numpy (grids: the oracle).  rgb: the colours
    the scanned columns carry (None: no colour column)."""
    for q in queries:
        sel = q.select(xyz, cls, t)
        for kind in kinds:
            what = (q, kind)
            g = {"count": ctx.count_collector, "buffer": ctx.buffer_collector,
                 "grid": lambda: ctx.grid_collector(GRID_BOX[0], GRID_BOX[1], CELL)}[kind]()
            try:
                scan(q.pred(), g)
                if kind != "grid":
                    assert g.point_count() == int(sel.sum()), what
                if kind == "buffer":
                    assert g.points().tobytes() == q.records(xyz, cls, rgb, sel).tobytes(), what
                elif kind == "grid":
                    og = oracle_grid(oracle, q, xyz, cls, rgb, sel)
                    assert_same_grid(g, og, what)
                    og.free()
            finally:
                g.free()


BOX = ([-2000, -3000, -500], [2500, 1000, 600])
# (for ti.points: x, y in [-5000, 5000), z in [-1000, 1000), classes 1, 2, 6, times in [1000, 2000))
QUERIES = [Query(*BOX, cls=2), Query(*BOX, cls=6), Query(*BOX, start=1200.0, end=1700.0)]


# ---------------------------------------------------------------------------------------------------------------------
# the fast count (K1 with a second column) and the strided count
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", range(8))
def test_fast_count_at_every_byte_phase(gpu_ctx, phase):
    """A million points (enough steps for every workgroup's software pipeline to turn): positions at 4-byte phase 0..3 mod
    16 (the head peel), class bytes at phase 0..7 and times at 8-byte phase 0 / 8 mod 16 (the fast kernel) or 1..7 (the
    strided kernel), each against numpy; adversarial times on and around the range's bounds."""
    n = 1_000_003 + 97 * phase
    xyz, cls, _, _ = ti.points(n, 500 + phase)
    start, end = -0.5, 0.5
    t = ti.adversarial_times(n, start, end, phase)
    dev = Dev(gpu_ctx)
    try:
        d_xyz = dev.put(xyz, pad=4 * (phase % 4))
        d_cls = dev.put(cls, pad=phase)
        queries = [Query(*BOX, cls=c) for c in (1, 2, 6, 7)] + [
            Query([-5000] * 3, [5000] * 3, cls=2),                   # every position
            Query([-1, -1, -1], [-2, 0, 0], cls=2),                 # empty (lmin > lmax)
            Query([I32_MAX + 1, 0, 0], [I32_MAX + 5, 1, 1], cls=2),  # outside i32
            Query([I32_MIN - 10, I32_MIN - 10, I32_MIN - 10], [I32_MAX + 10] * 3, cls=1)]  # clamped to everything
        cols = binding.make_columns(xyz=d_xyz, cls=d_cls, n=n, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), queries, xyz, cls, None, t, kinds=("count",))
        for tpad in (phase, 8 + phase):
            d_t = dev.put(t, pad=tpad)
            tcols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))
            tq = [Query(*BOX, start=a, end=b) for a, b in ti.RANGES] + [Query([-5000] * 3, [5000] * 3, start=start, end=end),
                                                                        Query([3, 3, 3], [2, 2, 2], start=-np.inf, end=np.inf)]
            run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(tcols, p, g), tq, xyz, cls, None, t, kinds=("count",))
    finally:
        dev.free()


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 511, 512, 513, 4096 + 7, 3 * 512 * 100 + 300])
def test_fast_count_at_small_and_ragged_sizes(gpu_ctx, n):
    """Fewer than a tile, whole tiles and steps, leftover tiles behind the last step, and the tail of single points."""
    xyz, cls, _, t = ti.points(n, n)
    dev = Dev(gpu_ctx)
    try:
        for pad in (0, 4, 12):
            d_xyz, d_cls, d_t = dev.put(xyz, pad=pad), dev.put(cls, pad=pad + 1), dev.put(t, pad=8 * (pad % 8 == 4))
            cols = binding.make_columns(xyz=d_xyz, cls=d_cls, n=n, scale=list(ti.SCALE), offset=list(ti.OFFSET))
            tcols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))
            run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), QUERIES[:2], xyz, cls, None, t, kinds=("count",))
            run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(tcols, p, g), QUERIES[2:], xyz, cls, None, t, kinds=("count",))
    finally:
        dev.free()


def test_box_faces_and_i32_extremes(oracle, gpu_ctx):
    """Points on every face of the box and at the i32 extremes: the compares are inclusive, in i64."""
    rng = np.random.default_rng(3)
    n = 50_000
    vals = np.array([I32_MIN, I32_MIN + 1, -11, -10, -9, 0, 9, 10, 11, I32_MAX - 1, I32_MAX], dtype=np.int64)
    xyz = rng.choice(vals, (n, 3)).astype(np.int32)
    cls = rng.choice(np.array([0, 2, 255], dtype=np.uint8), n)
    t = rng.choice(np.array([-1.0, 0.0, 1.0, np.nan]), n)
    dev = Dev(gpu_ctx)
    try:
        d_xyz, d_cls, d_t = dev.put(xyz), dev.put(cls, pad=3), dev.put(t)
        qs_c = [Query([-10] * 3, [10] * 3, cls=c) for c in (0, 2, 255)] + [
            Query([I32_MIN] * 3, [I32_MAX] * 3, cls=255), Query([I32_MAX] * 3, [I32_MAX] * 3, cls=2),
            Query([I32_MIN] * 3, [I32_MIN] * 3, cls=0), Query([I32_MIN - 1] * 3, [-10] * 3, cls=2),
            Query([10, -10, I32_MIN], [I32_MAX + 7, 10, 0], cls=0)]
        qs_t = [Query([-10] * 3, [10] * 3, start=0.0, end=1.0), Query([I32_MIN] * 3, [I32_MAX] * 3, start=-1.0, end=1.0),
                Query([-10] * 3, [10] * 3, start=np.nan, end=1.0), Query([-10] * 3, [10] * 3, start=1.0, end=1.0)]
        cols = binding.make_columns(xyz=d_xyz, cls=d_cls, n=n, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        tcols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), qs_c, xyz, cls, None, t, kinds=("count", "buffer"))
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(tcols, p, g), qs_t, xyz, cls, None, t, kinds=("count", "buffer"))
    finally:
        dev.free()


def test_absent_class_every_point_matching_nan_and_empty_ranges(oracle, gpu_ctx):
    n = 300_007
    xyz, cls, rgb, t = ti.points(n, 21)
    everything = ([-5000] * 3, [5000] * 3)
    one = np.full(n, 2, dtype=np.uint8)
    dev = Dev(gpu_ctx)
    try:
        d_xyz, d_cls, d_one, d_t = dev.put(xyz), dev.put(cls), dev.put(one), dev.put(t)
        cols = binding.make_columns(xyz=d_xyz, cls=d_cls, n=n, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        ones = binding.make_columns(xyz=d_xyz, cls=d_one, n=n, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        tcols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), [Query(*everything, cls=3), Query(*BOX, cls=0)], xyz, cls, None, t,
                kinds=("count", "buffer"))
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(ones, p, g), [Query(*everything, cls=2)], xyz, one, None, t, oracle,
                kinds=("count", "buffer"))
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(tcols, p, g),
                [Query(*everything, start=-np.inf, end=np.inf), Query(*everything, start=np.nan, end=np.inf),
                 Query(*everything, start=0.0, end=np.nan), Query(*BOX, start=1500.0, end=1500.0), Query(*BOX, start=1600.0, end=1500.0)],
                xyz, cls, None, t, kinds=("count", "buffer"))
    finally:
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# records and grids: packed (LAST) and strided (LAS) columns
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 1, 2, 3, 5])
def test_packed_records_and_grids(oracle, gpu_ctx, phase):
    n = 70_001 + phase
    xyz, cls, rgb, t = ti.points(n, 600 + phase)
    dev = Dev(gpu_ctx)
    try:
        d_xyz, d_cls, d_rgb, d_t = dev.put(xyz, pad=4 * (phase % 4)), dev.put(cls, pad=phase), dev.put(rgb, pad=2 * phase), dev.put(t, pad=8 * (phase % 2))
        cols = binding.make_columns(xyz=d_xyz, cls=d_cls, rgb=d_rgb, n=n, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        nocol = binding.make_columns(xyz=d_xyz, cls=d_cls, n=n, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        tcols = binding.make_columns(xyz=d_xyz, cls=d_t, rgb=d_rgb, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), QUERIES[:2], xyz, cls, rgb, t, oracle)
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(nocol, p, g), QUERIES[:1], xyz, cls, None, t, oracle)
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(tcols, p, g), QUERIES[2:], xyz, cls, rgb, t, oracle)  # (rgb ignored)
    finally:
        dev.free()


@pytest.mark.parametrize("fmt", [1, 3, 6, 7, 8])
def test_strided_las_records_and_grids(oracle, gpu_ctx, fmt):
    """LAS records: the class byte at +15 (formats 1-5) or +16 (6-10), the time at +20 / +22, colour where the format has
    one; the records carry the class search's class byte and colour (BOUNDS_CLASS) or class 0 and no colour (BOUNDS_TIME)."""
    n = 40_003
    xyz, cls, rgb, t = ti.points(n, 700 + fmt)
    rl, toff, coff, kof = ti.FORMATS[fmt]
    rec = ti.records(fmt, xyz, cls, rgb, t)
    dev = Dev(gpu_ctx)
    try:
        for pad in (0, 3):
            base = dev.put(rec.reshape(-1), pad=pad)
            rgbp = base + coff if coff else None
            cols = binding.make_columns(xyz=base, cls=base + kof, rgb=rgbp, n=n, xyz_stride=rl, cls_stride=rl, rgb_stride=rl,
                                        scale=list(ti.SCALE), offset=list(ti.OFFSET))
            tcols = binding.make_columns(xyz=base, cls=base + toff, rgb=rgbp, n=n, xyz_stride=rl, cls_stride=rl, rgb_stride=rl,
                                         scale=list(ti.SCALE), offset=list(ti.OFFSET))
            run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), QUERIES[:2], xyz, cls, rgb if coff else None, t, oracle)
            run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(tcols, p, g), QUERIES[2:], xyz, cls, None, t, oracle)
    finally:
        dev.free()


def test_class_records_against_the_oracle_bounds_search(oracle, gpu_ctx):
    """An oracle-synthesised LAST file: the combined records equal the oracle's bounds-search records whose class is C."""
    spec = specs.synth_ca13(points_per_file=200_003, files=1)[0]
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    n, otp = hdr.number_of_points, hdr.offset_to_point_data
    bmin, bmax = specs.box("ca13_XL")
    ob = oracle.buffer_collector()
    assert oracle.search_last_bounds(image, bmin, bmax, ob) == 0
    want = ob.points()
    ob.free()
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
    coff = {2: 20, 3: 28, 5: 28}.get(hdr.point_data_record_format)
    cols = binding.make_columns(xyz=image.ctypes.data + otp, cls=image.ctypes.data + otp + 15 * n,
                                rgb=image.ctypes.data + otp + coff * n if coff else None, n=n, scale=list(hdr.scale), offset=list(hdr.offset))
    for c in np.unique(want["classification"])[:3]:
        gb, cc = gpu_ctx.buffer_collector(), gpu_ctx.count_collector()
        pred = pkg.Predicate.bounds_class(lmin, lmax, int(c))
        gpu_ctx.scan_host(cols, pred, gb)
        gpu_ctx.scan_host(cols, pred, cc)
        sub = want[want["classification"] == c]
        assert cc.point_count() == gb.point_count() == len(sub) > 0
        assert gb.points().tobytes() == sub.tobytes()
        gb.free(), cc.free()


# ---------------------------------------------------------------------------------------------------------------------
# files through the host and file paths, across staging-chunk seams
# ---------------------------------------------------------------------------------------------------------------------
def _file_cols(fmt, layout, n, base, attr):
    otp = 375 if fmt >= 6 else 227
    rl, toff, coff, kof = ti.FORMATS[fmt]
    sc = dict(scale=list(ti.SCALE), offset=list(ti.OFFSET))
    if layout == "las":
        rgb = base + otp + coff if (coff and attr == "class") else None
        return binding.make_columns(xyz=base + otp, cls=base + otp + (kof if attr == "class" else toff), rgb=rgb, n=n, xyz_stride=rl,
                                    cls_stride=rl, rgb_stride=rl, **sc)
    if attr == "class":
        rgb = base + otp + n * coff if coff else None
        return binding.make_columns(xyz=base + otp, cls=base + otp + n * kof, rgb=rgb, n=n, **sc)
    return binding.make_columns(xyz=base + otp, cls=base + otp + n * toff, n=n, cls_stride=8, **sc)


@pytest.mark.parametrize("layout,fmt", [("las", 1), ("las", 3), ("las", 7), ("last", 3), ("last", 6)])
def test_host_and_fd_scans_across_staging_chunk_seams(oracle, tmp_path, layout, fmt):
    n = 3 * 4099 + 1_234
    xyz, cls, rgb, t = ti.points(n, 800 + fmt)
    img = ti.las_image(fmt, xyz, cls, rgb, t) if layout == "las" else ti.last_image(fmt, xyz, cls, rgb, t)
    path = tmp_path / f"f.{layout}"
    img.tofile(path)
    coff = ti.FORMATS[fmt][2]
    qc = [Query(*BOX, cls=2)]
    qt = [Query(*BOX, start=float(t[4095]), end=float(t[4099 * 2 + 3]))]  # starts and ends at a seam
    fd = os.open(path, os.O_RDONLY)
    try:
        with pkg.Context(0) as ctx:
            for chunk in (4096, 4099):
                for mode in (0, 1, 2):
                    ctx.set_option("chunk_points", chunk)
                    ctx.set_option("host_in_place", mode)
                    for attr, qs, rgbs in (("class", qc, rgb if coff else None), ("time", qt, None)):
                        hc, fc = _file_cols(fmt, layout, n, img.ctypes.data, attr), _file_cols(fmt, layout, n, 0, attr)
                        run_all(ctx, lambda p, g: ctx.scan_host(hc, p, g), qs, xyz, cls, rgbs, t, oracle)
                        run_all(ctx, lambda p, g: ctx.scan_fd(fd, fc, p, g), qs, xyz, cls, rgbs, t, oracle)
                        for coll in (ctx.count_collector(), ctx.buffer_collector()):  # the _nowait forms
                            ctx.scan_host_nowait(hc, qs[0].pred(), coll)
                            ctx.scan_fd_nowait(fd, fc, qs[0].pred(), coll)
                            ctx.synchronize()
                            sel = qs[0].select(xyz, cls, t)
                            assert coll.point_count() == 2 * int(sel.sum()), (attr, chunk, mode)
                            coll.free()
    finally:
        os.close(fd)


def test_two_files_into_one_buffer_and_grid(oracle, tmp_path):
    """Two LAS files scanned back to back (scan_fd_nowait, first_index continuing) into one buffer and one grid."""
    n = 2 * 4099 + 17
    xyz, cls, rgb, t = ti.points(n, 9)
    img = ti.las_image(7, xyz, cls, rgb, t)
    paths = [tmp_path / "a.las", tmp_path / "b.las"]
    for p in paths:
        img.tofile(p)
    fds = [os.open(p, os.O_RDONLY) for p in paths]
    try:
        with pkg.Context(0) as ctx:
            ctx.set_option("chunk_points", 4099)
            for q, attr, rgbs in ((Query(*BOX, cls=2), "class", rgb), (Query(*BOX, start=1300.0, end=1800.0), "time", None)):
                sel = q.select(xyz, cls, t)
                want = np.concatenate([q.records(xyz, cls, rgbs, sel)] * 2)
                og = oracle_grid(oracle, q, xyz, cls, rgbs, sel)
                og = oracle_grid(oracle, q, xyz, cls, rgbs, sel, og)
                gb, gg = ctx.buffer_collector(), ctx.grid_collector(GRID_BOX[0], GRID_BOX[1], CELL)
                for k, fd in enumerate(fds):
                    cols = _file_cols(7, "las", n, 0, attr)
                    cols.first_index = k * n
                    for coll in (gb, gg):
                        ctx.scan_fd_nowait(fd, cols, q.pred(), coll)
                ctx.synchronize()
                assert gb.points().tobytes() == want.tobytes(), attr
                assert_same_grid(gg, og, attr)
                gb.free(), gg.free(), og.free()
    finally:
        for fd in fds:
            os.close(fd)


# ---------------------------------------------------------------------------------------------------------------------
# the chunk index serves the combined kinds unindexed and keeps its own state; the batch refuses them
# ---------------------------------------------------------------------------------------------------------------------
def test_indexed_fall_through_leaves_the_index_alone(gpu_ctx):
    n = 400_003
    xyz, cls, _, t = ti.points(n, 11)
    xyz = xyz[np.argsort(xyz[:, 0], kind="stable")]  # coherent in x: a box prunes most chunks
    dev = Dev(gpu_ctx)
    ix = gpu_ctx.index_new()
    try:
        d_xyz, d_cls, d_t = dev.put(xyz), dev.put(cls), dev.put(t)
        cols = binding.make_columns(xyz=d_xyz, cls=d_cls, n=n, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        tcols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        bpred = pkg.Predicate.bounds([-100, -5000, -1000], [100, 5000, 1000])
        want_b = int(inside(xyz, [-100, -5000, -1000], [100, 5000, 1000]).sum())
        cc = gpu_ctx.count_collector()
        gpu_ctx.scan_dev_indexed(cols, bpred, ix, cc)  # builds the index
        cc.free()
        cc = gpu_ctx.count_collector()
        gpu_ctx.scan_dev_indexed(cols, bpred, ix, cc)
        assert cc.point_count() == want_b
        cc.free()
        before = gpu_ctx.index_stats(ix)
        assert before["skipped"] > 0 and before["built"] == 0, before
        for c, q in ((cols, Query(*BOX, cls=2)), (tcols, Query(*BOX, start=1200.0, end=1300.0))):
            sel = q.select(xyz, cls, t)
            for make in (gpu_ctx.count_collector, gpu_ctx.buffer_collector):
                a, b = make(), make()
                gpu_ctx.scan_dev_indexed(c, q.pred(), ix, a)
                st = gpu_ctx.index_stats(ix)
                assert not any(st.values()), st
                gpu_ctx.scan_dev(c, q.pred(), b)
                assert a.point_count() == b.point_count() == int(sel.sum())
                if a.has_points():
                    assert a.points().tobytes() == b.points().tobytes() == q.records(xyz, cls, None, sel).tobytes()
                a.free(), b.free()
        cc = gpu_ctx.count_collector()
        gpu_ctx.scan_dev_indexed(cols, bpred, ix, cc)  # still pruned by the index it had
        assert cc.point_count() == want_b
        cc.free()
        after = gpu_ctx.index_stats(ix)
        assert after == before, (before, after)
        total = dev.put(np.zeros(1, dtype=np.uint64))
        for p in (Query(*BOX, cls=2).pred(), Query(*BOX, start=0.0, end=1.0).pred()):
            with pytest.raises(Exception):
                gpu_ctx.scan_dev_count_batch([cols], [p], total)
    finally:
        gpu_ctx.index_free(ix)
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# the CLI and the C view
# ---------------------------------------------------------------------------------------------------------------------
def _query(args, env=None):
    r = subprocess.run([QUERY] + args, capture_output=True, text=True, timeout=300, env=env)
    return r.returncode, r.stdout, r.stderr


def _read_dump(path):
    b = open(path, "rb").read()
    n = struct.unpack_from("<I", b, 107)[0]
    scale = struct.unpack_from("<3d", b, 131)
    off = struct.unpack_from("<3d", b, 155)
    rec = np.frombuffer(b[227:227 + 26 * n], dtype=np.uint8).reshape(n, 26)
    xyz = rec[:, :12].copy().view("<i4").reshape(n, 3).astype(np.float64)
    w = np.stack([xyz[:, a] * scale[a] + off[a] for a in range(3)], axis=1)
    return w, rec[:, 15], rec[:, 20:26].copy().view("<u2").reshape(n, 3), scale[0]


def _rows(w, c, col):
    return np.concatenate([np.round(w, 6), c[:, None].astype(np.float64), col.astype(np.float64)], axis=1)


def _rows_close(got, want, tol):
    assert tol < 0.005
    got, want = got[np.lexsort(np.round(got, 6).T[::-1])], want[np.lexsort(np.round(want, 6).T[::-1])]
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= tol))


@pytest.mark.parametrize("parallel", [False, True])
@pytest.mark.parametrize("attr", ["class", "time"])
def test_cli_count_records_and_density_on_las_and_last(oracle, tmp_path, parallel, attr):
    """`query --combine --bounds B (--class C | --time S;E)` over format-3/6 LAS and LAST files: the count line, the -o
    records decoded (class byte and colour of the class search; class 0 and colour 0 of the time search), and the
    --density cells over the query box — one grid fed in the driver's file order, or one grid per file in --parallel."""
    d = tmp_path / "data"
    d.mkdir()
    data = {}
    for k, (fmt, layout) in enumerate([(3, "las"), (6, "las"), (3, "last"), (6, "last")]):
        xyz, cls, rgb, t = ti.points(5_000 + 1_000 * k, 900 + k)
        img = ti.las_image(fmt, xyz, cls, rgb, t) if layout == "las" else ti.last_image(fmt, xyz, cls, rgb, t)
        img.tofile(d / f"f{k}.{layout}")
        data[f"f{k}.{layout}"] = (xyz, cls, rgb if fmt == 3 else np.zeros_like(rgb), t)
    order = os.listdir(d)
    bmin, bmax = (60.0, -250.0, -20.0), (140.0, -150.0, 40.0)
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(ti.SCALE), list(ti.OFFSET))
    q = Query(lmin, lmax, cls=2) if attr == "class" else Query(lmin, lmax, start=1250.0, end=1500.0)
    flags = ["-i", str(d), "--combine", "--bounds", ";".join(map(str, bmin + bmax)), "--optimized"]
    flags += ["--class", "2"] if attr == "class" else ["--time", "1250;1500"]
    flags += ["--parallel"] if parallel else []
    sels = {f: q.select(v[0], v[1], v[3]) for f, v in data.items()}
    total = sum(int(s.sum()) for s in sels.values())
    assert total > 100
    rc, out, err = _query(flags)
    assert rc == 0, err
    assert f"Found {total} matching points" in out.splitlines() and "Point record size" not in out

    def want_rows(f, sel):
        xyz, cls, rgb, _ = data[f]
        c = cls[sel] if attr == "class" else np.zeros(int(sel.sum()), np.uint8)
        col = rgb[sel] if attr == "class" else np.zeros((int(sel.sum()), 3), np.uint16)
        return _rows(ti.world(xyz[sel]), c, col)

    o = tmp_path / "out"
    o.mkdir()
    rc, out, err = _query(flags + ["-o", str(o)])
    assert rc == 0, err
    assert not any(line.startswith("Found ") for line in out.splitlines())
    got = [_read_dump(o / f) for f in os.listdir(o)]
    want = np.concatenate([want_rows(f, sels[f]) for f in order])
    assert _rows_close(np.concatenate([_rows(*g[:3]) for g in got]), want, max(g[3] for g in got) / 2 + 1e-9)

    dens = tmp_path / "dens"
    dens.mkdir()
    rc, out, err = _query(flags + ["--density", "20", "-o", str(dens)])
    assert rc == 0, err
    groups = [[f] for f in order] if parallel else [order]
    want_pts = []
    for group in groups:
        og = oracle.grid_collector(bmin, bmax, 20.0)
        for f in group:
            xyz, cls, rgb, _ = data[f]
            w = ti.world(xyz)
            for i in np.flatnonzero(sels[f]):
                if attr == "class":
                    og.collect_one(float(w[i, 0]), float(w[i, 1]), float(w[i, 2]), int(rgb[i, 0]), int(rgb[i, 1]), int(rgb[i, 2]), int(cls[i]))
                else:
                    og.collect_one(float(w[i, 0]), float(w[i, 1]), float(w[i, 2]), 0, 0, 0, 0)
        p = og.points()
        want_pts.append(_rows(np.stack([p["x"], p["y"], p["z"]], axis=1), p["classification"], np.stack([p["r"], p["g"], p["b"]], axis=1)))
        og.free()
    got = [_read_dump(dens / f) for f in os.listdir(dens)]
    assert len(got) == len(groups)
    assert _rows_close(np.concatenate([_rows(*g[:3]) for g in got]), np.concatenate(want_pts), max(g[3] for g in got) / 2 + 1e-9)


@pytest.mark.parametrize("name,msg", [("f.laz", "compressed format .laz"), ("f.lazer", "combined search in .lazer files")])
def test_cli_refuses_laz_and_lazer(tmp_path, name, msg):
    d = tmp_path / "data"
    d.mkdir()
    (d / name).write_bytes(b"\0" * 512)
    for attr in (["--class", "2"], ["--time", "0;1"]):
        rc, out, err = _query(["-i", str(d), "--combine", "--bounds", "0;0;0;1;1;1", "--optimized"] + attr)
        assert rc == 1 and msg in err and "outside the MI355X hot path" in err, err


def test_cli_regular_implementation_fails_like_the_other_searches(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    xyz, cls, rgb, t = ti.points(100, 1)
    ti.las_image(1, xyz, cls, rgb, t).tofile(d / "f.las")
    rc, _, err = _query(["-i", str(d), "--combine", "--bounds", "0;0;0;1;1;1", "--time", "0;1"])
    rc_b, _, err_b = _query(["-i", str(d), "--class", "2"])
    assert rc == rc_b == 1 and "the Regular (non --optimized) search implementation" in err
    assert err == err_b


def test_c_view_search_file_bounds_class_and_time(tmp_path):
    q = pkg.load_query_library()
    D3 = C.c_double * 3
    xyz, cls, rgb, t = ti.points(10_000, 3)
    bmin, bmax = (60.0, -250.0, -20.0), (140.0, -150.0, 40.0)
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(ti.SCALE), list(ti.OFFSET))
    for layout in ("las", "last"):
        p = tmp_path / f"f.{layout}"
        (ti.las_image(6, xyz, cls, rgb, t) if layout == "las" else ti.last_image(6, xyz, cls, rgb, t)).tofile(p)
        c = C.c_void_p()
        assert q.pcq_query_collector_new_count(0, C.byref(c)) == 0
        try:
            assert q.pcq_query_search_file_bounds_class(str(p).encode(), D3(*bmin), D3(*bmax), 2, 1, c) == 0
            assert q.pcq_query_search_file_bounds_time(str(p).encode(), D3(*bmin), D3(*bmax), 1300.0, 1400.0, 1, c) == 0
            n = C.c_uint64()
            assert q.pcq_query_collector_point_count(c, C.byref(n)) == 0
            want = Query(lmin, lmax, cls=2).select(xyz, cls, t).sum() + Query(lmin, lmax, start=1300.0, end=1400.0).select(xyz, cls, t).sum()
            assert n.value == int(want) > 0
            assert q.pcq_query_search_file_bounds_class(str(p).encode(), D3(*bmin), D3(*bmax), 2, 0, c) == -11  # Regular
        finally:
            q.pcq_query_collector_free(c)


# ---------------------------------------------------------------------------------------------------------------------
# one full-size resident count
# ---------------------------------------------------------------------------------------------------------------------
def test_full_size_count_against_the_closed_form(gpu_ctx):
    """163 M points with x = i mod 1024, y = (i >> 10) mod 1024, z = i >> 20, class = x mod 8 and time = i: the box x in
    [100, 611], z in [10, 99] holds 90 * 1024 * 512 points, 90 * 1024 * 64 of class 3, and 30 * 1024 * 512 with a time in
    [20 * 2^20, 50 * 2^20)."""
    n = 163_000_000
    dev = Dev(gpu_ctx)
    try:
        d_xyz, d_cls, d_t = gpu_ctx.alloc(12 * n + 64), gpu_ctx.alloc(n + 64), gpu_ctx.alloc(8 * n + 64)
        dev.blocks += [d_xyz, d_cls, d_t]
        step = 8 << 20
        for i0 in range(0, n, step):
            i = np.arange(i0, min(n, i0 + step), dtype=np.int64)
            x, y, z = i & 1023, (i >> 10) & 1023, i >> 20
            gpu_ctx.to_device(d_xyz + 12 * i0, np.stack([x, y, z], axis=1).astype(np.int32))
            gpu_ctx.to_device(d_cls + i0, (x & 7).astype(np.uint8))
            gpu_ctx.to_device(d_t + 8 * i0, i.astype(np.float64))
        cols = binding.make_columns(xyz=d_xyz, cls=d_cls, n=n)
        tcols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8)
        lo, hi = [100, -5, 10], [611, 2000, 99]
        for c, pred, want in [(cols, pkg.Predicate.bounds_class(lo, hi, 3), 90 * 1024 * 64),
                              (cols, pkg.Predicate.bounds_class(lo, hi, 8), 0),
                              (tcols, pkg.Predicate.bounds_time(lo, hi, 20.0 * 2**20, 50.0 * 2**20), 30 * 1024 * 512),
                              (tcols, pkg.Predicate.bounds_time(lo, hi, -1.0, 1e12), 90 * 1024 * 512)]:
            cc = gpu_ctx.count_collector()
            gpu_ctx.scan_dev(c, pred, cc)
            assert cc.point_count() == want
            cc.free()
    finally:
        dev.free()
