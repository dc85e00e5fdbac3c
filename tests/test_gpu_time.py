"""The GPS time-range search (PCQ_PRED_TIME) on the GPU: counts, records and grids against numpy and the oracle's SparseGrid.

Expected results: sel = (t >= start) & (t < end) on float64 (NaN -> False); a match's record is x * scale + offset with
class 0 and colour (0, 0, 0) (las.rs:345-355) even where the file has both; a grid is the oracle's SparseGrid fed the
selected points in file order.  Covered: every byte phase of a packed (K3) and a strided time column through pcq_scan_dev,
IEEE edge values around both bounds, LAS formats 1, 3, 6, 7, 8 and LAST files, host and file scans across staging-chunk
seams, two files into one collector, the chunk index's fall-through, the CLI, and one full-size column.
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
POINT_DTYPE = binding.POINT_DTYPE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY = os.path.join(ROOT, "adhoc-queries-pointclouds_amd", "host", "query")
GRID_BOX = ((-60.0, -400.0, -50.0), (160.0, 0.0, 60.0))
CELL = 2.5


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


def oracle_grid(oracle, xyz, sel, og=None):
    og = og or oracle.grid_collector(GRID_BOX[0], GRID_BOX[1], CELL)
    w = ti.world(xyz)
    for i in np.flatnonzero(sel):
        og.collect_one(float(w[i, 0]), float(w[i, 1]), float(w[i, 2]), 0, 0, 0, 0)
    return og


def assert_same_grid(gg, og, what=""):
    assert gg.grid_params() == og.grid_params(), what
    assert gg.point_count() == og.point_count(), what
    gp, gk = gg.points(), gg.grid_cells()
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], og.grid_cells()), what
    assert gp[order].tobytes() == og.points().tobytes(), what


def run_all(ctx, scan, xyz, t, ranges, oracle=None, kinds=("count", "buffer", "grid")):
    """scan(pred, collector) for every range and collector kind, each against numpy (grids: the oracle)."""
    for start, end in ranges:
        sel = ti.select(t, start, end)
        pred = pkg.Predicate.time_range(start, end)
        for kind in kinds:
            what = (start, end, kind)
            g = {"count": ctx.count_collector, "buffer": ctx.buffer_collector,
                 "grid": lambda: ctx.grid_collector(GRID_BOX[0], GRID_BOX[1], CELL)}[kind]()
            try:
                scan(pred, g)
                if kind != "grid":  # (a grid's point count is its number of cells)
                    assert g.point_count() == int(sel.sum()), what
                if kind == "buffer":
                    assert g.points().tobytes() == ti.expect_records(xyz, sel, POINT_DTYPE).tobytes(), what
                elif kind == "grid":
                    og = oracle_grid(oracle, xyz, sel)
                    assert_same_grid(g, og, what)
                    og.free()
            finally:
                g.free()


# ---------------------------------------------------------------------------------------------------------------------
# pcq_scan_dev: packed and strided columns at all eight byte phases, adversarial times
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", range(8))
def test_packed_time_column_at_every_byte_phase(oracle, gpu_ctx, phase):
    """A LAST-like time block (stride 8) at address phase 0..7 mod 8 (and both 16-byte phases of the 8-aligned ones):
    K3 where the block is 8-byte aligned, the strided kernel otherwise; the same counts, records and grids."""
    n = 70_001 + phase
    xyz, _, _, _ = ti.points(n, 100 + phase)
    start, end = -0.5, 0.5
    t = ti.adversarial_times(n, start, end, phase)
    dev = Dev(gpu_ctx)
    try:
        d_xyz = dev.put(xyz)
        for extra in (0, 8):
            d_t = dev.put(t, pad=phase + extra)
            cols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))
            run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), xyz, t, ti.RANGES if extra == 0 else ti.RANGES[:3], oracle,
                    kinds=("count", "buffer", "grid") if extra == 0 else ("count",))
            # a count that does not need positions gets none
            count_cols = binding.make_columns(cls=d_t, n=n, cls_stride=8)
            cc = gpu_ctx.count_collector()
            gpu_ctx.scan_dev(count_cols, pkg.Predicate.time_range(start, end), cc)
            assert cc.point_count() == int(ti.select(t, start, end).sum())
            cc.free()
    finally:
        dev.free()


@pytest.mark.parametrize("phase", range(8))
def test_strided_time_column_at_every_byte_phase(oracle, gpu_ctx, phase):
    """LAS format-3 records (34 bytes: the time at +20 walks through every phase) placed at base phase 0..7."""
    n = 40_003
    xyz, cls, rgb, _ = ti.points(n, 200 + phase)
    t = ti.adversarial_times(n, 0.0, 1.0, 50 + phase)
    rec = ti.records(3, xyz, cls, rgb, t)
    dev = Dev(gpu_ctx)
    try:
        base = dev.put(rec.reshape(-1), pad=phase)
        cols = binding.make_columns(xyz=base, cls=base + 20, rgb=base + 28, n=n, xyz_stride=34, cls_stride=34, rgb_stride=34,
                                    scale=list(ti.SCALE), offset=list(ti.OFFSET))
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), xyz, t, ti.RANGES, oracle)
    finally:
        dev.free()


def test_records_carry_class_0_and_colour_0(oracle, gpu_ctx):
    """Every point of a file with classes and colours matches: the records and the grid winners still have class 0 and
    colour (0, 0, 0); small and large tiles take the sparse and the full emit."""
    n = 9_000
    xyz, cls, rgb, t = ti.points(n, 7)
    assert cls.min() > 0 and rgb.min() > 0
    rec = ti.records(7, xyz, cls, rgb, t)
    dev = Dev(gpu_ctx)
    try:
        base = dev.put(rec.reshape(-1))
        cols = binding.make_columns(xyz=base, cls=base + 22, rgb=base + 30, n=n, xyz_stride=36, cls_stride=36, rgb_stride=36,
                                    scale=list(ti.SCALE), offset=list(ti.OFFSET))
        lo = float(t[10])
        run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), xyz, t, [(-np.inf, np.inf), (lo, float(t[40])), (lo, float(t[4000]))],
                oracle, kinds=("buffer", "grid"))
        gb = gpu_ctx.buffer_collector()
        gpu_ctx.scan_dev(cols, pkg.Predicate.time_range(-np.inf, np.inf), gb)
        pts = gb.points()
        gb.free()
        assert len(pts) == n and not pts["classification"].any() and not pts["r"].any() and not pts["g"].any() and not pts["b"].any()
    finally:
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# LAS formats and LAST files through the host and file paths, across staging-chunk seams
# ---------------------------------------------------------------------------------------------------------------------
def _file_cols(fmt, layout, n, base):
    otp = 375 if fmt >= 6 else 227
    toff = ti.time_offset(fmt)
    if layout == "las":
        rl = ti.FORMATS[fmt][0]
        return binding.make_columns(xyz=base + otp, cls=base + otp + toff, n=n, xyz_stride=rl, cls_stride=rl,
                                    scale=list(ti.SCALE), offset=list(ti.OFFSET))
    return binding.make_columns(xyz=base + otp, cls=base + otp + n * toff, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))


@pytest.mark.parametrize("fmt", [1, 3, 6, 7, 8])
def test_las_formats_through_the_host_path(oracle, gpu_ctx, fmt):
    n = 20_011
    xyz, cls, rgb, t = ti.points(n, fmt)
    img = ti.las_image(fmt, xyz, cls, rgb, t)
    cols = _file_cols(fmt, "las", n, img.ctypes.data)
    run_all(gpu_ctx, lambda p, g: gpu_ctx.scan_host(cols, p, g), xyz, t,
            [(1200.0, 1300.0), (float(t[5]), float(t[5])), (1500.0, 1400.0), (-np.inf, np.inf)], oracle)


@pytest.mark.parametrize("layout,fmt", [("las", 1), ("las", 3), ("las", 6), ("last", 3), ("last", 7)])
def test_host_and_fd_scans_across_staging_chunk_seams(oracle, tmp_path, layout, fmt):
    n = 3 * 4099 + 1_234
    xyz, cls, rgb, t = ti.points(n, 300 + fmt)
    img = ti.las_image(fmt, xyz, cls, rgb, t) if layout == "las" else ti.last_image(fmt, xyz, cls, rgb, t)
    path = tmp_path / f"f.{layout}"
    img.tofile(path)
    ranges = [(float(t[4095]), float(t[4099 * 2 + 3])), (1100.0, 1900.0)]  # the first starts and ends at a seam
    fd = os.open(path, os.O_RDONLY)
    try:
        with pkg.Context(0) as ctx:
            host_cols, fd_cols = _file_cols(fmt, layout, n, img.ctypes.data), _file_cols(fmt, layout, n, 0)
            for chunk in (4096, 4099):
                for mode in (0, 1, 2):
                    ctx.set_option("chunk_points", chunk)
                    ctx.set_option("host_in_place", mode)
                    run_all(ctx, lambda p, g: ctx.scan_host(host_cols, p, g), xyz, t, ranges, oracle)
                    run_all(ctx, lambda p, g: ctx.scan_fd(fd, fd_cols, p, g), xyz, t, ranges, oracle)
    finally:
        os.close(fd)


def test_two_files_into_one_buffer_and_grid_with_equal_times(oracle, tmp_path):
    """Two LAS files scanned back to back (scan_fd_nowait, first_index continuing) into one buffer and one grid: records in
    file order across files and seams; both files hold the SAME points and times, so every cell's tie goes to file one."""
    n = 2 * 4099 + 17
    xyz, cls, rgb, t = ti.points(n, 9)
    t[::7] = 1500.0
    img = ti.las_image(3, xyz, cls, rgb, t)
    paths = [tmp_path / "a.las", tmp_path / "b.las"]
    for p in paths:
        img.tofile(p)
    start, end = 1400.0, 1600.0
    sel = ti.select(t, start, end)
    want = np.concatenate([ti.expect_records(xyz, sel, POINT_DTYPE)] * 2)
    og = oracle_grid(oracle, xyz, sel)
    og = oracle_grid(oracle, xyz, sel, og)
    fds = [os.open(p, os.O_RDONLY) for p in paths]
    try:
        with pkg.Context(0) as ctx:
            for mode in (0, 1, 2):
                ctx.set_option("chunk_points", 4099)
                ctx.set_option("host_in_place", mode)
                gb, gg = ctx.buffer_collector(), ctx.grid_collector(GRID_BOX[0], GRID_BOX[1], CELL)
                for k, fd in enumerate(fds):
                    cols = _file_cols(3, "las", n, 0)
                    cols.first_index = k * n
                    for coll in (gb, gg):
                        ctx.scan_fd_nowait(fd, cols, pkg.Predicate.time_range(start, end), coll)
                ctx.synchronize()
                assert gb.points().tobytes() == want.tobytes(), mode
                assert_same_grid(gg, og, mode)
                gb.free(), gg.free()
    finally:
        for fd in fds:
            os.close(fd)
        og.free()


# ---------------------------------------------------------------------------------------------------------------------
# the chunk index serves TIME unindexed; the batch refuses it
# ---------------------------------------------------------------------------------------------------------------------
def test_indexed_scan_of_time_equals_the_plain_scan(gpu_ctx):
    n = 300_001
    xyz, _, _, t = ti.points(n, 11)
    dev = Dev(gpu_ctx)
    ix = gpu_ctx.index_new()
    try:
        d_xyz, d_t = dev.put(xyz), dev.put(t)
        cols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))
        # an index built by a bounds scan of the same positions first: TIME must not use it
        cc = gpu_ctx.count_collector()
        gpu_ctx.scan_dev_indexed(cols, pkg.Predicate.bounds([-100] * 3, [100] * 3), ix, cc)
        cc.free()
        for start, end in [(1200.0, 1300.0), (0.0, 1.0), (-np.inf, np.inf)]:
            sel = ti.select(t, start, end)
            pred = pkg.Predicate.time_range(start, end)
            for make in (gpu_ctx.count_collector, gpu_ctx.buffer_collector):
                a, b = make(), make()
                gpu_ctx.scan_dev_indexed(cols, pred, ix, a)
                st = gpu_ctx.index_stats(ix)
                assert st["skipped"] == 0 and st["whole"] == 0 and st["built"] == 0, st
                gpu_ctx.scan_dev(cols, pred, b)
                assert a.point_count() == b.point_count() == int(sel.sum())
                if a.has_points():
                    assert a.points().tobytes() == b.points().tobytes() == ti.expect_records(xyz, sel, POINT_DTYPE).tobytes()
                a.free(), b.free()
        total = dev.put(np.zeros(1, dtype=np.uint64))
        with pytest.raises(Exception):
            gpu_ctx.scan_dev_count_batch([cols], [pkg.Predicate.time_range(0.0, 1.0)], total)
    finally:
        gpu_ctx.index_free(ix)
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# the CLI
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
    return w, rec[:, 15], rec[:, 20:26], scale[0]


def _rows_close(got, want, tol):
    """The same rows in any order, up to the dump's quantisation (the positions here are multiples of 0.01 / 0.02 / 0.05:
    rounded to 1e-6 they sort alike)."""
    assert tol < 0.005
    got, want = np.round(got, 6), np.round(want, 6)
    got, want = got[np.lexsort(got.T[::-1])], want[np.lexsort(want.T[::-1])]
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= tol))


@pytest.mark.parametrize("parallel", [False, True])
def test_cli_count_records_and_density_on_las_and_last(oracle, tmp_path, parallel):
    """`query --time` over a directory of format-1/3 LAS and LAST files: the count line, the -o records decoded (class 0,
    colour 0), and the --density cells — one grid over get_total_bounds fed in the driver's file order (readdir), or one
    grid per file in --parallel — against the oracle's SparseGrid."""
    d = tmp_path / "data"
    d.mkdir()
    data = {}
    for k, (fmt, layout) in enumerate([(1, "las"), (3, "las"), (1, "last"), (3, "last")]):
        xyz, cls, rgb, t = ti.points(5_000 + 1_000 * k, 400 + k)
        img = ti.las_image(fmt, xyz, cls, rgb, t) if layout == "las" else ti.last_image(fmt, xyz, cls, rgb, t)
        img.tofile(d / f"f{k}.{layout}")
        data[f"f{k}.{layout}"] = (xyz, t)
    order = os.listdir(d)  # get_all_input_files: read_dir order
    start, end = 1250.0, 1500.0
    flags = ["-i", str(d), "--time", f"{start};{end}", "--optimized"] + (["--parallel"] if parallel else [])
    sels = {f: ti.select(t, start, end) for f, (xyz, t) in data.items()}
    total = sum(int(s.sum()) for s in sels.values())
    rc, out, err = _query(flags)
    assert rc == 0, err
    assert f"Found {total} matching points" in out.splitlines()

    o = tmp_path / "out"
    o.mkdir()
    rc, out, err = _query(flags + ["-o", str(o)])
    assert rc == 0, err
    got = [_read_dump(o / f) for f in os.listdir(o)]
    assert not any(g[1].any() or g[2].any() for g in got)  # class 0, colour (0, 0, 0)
    want = np.concatenate([ti.world(data[f][0][sels[f]]) for f in order])
    assert _rows_close(np.concatenate([g[0] for g in got]), want, max(g[3] for g in got) / 2 + 1e-9)

    dens = tmp_path / "dens"
    dens.mkdir()
    rc, out, err = _query(flags + ["--density", "20", "-o", str(dens)])
    assert rc == 0, err
    hb = [struct.unpack_from("<6d", open(d / f, "rb").read(), 179) for f in order]
    bmin = [min(h[2 * a + 1] for h in hb) for a in range(3)]
    bmax = [max(h[2 * a] for h in hb) for a in range(3)]
    groups = [[f] for f in order] if parallel else [order]
    want_pts = []
    for group in groups:
        og = oracle.grid_collector(bmin, bmax, 20.0)
        for f in group:
            w = ti.world(data[f][0])
            for i in np.flatnonzero(sels[f]):
                og.collect_one(float(w[i, 0]), float(w[i, 1]), float(w[i, 2]), 0, 0, 0, 0)
        p = og.points()
        want_pts.append(np.stack([p["x"], p["y"], p["z"]], axis=1))
        og.free()
    got = [_read_dump(dens / f) for f in os.listdir(dens)]
    assert len(got) == len(groups)
    assert not any(g[1].any() or g[2].any() for g in got)
    assert _rows_close(np.concatenate([g[0] for g in got]), np.concatenate(want_pts), max(g[3] for g in got) / 2 + 1e-9)


@pytest.mark.parametrize("name,msg", [("f.laz", "compressed format .laz"), ("f.lazer", "time search in .lazer files")])
def test_cli_refuses_laz_and_lazer(tmp_path, name, msg):
    d = tmp_path / "data"
    d.mkdir()
    (d / name).write_bytes(b"\0" * 512)
    rc, out, err = _query(["-i", str(d), "--time", "0;1", "--optimized"])
    assert rc == 1 and msg in err and "outside the MI355X hot path" in err, err


def test_cli_regular_implementation_fails_like_the_other_searches(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    xyz, cls, rgb, t = ti.points(100, 1)
    ti.las_image(1, xyz, cls, rgb, t).tofile(d / "f.las")
    rc, _, err = _query(["-i", str(d), "--time", "0;1"])
    rc_b, _, err_b = _query(["-i", str(d), "--class", "2"])
    assert rc == rc_b == 1 and "the Regular (non --optimized) search implementation" in err
    assert err == err_b


def test_c_view_search_file_time(tmp_path):
    """pcq_query_search_file_time == the CLI's per-file search: counts through the C view's count collector."""
    q = pkg.load_query_library()
    xyz, cls, rgb, t = ti.points(10_000, 3)
    p = tmp_path / "f.last"
    ti.last_image(6, xyz, cls, rgb, t).tofile(p)
    c = C.c_void_p()
    assert q.pcq_query_collector_new_count(0, C.byref(c)) == 0
    try:
        assert q.pcq_query_search_file_time(str(p).encode(), 1300.0, 1400.0, 1, c) == 0
        n = C.c_uint64()
        assert q.pcq_query_collector_point_count(c, C.byref(n)) == 0
        assert n.value == int(ti.select(t, 1300.0, 1400.0).sum())
        assert q.pcq_query_search_file_time(str(p).encode(), 1300.0, 1400.0, 0, c) == -11  # Regular
    finally:
        q.pcq_query_collector_free(c)


# ---------------------------------------------------------------------------------------------------------------------
# one full-size column
# ---------------------------------------------------------------------------------------------------------------------
def test_full_size_count_against_the_closed_form(gpu_ctx):
    """163 M times gps = i * 0.001 in HBM: [1000.0005, 50000.0005) holds i = 1,000,001 .. 50,000,000 exactly, [162999.9985, 1e9)
    only the last time (162999.999)."""
    n = 163_000_000
    dev = Dev(gpu_ctx)
    try:
        t = np.arange(n, dtype=np.float64) * 0.001
        d_t = dev.put(t)
        del t
        for start, end, want in [(1000.0005, 50000.0005, 49_000_000), (-1.0, 1e9, n), (162999.9985, 1e9, 1), (5.0, 5.0, 0)]:
            cols = binding.make_columns(cls=d_t, n=n, cls_stride=8)
            cc = gpu_ctx.count_collector()
            gpu_ctx.scan_dev(cols, pkg.Predicate.time_range(start, end), cc)
            assert cc.point_count() == want, (start, end)
            cc.free()
    finally:
        dev.free()
