"""GPU parity: the HIP scans (through the C ABI) against the oracle on the same seeded inputs.

Bar: bit-exact (integer / byte / index work; the f64 position rebuild is two IEEE roundings on both
sides, so result records are compared byte-for-byte as well).
"""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")


def small_spec(seed, n, fmt=2, scale=(0.01, 0.01, 0.01), offset=(0.0, 0.0, 0.0), lo=(-5000, -5000, -1000),
               span=(10001, 10001, 2001), zo=None, classes=((1, 0.5), (2, 0.3), (6, 0.2))):
    return specs._spec(seed, n, fmt, scale, offset, lo, span, zo=zo, classes=list(classes))


class DevFile:
    """A LAST image resident in HBM (whole image uploaded; column pointers computed like last.rs:68-90)."""

    def __init__(self, ctx, image: np.ndarray, hdr, pad=0):
        self.ctx = ctx
        self.n = hdr.number_of_points
        self.hdr = hdr
        self.base = ctx.alloc(image.size + 64 + pad)
        self.ptr = self.base + pad
        ctx.to_device(self.ptr, image)
        otp = hdr.offset_to_point_data
        fmt = hdr.point_data_record_format
        self.xyz = self.ptr + otp
        self.cls = self.ptr + otp + (15 if fmt <= 5 else 16) * self.n
        col = {2: 20, 3: 28, 5: 28}.get(fmt)
        self.rgb = self.ptr + otp + col * self.n if col is not None else None

    def columns(self, with_attrs=True):
        return binding.make_columns(xyz=self.xyz, cls=self.cls if with_attrs else None, rgb=self.rgb if with_attrs else None,
                                    n=self.n, scale=list(self.hdr.scale), offset=list(self.hdr.offset))

    def free(self):
        self.ctx.free(self.base)


BOXES = [
    ((-10.0, -10.0, -2.0), (10.0, 10.0, 2.0)),           # about a fifth of the volume
    ((-50.0, -50.0, -10.0), (50.0, 50.0, 10.0)),         # everything
    ((-0.005, -0.005, -0.005), (0.005, 0.005, 0.005)),   # a handful
    ((40.0, 40.0, 5.0), (41.0, 41.0, 6.0)),              # a corner
    ((49.99, -50.0, -10.0), (50.0, 50.0, 10.0)),         # the max face
]


@pytest.mark.parametrize("n", [0, 1, 3, 255, 256, 257, 511, 512, 513, 1000, 4099, 100_003, 1_000_003])
def test_bounds_count_dev_matches_oracle(oracle, gpu_ctx, n):
    spec = small_spec(1234 + n, n)
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    if True:
        for pad in (0, 4, 8, 12):  # positions block at every 4-byte phase of a 16-byte line
            f = DevFile(gpu_ctx, image, hdr, pad=pad + 5)  # 227 + 5 = 232 = 8 mod 16, then +pad
            try:
                for bmin, bmax in BOXES:
                    oc = oracle.count_collector()
                    assert oracle.search_last_bounds(image, bmin, bmax, oc) == 0
                    lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
                    cc = gpu_ctx.count_collector()
                    gpu_ctx.scan_dev(f.columns(False), pkg.Predicate.bounds(lmin, lmax), cc)
                    got = cc.point_count()
                    cc.free()
                    # the oracle applies the header-AABB early-out (last.rs:92-94) before scanning;
                    # the column scan has no header: compare only when the file is not skipped
                    if oracle.aabb_intersects(list(hdr.min), list(hdr.max), bmin, bmax):
                        assert got == oc.point_count(), (n, pad, bmin)
                    oc.free()
            finally:
                f.free()


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 31, 1000, 65_537, 1_000_003])
def test_class_count_dev_matches_oracle(oracle, gpu_ctx, n):
    spec = small_spec(99 + n, n, fmt=1)
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    for pad in (0, 1, 7, 13):
        f = DevFile(gpu_ctx, image, hdr, pad=pad)
        try:
            for cls in (1, 2, 6, 19, 0, 255):
                oc = oracle.count_collector()
                assert oracle.search_last_class(image, cls, oc) == 0
                cc = gpu_ctx.count_collector()
                gpu_ctx.scan_dev(f.columns(True), pkg.Predicate.classification(cls), cc)
                assert cc.point_count() == oc.point_count(), (n, pad, cls)
                cc.free()
                oc.free()
        finally:
            f.free()


def test_count_collector_accumulates_and_external_counter(oracle, gpu_ctx):
    spec = small_spec(7, 50_000)
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    f = DevFile(gpu_ctx, image, hdr)
    ext = gpu_ctx.alloc(16)
    gpu_ctx.memset(ext, 0, 16)
    try:
        bmin, bmax = BOXES[0]
        oc = oracle.count_collector()
        oracle.search_last_bounds(image, bmin, bmax, oc)
        lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
        cc = gpu_ctx.count_collector(device_counter=ext)
        for _ in range(3):  # sequential mode feeds several files into one collector (main.rs:129-133)
            gpu_ctx.scan_dev(f.columns(False), pkg.Predicate.bounds(lmin, lmax), cc)
        assert cc.point_count() == 3 * oc.point_count()
        host = np.zeros(1, dtype=np.uint64)
        gpu_ctx.to_host(host, ext)
        assert int(host[0]) == 3 * oc.point_count()
        cc.free()
        oc.free()
    finally:
        gpu_ctx.free(ext)
        f.free()


def test_count_batch_matches_sum_of_files(oracle, gpu_ctx):
    files, cols, preds, expect = [], [], [], 0
    bmin, bmax = (-20.0, -30.0, -3.0), (15.0, 45.0, 4.0)
    try:
        for i, n in enumerate([100_003, 0, 255, 256, 70_001, 1_000_003, 511, 512, 513, 767, 768, 769, 1535, 1536, 1537]):
            spec = small_spec(500 + i, n, offset=(float(i), 0.0, 0.0))
            image = oracle.synth_image(spec, transposed=True)
            hdr = oracle.parse_header(image[:400].tobytes())
            f = DevFile(gpu_ctx, image, hdr, pad=13)  # 227 + 13 = 240: 16-byte aligned positions block
            files.append(f)
            oc = oracle.count_collector()
            assert oracle.search_last_bounds(image, bmin, bmax, oc) == 0
            expect += oc.point_count()
            oc.free()
            lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
            cols.append(f.columns(False))
            preds.append(pkg.Predicate.bounds(lmin, lmax))
        total = gpu_ctx.alloc(16)
        gpu_ctx.memset(total, 0, 16)
        gpu_ctx.scan_dev_count_batch(cols, preds, total)
        gpu_ctx.scan_dev_count_batch(cols, preds, total)  # accumulates
        host = np.zeros(1, dtype=np.uint64)
        gpu_ctx.to_host(host, total)
        gpu_ctx.free(total)
        assert int(host[0]) == 2 * expect
    finally:
        for f in files:
            f.free()


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 300, 2048, 2049, 50_021])
def test_buffer_collector_dev_matches_oracle(oracle, gpu_ctx, fmt, n):
    spec = small_spec(4242 + n + fmt, n, fmt=fmt, scale=(0.01, 0.02, 0.05), offset=(100.0, -200.0, 7.5))
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    f = DevFile(gpu_ctx, image, hdr)
    try:
        for bmin, bmax in [((90.0, -250.0, 0.0), (120.0, -150.0, 20.0)), ((0.0, -400.0, -100.0), (200.0, 0.0, 100.0))]:
            ob = oracle.buffer_collector()
            assert oracle.search_last_bounds(image, bmin, bmax, ob) == 0
            lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
            gb = gpu_ctx.buffer_collector()
            gpu_ctx.scan_dev(f.columns(True), pkg.Predicate.bounds(lmin, lmax), gb)
            if oracle.aabb_intersects(list(hdr.min), list(hdr.max), bmin, bmax):
                assert gb.point_count() == ob.point_count()
                assert gb.points().tobytes() == ob.points().tobytes()  # same records, same (file) order
            gb.free()
            ob.free()
        for cls in (2, 6, 19):
            ob = oracle.buffer_collector()
            assert oracle.search_last_class(image, cls, ob) == 0
            gb = gpu_ctx.buffer_collector()
            gpu_ctx.scan_dev(f.columns(True), pkg.Predicate.classification(cls), gb)
            assert gb.points().tobytes() == ob.points().tobytes()
            gb.free()
            ob.free()
    finally:
        f.free()


@pytest.mark.parametrize("fmt", [1, 2, 3])
@pytest.mark.parametrize("sparse_max,park_max", [(0, 0), (1, 0), (9, 0), (256, 0), (2048, 0), (64, 256), (0, 256), (64, 1), (300, 37)])
def test_buffer_collector_sparse_and_dense_tiles_write_the_same_records(oracle, gpu_ctx, fmt, sparse_max, park_max):
    """The emit has three writers per scan: k_emit_points (a tile's whole image through LDS) for tiles with many matches,
    k_emit_parked for tiles with at most `emit_park_max` matches (bounds queries on files without a colour block: the count
    pass left the matches themselves, 16 bytes each) and k_emit_sparse (one wave per tile, from the match bits the count pass
    leaves) for tiles with at most `emit_sparse_max` where nothing is parked.
    Whatever the thresholds — never, one match, a few, the defaults, always — the records and their order are the oracle's:
    boxes that keep about 1 / 1000, 1 %, 10 %, a half and all of a file in random order, class queries, two scans appended
    into one collector (a record base that is no multiple of 16), a file whose last tile is ragged."""
    n = 2048 * 9 + 777
    spec = small_spec(9100 + fmt, n, fmt=fmt, scale=(0.01, 0.02, 0.05), offset=(100.0, -200.0, 7.5))
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    f = DevFile(gpu_ctx, image, hdr)
    lo, hi = np.array(hdr.min), np.array(hdr.max)
    gpu_ctx.set_option("emit_sparse_max", sparse_max)
    gpu_ctx.set_option("emit_park_max", park_max)
    try:
        ob, gb = oracle.buffer_collector(), gpu_ctx.buffer_collector()
        for frac in (0.001, 0.01, 0.1, 0.5, 1.0):
            bmin = [float(lo[0]), float(lo[1]), float(lo[2])]
            bmax = [float(lo[0] + (hi[0] - lo[0]) * frac), float(hi[1]), float(hi[2])]
            lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
            one_o, one_g = oracle.buffer_collector(), gpu_ctx.buffer_collector()
            for o, g in ((one_o, one_g), (ob, gb)):
                assert oracle.search_last_bounds(image, bmin, bmax, o) == 0
                gpu_ctx.scan_dev(f.columns(True), pkg.Predicate.bounds(lmin, lmax), g)
            assert one_g.point_count() == one_o.point_count(), frac
            assert one_g.points().tobytes() == one_o.points().tobytes(), frac
            one_o.free(), one_g.free()
        for cls in (2, 6, 19):
            for o, g in ((ob, gb),):
                assert oracle.search_last_class(image, cls, o) == 0
                gpu_ctx.scan_dev(f.columns(True), pkg.Predicate.classification(cls), g)
        assert gb.point_count() == ob.point_count() > n
        assert gb.points().tobytes() == ob.points().tobytes()
        ob.free(), gb.free()
    finally:
        gpu_ctx.set_option("emit_sparse_max", 64)
        gpu_ctx.set_option("emit_park_max", 256)
        f.free()


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("n", [2048 * 5, 50_021])
def test_buffer_collector_skips_tiles_without_a_match(oracle, gpu_ctx, fmt, n):
    """A file whose points are sorted along x, cut by boxes in x: the emit does not read a 2048-point tile again in which the
    count pass found nothing — empty tiles in front, behind and between, tiles with one match, a box that matches nothing at
    all, and a second scan appended behind the first (record base not a multiple of 16).  Same image for the oracle."""
    spec = small_spec(777 + n + fmt, n, fmt=fmt)
    image = oracle.synth_image(spec, transposed=True).copy()
    hdr = oracle.parse_header(image[:400].tobytes())
    otp = hdr.offset_to_point_data
    pos = image[otp:otp + 12 * n].view(np.int32).reshape(n, 3)
    pos[:] = pos[np.argsort(pos[:, 0], kind="stable")]
    xs = pos[:, 0].astype(np.float64) * 0.01
    f = DevFile(gpu_ctx, image, hdr)
    try:
        boxes = [((xs[n // 3], -60.0, -20.0), (xs[n // 3 + 2500], 60.0, 20.0)),      # a run in the middle
                 ((xs[0], -60.0, -20.0), (xs[10], 60.0, 20.0)),                     # the first tile only
                 ((xs[n - 1], -60.0, -20.0), (60.0, 60.0, 20.0)),                   # the last point(s) only
                 ((xs[2048 * 2], -60.0, -20.0), (xs[2048 * 3 - 1], 60.0, 20.0)),    # one whole tile (ties at its ends permitting)
                 ((xs[5000], 49.999, 9.9999), (xs[5001], 50.0, 10.0)),              # nothing
                 ((-60.0, -0.5, -20.0), (60.0, 0.5, 20.0))]                         # a slab across x: a few matches in every tile
        ob, gb = oracle.buffer_collector(), gpu_ctx.buffer_collector()
        for bmin, bmax in boxes:
            one_o, one_g = oracle.buffer_collector(), gpu_ctx.buffer_collector()
            lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
            for o, g in ((one_o, one_g), (ob, gb)):
                assert oracle.search_last_bounds(image, bmin, bmax, o) == 0
                if oracle.aabb_intersects(list(hdr.min), list(hdr.max), bmin, bmax):  # (the column scan has no header early-out)
                    gpu_ctx.scan_dev(f.columns(True), pkg.Predicate.bounds(lmin, lmax), g)
            assert one_g.point_count() == one_o.point_count(), (bmin, bmax)
            assert one_g.points().tobytes() == one_o.points().tobytes()
            one_o.free()
            one_g.free()
        assert gb.point_count() == ob.point_count() > 0
        assert gb.points().tobytes() == ob.points().tobytes()
        ob.free()
        gb.free()
    finally:
        f.free()


@pytest.mark.parametrize("n,cell", [(1, 1.0), (5000, 2.5), (200_003, 0.7), (200_003, 10.0)])
def test_grid_collector_dev_matches_oracle(oracle, gpu_ctx, n, cell):
    spec = small_spec(31337 + n, n, fmt=2)
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    f = DevFile(gpu_ctx, image, hdr)
    try:
        for bmin, bmax in [((-20.0, -20.0, -5.0), (20.0, 20.0, 5.0)), ((-50.0, -50.0, -10.0), (50.0, 50.0, 10.0))]:
            og = oracle.grid_collector(bmin, bmax, cell)
            assert oracle.search_last_bounds(image, bmin, bmax, og) == 0
            lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
            gg = gpu_ctx.grid_collector(bmin, bmax, cell)
            assert gg.grid_params() == og.grid_params()
            gpu_ctx.scan_dev(f.columns(True), pkg.Predicate.bounds(lmin, lmax), gg)
            assert gg.point_count() == og.point_count()
            gp, gk = gg.points(), gg.grid_cells()
            order = np.argsort(gk, kind="stable")
            assert np.array_equal(gk[order], og.grid_cells())
            assert gp[order].tobytes() == og.points().tobytes()  # per cell: the same winner
            gg.free()
            og.free()
    finally:
        f.free()


@pytest.mark.parametrize("cell", [0.7, 2.5, 20.0])
def test_grid_collector_on_spatially_coherent_files(oracle, gpu_ctx, cell):
    """The seeded files are in random order: neighbouring lanes never share a cell.  Real tiles are written along
    scan lines; here the points are sorted along x/y strips, a third of them snapped to a lattice (exact duplicates:
    same-address atomics and distance ties inside a wave, first in file order wins), and a class query interleaves
    lanes that do not match."""
    n = 150_001
    spec = small_spec(777, n, fmt=2)
    image = oracle.synth_image(spec, transposed=True).copy()
    hdr = oracle.parse_header(image[:400].tobytes())
    otp = hdr.offset_to_point_data
    xyz = image[otp:otp + 12 * n].view("<i4").reshape(n, 3).copy()
    rng = np.random.default_rng(5)
    snap = rng.random(n) < 0.33
    xyz[snap] = xyz[snap] // 64 * 64
    strip = xyz[:, 1] // 300
    order = np.lexsort((np.where(strip % 2 == 0, xyz[:, 0], -xyz[:, 0]), strip))  # boustrophedon strips
    image[otp:otp + 12 * n] = np.frombuffer(np.ascontiguousarray(xyz[order]).tobytes(), dtype=np.uint8)
    f = DevFile(gpu_ctx, image, hdr)
    try:
        for bmin, bmax in [((-20.0, -20.0, -5.0), (20.0, 20.0, 5.0)), ((-50.0, -50.0, -10.0), (50.0, 50.0, 10.0))]:
            lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
            for pred, search in ((pkg.Predicate.bounds(lmin, lmax), lambda og: oracle.search_last_bounds(image, bmin, bmax, og)),
                                 (pkg.Predicate.classification(2), lambda og: oracle.search_last_class(image, 2, og))):
                og = oracle.grid_collector(bmin, bmax, cell)
                assert search(og) == 0
                gg = gpu_ctx.grid_collector(bmin, bmax, cell)
                gpu_ctx.scan_dev(f.columns(True), pred, gg)
                assert gg.point_count() == og.point_count()
                gp, gk = gg.points(), gg.grid_cells()
                order_k = np.argsort(gk, kind="stable")
                assert np.array_equal(gk[order_k], og.grid_cells())
                assert gp[order_k].tobytes() == og.points().tobytes()
                gg.free()
                og.free()
    finally:
        f.free()


@pytest.mark.parametrize("cell,bmin,bmax", [
    (2.5, (-20.0, -20.0, -5.0), (20.0, 20.0, 5.0)),      # 2.5 / 0.01: every 250th integer coordinate is a cell boundary
    (0.64, (-32.0, -32.0, -6.4), (32.0, 32.0, 6.4)),     # 0.64 / 0.01 = 64: the snapped third of the points sits on boundaries
    (1.0, (-10.0, -10.0, -2.0), (10.0, 10.0, 2.0)),      # a grid smaller than the data: the class query brings points below and beyond it
    (3.0, (5.0, 5.0, 1.0), (5.0, 40.0, 8.0)),            # a flat grid: zero extent along x (0 / 0 and x / 0 in the cell index)
])
def test_grid_cells_on_and_next_to_cell_boundaries(oracle, gpu_ctx, cell, bmin, bmax):
    """The kernels find a point's cell with one multiply and take the reference's division only within a few ulp of a
    cell boundary, outside the grid's range or for a degenerate grid: files whose coordinates sit ON the boundaries
    (and one integer step either side), below the grid's minimum (the reference saturates to cell 0) and beyond its
    maximum must give the reference's cells and winners."""
    n = 120_011
    spec = small_spec(4711, n, fmt=2)
    image = oracle.synth_image(spec, transposed=True).copy()
    hdr = oracle.parse_header(image[:400].tobytes())
    otp = hdr.offset_to_point_data
    xyz = image[otp:otp + 12 * n].view("<i4").reshape(n, 3).copy()
    rng = np.random.default_rng(99)
    step = max(1, int(round(cell / 0.01)))
    snap = rng.random(n) < 0.4
    xyz[snap] = xyz[snap] // step * step + rng.integers(-1, 2, size=(int(snap.sum()), 3))
    image[otp:otp + 12 * n] = np.frombuffer(np.ascontiguousarray(xyz).tobytes(), dtype=np.uint8)
    f = DevFile(gpu_ctx, image, hdr)
    try:
        lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
        for pred, search in ((pkg.Predicate.bounds(lmin, lmax), lambda og: oracle.search_last_bounds(image, bmin, bmax, og)),
                             (pkg.Predicate.classification(1), lambda og: oracle.search_last_class(image, 1, og))):
            og = oracle.grid_collector(bmin, bmax, cell)
            assert search(og) == 0
            gg = gpu_ctx.grid_collector(bmin, bmax, cell)
            gpu_ctx.scan_dev(f.columns(True), pred, gg)
            assert gg.point_count() == og.point_count()
            gp, gk = gg.points(), gg.grid_cells()
            order_k = np.argsort(gk, kind="stable")
            assert np.array_equal(gk[order_k], og.grid_cells())
            assert gp[order_k].tobytes() == og.points().tobytes()
            gg.free()
            og.free()
    finally:
        f.free()


def test_grid_fold_levels_refold_and_forced_fanout(oracle):
    """The grid collector partitions the matches by cell key and folds each partition in LDS (csrc/grid_*.hip): a coarse
    grid folds its 512 level-1 bins directly (one 6400-slot table per workgroup), a dense one gets a second partition
    level whose fan-out comes from a measured estimate, and a fan-out that turns out too small (forced here) makes
    partitions overflow their LDS table and the fold is repeated with more partitions.  Same cells and winners as the
    oracle in every case."""
    n = 3_000_000
    spec = small_spec(424242, n, fmt=2)
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    bmin, bmax = (-500.0, -500.0, -100.0), (500.0, 500.0, 100.0)  # wider than the data: the key space does not cap the bound
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
    expect = {}
    for cell in (1.0, 0.72, 0.25, 0.2):
        og = oracle.grid_collector(bmin, bmax, cell)
        assert oracle.search_last_bounds(image, bmin, bmax, og) == 0
        expect[cell] = (og.point_count(), og.grid_cells().copy(), og.points().tobytes())
        og.free()
    per_bin = {cell: expect[cell][0] / 512 for cell in expect}  # cells per level-1 bin
    assert per_bin[1.0] < per_bin[0.72] < 2000            # folded directly
    assert 5000 < per_bin[0.25] < 5350                    # over the estimate's limit for a direct fold (4700): second level
    assert 5480 < per_bin[0.2]                            # over what the big LDS table holds (5440 cells)
    with pkg.Context(0) as ctx:
        f = DevFile(ctx, image, hdr)
        try:
            def run(cell):
                before = [ctx.get_option(k) for k in ("grid_folds", "grid_level2", "grid_refolds")]
                gg = ctx.grid_collector(bmin, bmax, cell)
                ctx.scan_dev(f.columns(True), pkg.Predicate.bounds(lmin, lmax), gg)
                cnt, cells, pts = expect[cell]
                assert gg.point_count() == cnt
                gp, gk = gg.points(), gg.grid_cells()
                order = np.argsort(gk, kind="stable")
                assert np.array_equal(gk[order], cells)
                assert gp[order].tobytes() == pts
                gg.free()
                after = [ctx.get_option(k) for k in ("grid_folds", "grid_level2", "grid_refolds")]
                return tuple(a - b for a, b in zip(after, before)) + (ctx.get_option("grid_last_f2"),)

            assert run(1.0) == (1, 0, 0, 1)
            assert run(0.72) == (1, 0, 0, 1)
            assert run(0.25) == (1, 1, 0, 6)       # ~5270 cells per bin / 1000 per partition
            ctx.set_option("grid_f2", 1)           # forced direct fold: the bins overflow the table, the fold is repeated
            folds, level2, refolds, f2 = run(0.2)
            assert folds == 1 and level2 >= 1 and refolds >= 1 and f2 > 1
            ctx.set_option("grid_f2", 3)           # forced, too few partitions: 1840 cells each against 870 slots
            folds, level2, refolds, f2 = run(0.2)
            assert refolds >= 1 and f2 >= 6
            ctx.set_option("grid_f2", 13)          # a fan-out that is not a power of two, more partitions than needed
            assert run(0.25) == (1, 1, 0, 13) and run(1.0) == (1, 1, 0, 13)
            ctx.set_option("grid_f2", 0)
        finally:
            f.free()


def test_grid_second_level_regions_outgrown_by_hot_cells(oracle):
    """The second partition level writes each sub-partition into a fixed region (1.3 x the mean partition + 64 tuples)
    in one pass; a cell holding thousands of points makes its sub-partition outgrow the region, the kernel reports it and
    the host repeats the cut in the exact form (count, then scatter).  Same cells and winners as the oracle, and the
    counter shows which way it went."""
    n = 400_000
    spec = small_spec(9090, n, fmt=2)
    image = oracle.synth_image(spec, transposed=True).copy()
    hdr = oracle.parse_header(image[:400].tobytes())
    otp = hdr.offset_to_point_data
    xyz = image[otp:otp + 12 * n].view("<i4").reshape(n, 3).copy()
    rng = np.random.default_rng(1)
    hot = rng.random(n) < 0.1
    xyz[hot] = np.array([1234, -777, 55]) + rng.integers(0, 3, size=(int(hot.sum()), 3))  # 40 000 points in one or two cells
    image[otp:otp + 12 * n] = np.frombuffer(np.ascontiguousarray(xyz).tobytes(), dtype=np.uint8)
    bmin, bmax = (-60.0, -60.0, -12.0), (60.0, 60.0, 12.0)
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
    cell = 0.5
    og = oracle.grid_collector(bmin, bmax, cell)
    assert oracle.search_last_bounds(image, bmin, bmax, og) == 0
    with pkg.Context(0) as ctx:
        f = DevFile(ctx, image, hdr)
        try:
            # 2048 partitions of ~200 tuples: the hot cell does not fit · no second level at all · more sub-partitions per bin than
            # the one-pass form handles (1024): the counting form from the start
            for forced, outgrown in ((4, True), (0, False), (1500, False)):
                ctx.set_option("grid_f2", forced)
                before = ctx.get_option("grid_level2_exact")
                gg = ctx.grid_collector(bmin, bmax, cell)
                ctx.scan_dev(f.columns(True), pkg.Predicate.bounds(lmin, lmax), gg)
                assert gg.point_count() == og.point_count()
                gp, gk = gg.points(), gg.grid_cells()
                order = np.argsort(gk, kind="stable")
                assert np.array_equal(gk[order], og.grid_cells())
                assert gp[order].tobytes() == og.points().tobytes()
                gg.free()
                assert (ctx.get_option("grid_level2_exact") - before >= 1) == outgrown
            ctx.set_option("grid_f2", 0)
        finally:
            f.free()
    og.free()


@pytest.mark.parametrize("cell", [1.0, 0.72, 0.25])
def test_grid_shared_by_several_scans_with_guessed_tables(oracle, cell):
    """Sequential mode (main.rs:129-133): ONE grid folds several files, first seen wins across them — with the files
    folded together (one fold at the end) and with a fold after every file (point_count in between): the earlier
    winners are merged partition by partition, and at the densest cell size the second-level fan-out grows from fold
    to fold, so they are re-cut."""
    n = 1_400_000
    bmin, bmax = (-500.0, -500.0, -100.0), (500.0, 500.0, 100.0)
    images, hdrs = [], []
    for k in range(3):
        img = oracle.synth_image(small_spec(9000 + k, n, fmt=2), transposed=True)
        images.append(img)
        hdrs.append(oracle.parse_header(img[:400].tobytes()))
    og = oracle.grid_collector(bmin, bmax, cell)
    for img in images:
        assert oracle.search_last_bounds(img, bmin, bmax, og) == 0
    with pkg.Context(0) as ctx:
        gg = ctx.grid_collector(bmin, bmax, cell)
        files = []
        try:
            first = 0
            for img, hdr in zip(images, hdrs):
                f = DevFile(ctx, img, hdr)
                files.append(f)
                lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
                cols = f.columns(True)
                cols.first_index = first
                ctx.scan_dev(cols, pkg.Predicate.bounds(lmin, lmax), gg)
                first += n
            assert gg.point_count() == og.point_count()
            gp, gk = gg.points(), gg.grid_cells()
            order = np.argsort(gk, kind="stable")
            assert np.array_equal(gk[order], og.grid_cells())
            assert gp[order].tobytes() == og.points().tobytes()
            # the same with a fold behind every file
            g2 = ctx.grid_collector(bmin, bmax, cell)
            first, f2s, seen = 0, [], 0
            for f, hdr in zip(files, hdrs):
                lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
                cols = f.columns(True)
                cols.first_index = first
                ctx.scan_dev(cols, pkg.Predicate.bounds(lmin, lmax), g2)
                first += n
                now = g2.point_count()
                assert now >= seen
                seen = now
                f2s.append(ctx.get_option("grid_last_f2"))
            assert seen == og.point_count()
            gp, gk = g2.points(), g2.grid_cells()
            order = np.argsort(gk, kind="stable")
            assert np.array_equal(gk[order], og.grid_cells())
            assert gp[order].tobytes() == og.points().tobytes()
            if cell == 0.25:
                assert f2s[0] < f2s[-1]  # the earlier winners were re-cut for a larger fan-out
            g2.free()
        finally:
            gg.free()
            for f in files:
                f.free()
    og.free()


@pytest.mark.parametrize("cell", [1.0, 0.25])
def test_grid_through_the_host_path_in_large_chunks(oracle, cell):
    """pcq_scan_host of a 4 M-point file in staging chunks of 1.3 M points: every chunk is a scan of its own into the
    same grid (the CLI's path for files on disk) — all chunks folded together, and with a pending budget so small
    that every chunk is folded before the next one is scanned."""
    n = 4_000_003
    bmin, bmax = (-500.0, -500.0, -100.0), (500.0, 500.0, 100.0)
    image = oracle.synth_image(small_spec(31, n, fmt=2), transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    otp = hdr.offset_to_point_data
    og = oracle.grid_collector(bmin, bmax, cell)
    assert oracle.search_last_bounds(image, bmin, bmax, og) == 0
    with pkg.Context(0) as ctx:
        ctx.set_option("chunk_points", 1_300_000)
        gg = ctx.grid_collector(bmin, bmax, cell)
        try:
            base = image.ctypes.data + otp
            cols = binding.make_columns(xyz=base, cls=base + 15 * n, rgb=base + 20 * n, n=n, scale=list(hdr.scale),
                                        offset=list(hdr.offset))
            lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
            for budget in (0, 1_000_000):
                ctx.set_option("grid_pending_budget", budget)
                folds = ctx.get_option("grid_folds")
                ctx.scan_host(cols, pkg.Predicate.bounds(lmin, lmax), gg)
                assert gg.point_count() == og.point_count()
                # 19 staged bytes per point -> 5 chunks of ~0.82 M points: one fold in all, or one per chunk
                assert ctx.get_option("grid_folds") - folds == (5 if budget else 1)
                gp, gk = gg.points(), gg.grid_cells()
                order = np.argsort(gk, kind="stable")
                assert np.array_equal(gk[order], og.grid_cells())
                assert gp[order].tobytes() == og.points().tobytes()
                gg.reset()
        finally:
            gg.free()
    og.free()


def test_synth_device_generator_is_bit_identical(oracle, gpu_ctx):
    for spec in (small_spec(1, 100_003, zo=(3000, -9000, 18001)), specs.synth_ca13(50_001)[5], specs.synth_doc(40_000)[3],
                 specs.synth_navvis(30_011)[0]):
        n = spec.n
        xyz_h, cls_h = oracle.synth_columns(spec)
        dx, dc = gpu_ctx.alloc(12 * n), gpu_ctx.alloc(n)
        gpu_ctx.synth_fill(spec, 0, n, dx, dc)
        gx, gc = np.zeros((n, 3), dtype=np.int32), np.zeros(n, dtype=np.uint8)
        gpu_ctx.to_host(gx, dx)
        gpu_ctx.to_host(gc, dc)
        gpu_ctx.free(dx)
        gpu_ctx.free(dc)
        assert np.array_equal(gx, xyz_h)
        assert np.array_equal(gc, cls_h)


def test_allreduce_single_rank_through_the_real_rccl_calls(gpu_ctx):
    """With option "allreduce_single_rank" a ONE-rank all-reduce still binds RCCL at run time (dlopen, the six symbols),
    builds a communicator of one device — here through pcq_allreduce_prepare, as the CLI does from a thread of its own — and runs
    ncclAllReduce(sum, ncclUint64 = 5, count 1) on the context's stream, out of place (word 0 -> word 1): the whole call
    path of the multi-GPU merge (main.rs:164-180), minus a second GPU.  Two entries on one device are refused (one rank
    per GPU).  The injected failures (option "allreduce_fail") leave the value that was sent untouched — what the CLI's
    host-side fallback sums."""
    d = gpu_ctx.alloc(16)
    gpu_ctx.to_device(d, np.array([98765432109876543, 7], dtype=np.uint64))
    ctxs = (C.c_void_p * 2)(gpu_ctx.handle.value, gpu_ctx.handle.value)
    send = (C.c_void_p * 2)(d, d)
    recv = (C.c_void_p * 2)(d + 8, d + 8)
    gpu_ctx.set_option("allreduce_single_rank", 1)
    try:
        devs = (C.c_int * 1)(0)  # the fixture's context is on device 0
        assert gpu_ctx.lib.pcq_allreduce_prepare(devs, 1) == 0
        for _ in range(3):  # the communicator is built once (by the prepare) and reused
            assert gpu_ctx.lib.pcq_allreduce_sum_u64(ctxs, send, recv, 1) == 0, gpu_ctx.lib.pcq_last_error()
        out = np.zeros(2, dtype=np.uint64)
        gpu_ctx.to_host(out, d)
        assert [int(v) for v in out] == [98765432109876543, 98765432109876543]
        assert gpu_ctx.lib.pcq_allreduce_sum_u64(ctxs, send, send, 1) == 0  # in place is allowed
        assert gpu_ctx.lib.pcq_allreduce_sum_u64(ctxs, send, recv, 2) == -8  # PCQ_ERR_ARG: both on device 0
        assert b"one rank per GPU" in gpu_ctx.lib.pcq_last_error()
        for mode, where in ((1, b"before"), (2, b"after"), (3, b"inside the group")):
            gpu_ctx.to_device(d + 8, np.array([0], dtype=np.uint64))
            gpu_ctx.set_option("allreduce_fail", mode)
            assert gpu_ctx.lib.pcq_allreduce_sum_u64(ctxs, send, recv, 1) != 0
            assert b"injected failure" in gpu_ctx.lib.pcq_last_error() and where in gpu_ctx.lib.pcq_last_error()
            gpu_ctx.set_option("allreduce_fail", 0)
            gpu_ctx.to_host(out, d)  # (reads on the context's stream: a collective left half-enqueued there would hang this)
            assert int(out[0]) == 98765432109876543                      # what was sent is what the fallback reads
            if mode != 3:  # (a failure inside the group aborts the communicator: the reduction may or may not have run)
                assert int(out[1]) == (0 if mode == 1 else 98765432109876543)  # the late failure comes after the reduction ran
            # the next collective is not swallowed — after mode 3 on a communicator built anew (the aborted one is gone)
            gpu_ctx.to_device(d + 8, np.array([0], dtype=np.uint64))
            assert gpu_ctx.lib.pcq_allreduce_sum_u64(ctxs, send, recv, 1) == 0, gpu_ctx.lib.pcq_last_error()
            gpu_ctx.to_host(out, d)
            assert [int(v) for v in out] == [98765432109876543, 98765432109876543]
    finally:
        gpu_ctx.set_option("allreduce_fail", 0)
        gpu_ctx.set_option("allreduce_single_rank", 0)
        gpu_ctx.free(d)


def test_prepare_leaves_no_thread_behind():
    """pcq_allreduce_prepare builds the communicator synchronously; the library starts no thread.  (Round 3 first had a helper
    thread in there: a process that ended while it was still inside RCCL died of std::terminate on the joinable thread, then of
    SIGSEGV in the runtime's exit handlers, then hung in them.)  A process that prepares and ends without an all-reduce —
    after a device list RCCL refuses, and after one it accepts — ends with status 0."""
    import os
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import importlib, ctypes as C, sys, threading\n"
            "sys.path.insert(0, %r)\n"
            "pkg = importlib.import_module('adhoc-queries-pointclouds_amd')\n"
            "ctx = pkg.Context(0)\n"
            "n0 = threading.active_count()\n"
            "assert ctx.lib.pcq_allreduce_prepare((C.c_int * 2)(0, 0), 2) != 0\n"    # a repeated device: refused, reported at once
            "assert ctx.lib.pcq_allreduce_sum_u64(None, None, None, 0) != 0\n"
            "assert ctx.lib.pcq_allreduce_prepare((C.c_int * 1)(0), 1) == 0\n"       # ready when this returns
            "print('done', flush=True)\n") % ROOT
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "done" in r.stdout, (r.returncode, r.stderr[-2000:])


def test_allreduce_entry_point_single_rank(gpu_ctx):
    """pcq_allreduce_sum_u64 with one rank copies the value (the n > 1 RCCL path needs several GPUs)."""
    d = gpu_ctx.alloc(16)
    gpu_ctx.to_device(d, np.array([12345678901234567, 0], dtype=np.uint64))
    ctxs = (C.c_void_p * 1)(gpu_ctx.handle.value)
    send = (C.c_void_p * 1)(d)
    recv = (C.c_void_p * 1)(d + 8)
    assert gpu_ctx.lib.pcq_allreduce_sum_u64(ctxs, send, recv, 1) == 0
    out = np.zeros(2, dtype=np.uint64)
    gpu_ctx.to_host(out, d)
    gpu_ctx.free(d)
    assert [int(v) for v in out] == [12345678901234567, 12345678901234567]


def test_class_count_batch_matches_sum_of_files(oracle, gpu_ctx):
    files, cols, preds, expect = [], [], [], 0
    try:
        for i, (n, pad) in enumerate([(100_003, 0), (0, 3), (15, 7), (4096 + 17, 1), (70_001, 13), (1_000_003, 5), (6143, 2), (6144 + 16, 9),
                                      (12_288 + 31, 4)]):
            spec = small_spec(700 + i, n, fmt=1)
            image = oracle.synth_image(spec, transposed=True)
            hdr = oracle.parse_header(image[:400].tobytes())
            f = DevFile(gpu_ctx, image, hdr, pad=pad)
            files.append(f)
            cls = 6 if i % 2 == 0 else 2
            oc = oracle.count_collector()
            assert oracle.search_last_class(image, cls, oc) == 0
            expect += oc.point_count()
            oc.free()
            cols.append(f.columns(True))
            preds.append(pkg.Predicate.classification(cls))
        total = gpu_ctx.alloc(16)
        gpu_ctx.memset(total, 0, 16)
        gpu_ctx.scan_dev_count_batch(cols, preds, total)
        gpu_ctx.scan_dev_count_batch(cols, preds, total)
        host = np.zeros(1, dtype=np.uint64)
        gpu_ctx.to_host(host, total)
        assert int(host[0]) == 2 * expect
        # mixing kinds in one batch is rejected
        with pytest.raises(pkg.PcqError):
            gpu_ctx.scan_dev_count_batch(cols[:2], [preds[0], pkg.Predicate.bounds([0, 0, 0], [1, 1, 1])], total)
        gpu_ctx.free(total)
    finally:
        for f in files:
            f.free()


def test_accessor_waits_for_scans_enqueued_on_a_caller_stream(oracle, gpu_ctx):
    import torch
    ts = torch.cuda.Stream()
    spec = small_spec(77, 3_000_017)
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    f = DevFile(gpu_ctx, image, hdr)
    try:
        bmin, bmax = BOXES[0]
        oc = oracle.count_collector()
        oracle.search_last_bounds(image, bmin, bmax, oc)
        ob = oracle.buffer_collector()
        oracle.search_last_bounds(image, bmin, bmax, ob)
        lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
        pred = pkg.Predicate.bounds(lmin, lmax)
        for _ in range(5):
            cc = gpu_ctx.count_collector()
            for _ in range(4):
                gpu_ctx.scan_dev(f.columns(False), pred, cc, ts.cuda_stream)
            assert cc.point_count() == 4 * oc.point_count()  # no explicit synchronisation by the caller
            cc.free()
        gb = gpu_ctx.buffer_collector()
        gpu_ctx.scan_dev(f.columns(True), pred, gb, ts.cuda_stream)
        assert gb.points().tobytes() == ob.points().tobytes()
        gb.free()
    finally:
        f.free()


def test_scan_host_nowait_lets_the_caller_reuse_its_buffer(oracle, gpu_ctx):
    """pcq_scan_host_nowait returns once the caller's columns have been copied out: the SAME host buffer is
    overwritten with the next block right away; counts and the ordered result buffer must still be exact."""
    gpu_ctx.set_option("chunk_points", 4096)  # several staging chunks per call, so both staging pairs stay busy across calls
    try:
        blocks = []
        for i, n in enumerate([10_000, 3, 70_001, 4096, 8192 + 5, 1, 50_000]):
            spec = small_spec(900 + i, n, fmt=1)  # no colour column
            image = oracle.synth_image(spec, transposed=True)
            hdr = oracle.parse_header(image[:400].tobytes())
            blocks.append((image, hdr))
        bmin, bmax = BOXES[0]
        nmax = max(h.number_of_points for _, h in blocks)
        xyz = np.zeros(nmax * 12, dtype=np.uint8)
        cls = np.zeros(nmax, dtype=np.uint8)
        cc, bc = gpu_ctx.count_collector(), gpu_ctx.buffer_collector()
        expect_pts, first = [], 0
        for image, hdr in blocks:
            n, otp = hdr.number_of_points, hdr.offset_to_point_data
            lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
            pred = pkg.Predicate.bounds(lmin, lmax)
            for coll in (cc, bc):
                xyz[:12 * n] = image[otp:otp + 12 * n]  # overwrite the shared buffer: the previous call has let go of it
                cls[:n] = image[otp + 15 * n: otp + 16 * n]
                cols = binding.make_columns(xyz=xyz.ctypes.data, cls=cls.ctypes.data, n=n, first_index=first,
                                            scale=list(hdr.scale), offset=list(hdr.offset))
                gpu_ctx.scan_host_nowait(cols, pred, coll)
                xyz[:12 * n] = 0xEE  # scribble at once
            first += n
            ob = oracle.buffer_collector()
            assert oracle.search_last_bounds(image, bmin, bmax, ob) == 0
            assert oracle.aabb_intersects(list(hdr.min), list(hdr.max), bmin, bmax)  # (the column scan has no header early-out)
            expect_pts.append(ob.points())
            ob.free()
        want = np.concatenate(expect_pts)
        assert cc.point_count() == len(want) > 0
        assert bc.points().tobytes() == want.tobytes()
        cc.free(), bc.free()
    finally:
        gpu_ctx.set_option("chunk_points", 1 << 20)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_host_scans_read_the_staging_ring_in_place_or_through_its_device_twin(oracle, mode):
    """host_in_place: the kernels of a count or grid scan read the pinned staging ring over PCIe (1), a device copy of it (0), or
    the one while a thread of the library sets the process's copy path up and the other from then on (2, the default) — and the
    buffer collector always the copy.  Several chunks per call, several calls per context (mode 2 changes over between them)."""
    spec = small_spec(4242, 90_001, fmt=1)
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    n, otp = hdr.number_of_points, hdr.offset_to_point_data
    bmin, bmax = BOXES[0]
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
    xyz = np.ascontiguousarray(image[otp:otp + 12 * n])
    cls = np.ascontiguousarray(image[otp + 15 * n: otp + 16 * n])
    cols = binding.make_columns(xyz=xyz.ctypes.data, cls=cls.ctypes.data, n=n, scale=list(hdr.scale), offset=list(hdr.offset))
    oc, ob, og = oracle.count_collector(), oracle.buffer_collector(), oracle.grid_collector(bmin, bmax, 1.5)
    for c in (oc, ob, og):
        assert oracle.search_last_bounds(image, bmin, bmax, c) == 0
    with pkg.Context(0) as ctx:
        ctx.set_option("host_in_place", mode)
        ctx.set_option("chunk_points", 8192)
        pred = pkg.Predicate.bounds(lmin, lmax)
        for rep in range(3):
            cc, bc, gc = ctx.count_collector(), ctx.buffer_collector(), ctx.grid_collector(bmin, bmax, 1.5)
            ctx.scan_host(cols, pred, cc)
            ctx.scan_host(cols, pred, gc)
            ctx.scan_host(cols, pred, bc)
            assert cc.point_count() == oc.point_count() > 0
            assert bc.points().tobytes() == ob.points().tobytes()
            assert gc.point_count() == og.point_count()
            gp, gk = gc.points(), gc.grid_cells()
            order = np.argsort(gk, kind="stable")
            assert np.array_equal(gk[order], og.grid_cells())
            assert gp[order].tobytes() == og.points().tobytes()  # per cell: the same winner
            cc.free(), bc.free(), gc.free()
    oc.free(), ob.free(), og.free()


def test_prepare_host_scans_runs_beside_the_caller_and_changes_nothing(oracle):
    """pcq_prepare_host_scans pins the staging ring on a thread of the library: a scan issued at once waits for it, a scan
    with larger chunks than it prepared replaces the ring, a context shut down before any scan joins it; results are the
    oracle's either way."""
    spec = small_spec(77, 60_000, fmt=1)
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    n, otp = hdr.number_of_points, hdr.offset_to_point_data
    bmin, bmax = BOXES[0]
    oc = oracle.count_collector()
    assert oracle.search_last_bounds(image, bmin, bmax, oc) == 0
    want = oc.point_count()
    oc.free()
    assert want > 0
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(hdr.scale), list(hdr.offset))
    xyz = np.ascontiguousarray(image[otp:otp + 12 * n])
    cols = binding.make_columns(xyz=xyz.ctypes.data, n=n, scale=list(hdr.scale), offset=list(hdr.offset))
    for chunk_points in (None, 4096, 8 << 20):
        with pkg.Context(0) as ctx:
            ctx.prepare_host_scans()
            ctx.prepare_host_scans()  # (a second call while the first is under way is a no-op)
            if chunk_points:
                ctx.set_option("chunk_points", chunk_points)
            cc = ctx.count_collector()
            ctx.scan_host(cols, pkg.Predicate.bounds(lmin, lmax), cc)
            assert cc.point_count() == want
            cc.free()
    # The prepare thread reads numa_local, copy_threads and chunk_points, and allocates what numa_local frees: each of
    # them set right behind it waits for the thread.  60 000 points in chunks of 4096: 15 chunks, both pairs, pairs reused.
    ob = oracle.buffer_collector()
    assert oracle.search_last_bounds(image, bmin, bmax, ob) == 0
    rcols = binding.make_columns(xyz=image.ctypes.data + otp, cls=image.ctypes.data + otp + 15 * n, n=n,
                                 scale=list(hdr.scale), offset=list(hdr.offset))
    with pkg.Context(0) as ctx:
        numa_local = ctx.get_option("numa_local")
        ctx.prepare_host_scans()
        ctx.set_option("numa_local", 0)
        ctx.set_option("copy_threads", 3)
        ctx.set_option("chunk_points", 4096)
        cc, gb = ctx.count_collector(), ctx.buffer_collector()
        ctx.scan_host(cols, pkg.Predicate.bounds(lmin, lmax), cc)
        ctx.scan_host(rcols, pkg.Predicate.bounds(lmin, lmax), gb)
        assert cc.point_count() == want == gb.point_count()
        assert gb.points().tobytes() == ob.points().tobytes()
        cc.free()
        gb.free()
        ctx.set_option("numa_local", numa_local)
    ob.free()
    with pkg.Context(0) as ctx:
        ctx.prepare_host_scans()  # and nothing else: shutdown joins the thread


@pytest.mark.parametrize("n", [3_000, 400_003])
def test_grid_massive_aliasing_is_replayed_exactly(oracle, gpu_ctx, n):
    """A grid box much smaller than the data it is fed: almost every matched point lands in a cell >= 2^bits, whose key
    aliases onto another cell's while the distance is taken to its OWN centre (grid_sampling.rs:62-82) — the fold's
    result then depends on the visiting order, and every aliased key is replayed in file order.  The short list goes
    through the quadratic rank kernel, the long one (n = 400 003: ~10^5 aliased tuples) through the radix sort."""
    spec = small_spec(4711 + n, n, fmt=2)
    image = oracle.synth_image(spec, transposed=True)
    hdr = oracle.parse_header(image[:400].tobytes())
    f = DevFile(gpu_ctx, image, hdr)
    try:
        pbox = ((-60.0, -60.0, -12.0), (60.0, 60.0, 12.0))          # the predicate: (nearly) everything
        for gmin, gmax, cell in [((-3.0, -3.0, -1.0), (5.0, 5.0, 1.0), 1.0),     # dims 8 x 8 x 2: powers of two, masks alias
                                 ((0.0, 0.0, 0.0), (3.0, 2.5, 0.7), 0.4)]:        # dims 8 x 7 x 2
            og = oracle.grid_collector(gmin, gmax, cell)
            assert oracle.search_last_bounds(image, pbox[0], pbox[1], og) == 0
            lmin, lmax = pkg.box_to_local(pbox[0], pbox[1], list(hdr.scale), list(hdr.offset))
            for pieces in (1, 3):  # one scan, and three scans into the same collector with a fold in between
                gg = gpu_ctx.grid_collector(gmin, gmax, cell)
                assert gg.grid_params() == og.grid_params()
                step = (n + pieces - 1) // pieces
                for k in range(pieces):
                    first, count = k * step, min(step, n - k * step)
                    cols = f.columns(True)
                    cols.xyz += 12 * first
                    cols.cls += first
                    cols.rgb += 6 * first
                    cols.n, cols.first_index = count, first
                    gpu_ctx.scan_dev(cols, pkg.Predicate.bounds(lmin, lmax), gg)
                    if pieces > 1:
                        gg.point_count()
                assert gg.point_count() == og.point_count()
                gp, gk = gg.points(), gg.grid_cells()
                order = np.argsort(gk, kind="stable")
                assert np.array_equal(gk[order], og.grid_cells())
                assert gp[order].tobytes() == og.points().tobytes()
                gg.free()
            og.free()
    finally:
        f.free()
