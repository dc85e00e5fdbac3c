"""k_p0_part (csrc/grid_pass0.hip) beyond the first trip of its tile loop, against the oracle's SparseGrid: same point count, same
sorted cell keys, every byte of every winner record.  The corpora and what each reaches are _grid_trips.py's (proven without a GPU
in test_grid_trips_plan.py):

  a. at the device's own geometry — (2 CUs + 37) tiles and 1234 points in scan order: 37 workgroups make a third trip (the prefetch
     has gone round twice, the match counters are back at the first), the 38th meets the short tile on it.  BOUNDS on packed LAST
     blocks of format 1 (16-byte tuples) and 2 (colours, 24-byte tuples), CLASS on format 1 (positions loaded for the matches only),
     BOUNDS on LAS records; a coarse and a dense grid; the tile fold adaptive, always and never.
  b. deep trips under a workgroup cap (the option grid_p0_blocks) — 80 tiles built so that the tuples that leave pass 0 follow
     from the back-off's state machine: 1, 2 and 7 workgroups, every back-off value, resets by a cluster and by an empty tile,
     both sides of the `total * 4 > matched * 3` rule, table tiles behind table tiles and behind tiles without one.
  c. every predicate kind and layout on three workgroups, 13 to 14 trips each.
"""
import contextlib
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _grid_trips as gt  # noqa: E402
import _time_images as ti  # noqa: E402
from _grid_trips import check_same  # noqa: E402
from test_gpu_scan import DevFile  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")


@contextlib.contextmanager
def options(ctx, **kw):
    saved = {k: ctx.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


@pytest.fixture(scope="module")
def ctx():
    with pkg.Context(0) as c:
        yield c


class Dev:
    """Device copies of host arrays (256-byte aligned), freed together."""

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


def is_packed(cols, time):
    """grid_host.hip: LAST blocks at aligned addresses take the kernel's PACKED form"""
    return (cols.xyz_stride == 12 and cols.xyz % 4 == 0 and (not cols.rgb or cols.rgb_stride == 6)
            and ((cols.cls_stride == 8 and cols.cls % 8 == 0) if time else (not cols.cls or cols.cls_stride == 1)))


def las_columns(ptr, fmt, n, scale, offset, time=False, colour=True):
    rl, toff, coff, kof = ti.FORMATS[fmt]
    return binding.make_columns(xyz=ptr, cls=ptr + (toff if time else kof), rgb=ptr + coff if coff is not None and colour and not time else None, n=n,
                                xyz_stride=rl, cls_stride=rl, rgb_stride=rl, scale=list(scale), offset=list(offset))


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the device's own geometry
# ---------------------------------------------------------------------------------------------------------------------------------
COARSE = (20.0, (-60.0, -60.0, -12.0), (60.0, 60.0, 12.0))
DENSE = (0.3, (-50.0, -50.0, -10.0), (50.0, 50.0, 10.0))
TRIP_CASES = ("last1 bounds", "last2 bounds", "last1 class", "las1 bounds")


class TripFiles:
    """The scan-ordered files of formats 1 and 2 and the first one's points as LAS records, on the device; the oracle's grids and the
    match counts, each computed once."""

    def __init__(self, ctx, oracle):
        self.ctx, self.oracle = ctx, oracle
        self.cus = ctx.device_info()["compute_units"]
        self.n = n = gt.trips_points(self.cus)
        self.dev = Dev(ctx)
        self.images, self.cols, self.hdr = {}, {}, None
        self.files = []
        for fmt in (1, 2):
            image, hdr = gt.scan_ordered_image(oracle, 20300 + fmt, n, fmt)
            f = DevFile(ctx, image, hdr, pad=1)   # (the header is 227 bytes: the positions 4-byte aligned)
            self.files.append(f)
            self.images["last%d" % fmt], self.cols["last%d" % fmt] = image, f.columns(True)
            self.hdr = self.hdr or hdr
        xyz, cls = gt.last_columns(self.images["last1"], self.hdr)
        self.scale, self.offset = list(self.hdr.scale), list(self.hdr.offset)
        las = ti.las_image(1, xyz, cls, None, np.zeros(n), scale=tuple(self.scale), offset=tuple(self.offset))
        self.images["las1"] = las
        self.cols["las1"] = las_columns(self.dev.put(las[227:]), 1, n, self.scale, self.offset)
        assert is_packed(self.cols["last1"], False) and is_packed(self.cols["last2"], False) and not is_packed(self.cols["las1"], False)
        self._grids, self._matched = {}, {}

    def pred(self, case, box):
        if case.endswith("class"):
            return pkg.Predicate.classification(2)
        lmin, lmax = pkg.box_to_local(box[0], box[1], self.scale, self.offset)
        return pkg.Predicate.bounds(lmin, lmax)

    def grid(self, case, which):
        """The oracle's grid of the case (kept: nine tests read each)"""
        if (case, which) not in self._grids:
            cell, bmin, bmax = which
            layout, kind = case.split()
            o, og = self.oracle, self.oracle.grid_collector(bmin, bmax, cell)
            image = self.images[layout]
            if kind == "class":
                assert o.search_last_class(image, 2, og) == 0
            elif layout.startswith("last"):
                assert o.search_last_bounds(image, bmin, bmax, og) == 0
            else:
                assert o.search_las_bounds(image, bmin, bmax, og)[0] == 0
            self._grids[case, which] = og
        return self._grids[case, which]

    def matched(self, case, which):
        if (case, which) not in self._matched:
            cc = self.ctx.count_collector()
            self.ctx.scan_dev(self.cols[case.split()[0]], self.pred(case, which[1:]), cc)
            self._matched[case, which] = cc.point_count()
            cc.free()
        return self._matched[case, which]

    def free(self):
        for og in self._grids.values():
            og.free()
        for f in self.files:
            f.free()
        self.dev.free()


@pytest.fixture(scope="module")
def trip_files(ctx, oracle):
    t = TripFiles(ctx, oracle)
    yield t
    t.free()


@pytest.mark.parametrize("agg", [0, 1, 2])
@pytest.mark.parametrize("case", TRIP_CASES)
def test_pass0_third_trip_at_one_workgroup_per_cu(ctx, trip_files, case, agg):
    tf = trip_files
    tiles = gt.ntiles(tf.n)
    assert tiles == 2 * tf.cus + gt.EXTRA + 1 and gt.workgroups(tiles, tf.cus) == tf.cus and ctx.get_option("grid_p0_blocks") == 0
    with options(ctx, grid_agg=agg):
        for which in (COARSE, DENSE):
            cell, bmin, bmax = which
            gg = ctx.grid_collector(bmin, bmax, cell)
            try:
                ctx.scan_dev(tf.cols[case.split()[0]], tf.pred(case, (bmin, bmax)), gg)
                check_same(gg, tf.grid(case, which))
                tuples, matched = ctx.get_option("grid_last_tuples"), tf.matched(case, which)
                print(case, "agg", agg, "cell", cell, "tuples", tuples, "matched", matched)
                assert ctx.get_option("grid_last_tuple_bytes") == (24 if case.startswith("last2") else 16)
                assert matched > tf.n // 5
                if agg == 2:
                    assert tuples == matched     # every match travels
                elif which is COARSE:
                    assert tuples < matched // 4, (tuples, matched)   # hundreds of consecutive points per cell: the tile fold sheds them
            finally:
                gg.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# b. deep trips and the back-off, exactly
# ---------------------------------------------------------------------------------------------------------------------------------
class DeepFile:
    def __init__(self, ctx, oracle):
        self.c = c = gt.deep_corpus()
        image = c.image()
        self.hdr = oracle.parse_header(image[:400].tobytes())
        self.f = DevFile(ctx, image, self.hdr, pad=1)
        self.cols = self.f.columns(True)
        assert is_packed(self.cols, False)
        self.og = oracle.grid_collector(gt.DEEP_BMIN, gt.DEEP_BMAX, gt.DEEP_CELL)
        assert oracle.search_last_bounds(image, gt.DEEP_BMIN, gt.DEEP_BMAX, self.og) == 0
        assert self.og.point_count() == c.cells
        lmin, lmax = pkg.box_to_local(gt.DEEP_BMIN, gt.DEEP_BMAX, list(gt.DEEP_SCALE), list(gt.DEEP_OFFSET))
        self.pred = pkg.Predicate.bounds(lmin, lmax)

    def free(self):
        self.og.free()
        self.f.free()


@pytest.fixture(scope="module")
def deep_file(ctx, oracle):
    d = DeepFile(ctx, oracle)
    yield d
    d.free()


@pytest.mark.parametrize("agg", [0, 1, 2])
@pytest.mark.parametrize("w", [1, 2, 7])
def test_pass0_back_off_state_under_a_workgroup_cap(ctx, deep_file, w, agg):
    """The tuples that leave pass 0 are the model's sum, per workgroup over its tiles w, w + W, ...: 1, 3840 or 3841 where the tile
    folded, its matches where it did not."""
    d = deep_file
    with options(ctx, grid_agg=agg, grid_p0_blocks=w):
        gg = ctx.grid_collector(gt.DEEP_BMIN, gt.DEEP_BMAX, gt.DEEP_CELL)
        try:
            ctx.scan_dev(d.cols, d.pred, gg)
            check_same(gg, d.og)
            tuples, want = ctx.get_option("grid_last_tuples"), d.c.expected_tuples(w, agg)
            print("workgroups", w, "agg", agg, "tuples", tuples, "model", want,
                  {m: d.c.expected_tuples(w, agg, m) for m in ("no_reset", "skip_from_attempt", "empty_fails")})
            assert tuples == want
            assert ctx.get_option("grid_last_tuple_bytes") == 16
        finally:
            gg.free()
    assert ctx.get_option("grid_p0_blocks") == 0


def test_the_workgroup_cap_never_raises_the_count(ctx, deep_file):
    """A cap above one workgroup per CU is the default launch: the same tuples leave as with the option at 0"""
    d = deep_file
    cus = ctx.device_info()["compute_units"]
    seen = []
    for cap in (0, cus, cus + 1, 65536):
        with options(ctx, grid_p0_blocks=cap):
            gg = ctx.grid_collector(gt.DEEP_BMIN, gt.DEEP_BMAX, gt.DEEP_CELL)
            try:
                ctx.scan_dev(d.cols, d.pred, gg)
                check_same(gg, d.og)
                seen.append(ctx.get_option("grid_last_tuples"))
            finally:
                gg.free()
    assert seen == [d.c.expected_tuples(min(cus, gt.DEEP_TILES), 0)] * 4


# ---------------------------------------------------------------------------------------------------------------------------------
# c. every predicate kind and layout, past the second trip
# ---------------------------------------------------------------------------------------------------------------------------------
# (positions are 100 + 0.01 k, -200 + 0.01 k, 7.5 + 0.01 k: the faces lie between two of them, and the box holds the offset, so that the
# truncation of last.rs:98-109 rounds the lower corner up and the upper one down — the integer box and the world box select the same points)
KBOX = ((62.345, -237.135, -1.123), (141.777, -161.615, 14.321))
KCLASS = 2
KTIME = (1200.0, 1700.0)
KCELLS = (2.5, 0.4)
KINDS = ("bounds", "class", "bounds_class", "bounds_f64", "time", "bounds_time")
KLAYOUTS = {False: ("last1", "last3", "las1", "las3"), True: ("last1", "las1", "las3")}   # by "tests the time"


class KindsFiles:
    def __init__(self, ctx):
        self.c = c = gt.kinds_corpus()
        self.dev = dev = Dev(ctx)
        n, so = c.n, dict(scale=list(c.scale), offset=list(c.offset))
        xyz, cls, rgb, t = dev.put(c.xyz), dev.put(c.cls), dev.put(c.rgb), dev.put(c.t)
        self.cols = {("last1", False): binding.make_columns(xyz=xyz, cls=cls, n=n, **so),
                     ("last3", False): binding.make_columns(xyz=xyz, cls=cls, rgb=rgb, n=n, **so),
                     ("last1", True): binding.make_columns(xyz=xyz, cls=t, cls_stride=8, n=n, **so)}
        for fmt in (1, 3):
            rec = dev.put(ti.records(fmt, c.xyz, c.cls, c.rgb, c.t))
            for time in (False, True):
                self.cols["las%d" % fmt, time] = las_columns(rec, fmt, n, c.scale, c.offset, time=time)
        for (layout, time), cols in self.cols.items():
            assert is_packed(cols, time) == layout.startswith("last"), (layout, time)
        assert self.cols["las3", False].rgb and not self.cols["las3", True].rgb


@pytest.fixture(scope="module")
def kinds_files(ctx):
    k = KindsFiles(ctx)
    yield k
    k.dev.free()


def kind_cases():
    return [(kind, layout) for kind in KINDS for layout in KLAYOUTS[kind.endswith("time")]]


@pytest.mark.parametrize("kind,layout", kind_cases())
def test_pass0_every_kind_and_layout_past_the_second_trip(ctx, oracle, kinds_files, kind, layout):
    """Three workgroups over 41 tiles: each instantiation KIND x RGB x PACKED x WIDE of k_p0_part that the layouts reach makes 13 or
    14 trips.  CLASS and TIME match beyond the grid's box: aliased keys go through the tile's table as they are."""
    k, c = kinds_files, kinds_files.c
    time = kind.endswith("time")
    cols = k.cols[layout, time]
    lay, fmt = layout[:-1], int(layout[-1])
    image = c.image(lay, fmt)
    lmin, lmax = pkg.box_to_local(KBOX[0], KBOX[1], list(c.scale), list(c.offset))
    pred = {"bounds": lambda: pkg.Predicate.bounds(lmin, lmax), "class": lambda: pkg.Predicate.classification(KCLASS),
            "bounds_class": lambda: pkg.Predicate.bounds_class(lmin, lmax, KCLASS), "bounds_f64": lambda: pkg.Predicate.bounds_f64(*KBOX),
            "time": lambda: pkg.Predicate.time_range(*KTIME), "bounds_time": lambda: pkg.Predicate.bounds_time(lmin, lmax, *KTIME)}[kind]()

    def search(og):
        if kind in ("bounds", "bounds_f64"):
            return oracle.search_last_bounds(image, *KBOX, og) if lay == "last" else oracle.search_las_bounds(image, *KBOX, og)[0]
        if kind == "class":
            return (oracle.search_last_class if lay == "last" else oracle.search_las_class)(image, KCLASS, og)
        if kind == "bounds_class":
            return oracle.search_bounds_class(image, lay, *KBOX, KCLASS, og)
        if kind == "time":
            return oracle.search_time(image, lay, *KTIME, og)
        return oracle.search_bounds_time(image, lay, *KBOX, *KTIME, og)

    if kind == "bounds_f64":  # the oracle's answer to the world box is its answer to the integer box
        w = ti.world(c.xyz, c.scale, c.offset)
        assert np.array_equal(np.all((c.xyz >= lmin) & (c.xyz <= lmax), axis=1), np.all((w >= KBOX[0]) & (w <= KBOX[1]), axis=1))
    wide = kind == "bounds_f64" or (layout.endswith("3") and not time)
    for cell in KCELLS:
        og = oracle.grid_collector(*KBOX, cell)
        try:
            assert search(og) == 0
            assert og.point_count() > 100
            for agg in (0, 1, 2):
                with options(ctx, grid_agg=agg, grid_p0_blocks=3):
                    gg = ctx.grid_collector(*KBOX, cell)
                    try:
                        ctx.scan_dev(cols, pred, gg)
                        check_same(gg, og)
                        assert ctx.get_option("grid_last_tuple_bytes") == (24 if wide else 16)
                    finally:
                        gg.free()
        finally:
            og.free()
