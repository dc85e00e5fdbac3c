"""The grid fold's recovery routes that no counter was read for (csrc/grid_host.hip, grid_fold.hip, grid_fold_stream.hip,
grid_level2.hip): the streaming fold's defer list (`grid_deferred`: some bins of a fold finished by k_fold_stream, the others
handed to k_fold<BIG>, both writing one winner array), k_fold_dense's defer list (`grid_dense_deferred`: partitions left to
k_fold<SMALL>) and the block padding option (`grid_block_pad`).

The trigger is TIES.  k_fold_stream keeps a tuple when `dbits <= seen` (grid_fold_stream.hip:322): K points at one stored
position — no other tuple of their cell closer to its centre — are K survivors of their bin, whatever order the waves run
in, and the oracle (grid_sampling.rs:62-82: strict `<`) keeps the first of them in file order: the `(order + 1) << 32`
tie-break of both kernels.  The tied points carry different class and colour bytes, so a wrong winner shows in the record.

Every case compares cells and winner records with the oracle (check_same) AND reads the counter deltas around its own fold:
the one that proves the route ran, and the zeros that prove its neighbour's did not.  The thresholds below are read off the
code, not measured.  Each construction is first checked against the oracle alone (one cell and winner = point 0; the hot
cells' winners are the first hot points; the second file does / does not take the cell; the aliased case depends on the file
order), so that no case passes vacuously."""
import contextlib
import importlib
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
from test_gpu_scan import DevFile, small_spec  # noqa: E402
from test_gpu_grid_tiles import TILE, check_same, scan_ordered_image  # noqa: E402

# ---- the thresholds, with their source lines (csrc/) ----------------------------------------------------------------
F1 = 512                    # grid_common.h:72 — level-1 bins
BIG_LIMIT = 5440            # grid_common.h:88 — cells the big LDS table holds: more in one bin -> the fold is repeated
DENSE_CHUNK = 512 * 3       # grid_common.h:92 DENSE_NT * DENSE_K; k_fold_dense defers `cnt > CHUNK` (grid_fold.hip:468)
L2_STAGED_F2 = 1024         # grid_common.h:97 — above it the second level is k_level2_direct from the start (grid_host.hip:399)


def surv_cap(m):
    """grid_host.hip:458 — the survivor list of one workgroup, m = the fold's pending tuples (`grid_last_tuples`); a bin defers
    when `nsurv > surv_cap` (grid_fold_stream.hip:379)."""
    return min(65536, max(4096, 2 * (m // F1)))


def staged_region(m, nparts):
    """grid_host.hip:398 — tuples a sub-partition's region of the staged second level has room for."""
    return math.ceil(m / nparts * 1.3) + 64


def bin_of_keys(keys, wide):
    """grid_common.h:291-299 — the level-1 bin of a cell key: the top nine bits of cell_hash()'s upper word."""
    k = np.asarray(keys, dtype=np.uint64)
    m32 = np.uint64(0xffffffff)
    k32 = k & m32
    if wide:
        k32 = k32 ^ (((k >> np.uint64(32)) * np.uint64(0x27d4eb2f)) & m32)
    hi = (k32 * np.uint64(0x9e3779b9)) & m32
    hi = hi ^ (hi >> np.uint64(15))
    return (hi >> np.uint64(23)).astype(np.int64)


COUNTERS = ("grid_folds", "grid_deferred", "grid_dense_deferred", "grid_refolds", "grid_level2", "grid_level2_exact", "grid_compactions")
BOX = ((-60.0, -60.0, -12.0), (60.0, 60.0, 12.0))    # holds every point of a small_spec file at its default scale
SCALE2, OFFSET2 = (0.02, 0.01, 0.005), (1.0, -2.0, 0.5)  # the second file of a fold with several entries


def counters(ctx):
    return {k: ctx.get_option(k) for k in COUNTERS}


def since(ctx, before):
    return {k: ctx.get_option(k) - before[k] for k in COUNTERS}


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


class Cols:
    """The columns of a LAST image that the scans and the oracle read, as arrays to edit; store() writes them back."""

    def __init__(self, oracle, image):
        self.image = image
        self.hdr = hdr = oracle.parse_header(image[:400].tobytes())
        self.n = n = hdr.number_of_points
        otp, fmt = hdr.offset_to_point_data, hdr.point_data_record_format
        self.at = {"xyz": (otp, 12), "cls": (otp + 15 * n, 1)}
        if fmt == 2:
            self.at["rgb"] = (otp + 20 * n, 6)
        self.xyz = self._get("xyz").view("<i4").reshape(n, 3).copy()
        self.cls = self._get("cls").copy()
        self.rgb = self._get("rgb").view("<u2").reshape(n, 3).copy() if fmt == 2 else None

    def _get(self, name):
        lo, width = self.at[name]
        return self.image[lo:lo + width * self.n]

    def store(self):
        for name in self.at:
            self._get(name)[:] = np.frombuffer(np.ascontiguousarray(getattr(self, name)).tobytes(), dtype=np.uint8)
        return self

    def stamp(self, idx, tag, cls=None):
        """Point idx[r] gets class 1 + r % 251 (or `cls`) and colour (r & 0xffff, r >> 16, tag): who won shows in the record."""
        r = np.arange(len(idx))
        self.cls[idx] = 1 + r % 251 if cls is None else cls
        if self.rgb is not None:
            self.rgb[idx] = np.stack([r & 0xffff, r >> 16, np.full(len(idx), tag)], axis=1)

    def world(self, ixyz):
        """A stored position as the record holds it (last.rs:156-160: two roundings per axis)."""
        return tuple(float(ixyz[a]) * self.hdr.scale[a] + self.hdr.offset[a] for a in range(3))

    def is_point(self, rec, i):
        """The record carries point i's position, class and colour."""
        same = (rec["x"], rec["y"], rec["z"]) == self.world(self.xyz[i]) and rec["classification"] == self.cls[i]
        if self.rgb is not None:
            same = same and (rec["r"], rec["g"], rec["b"]) == tuple(self.rgb[i])
        return bool(same)


def new_cols(oracle, seed, n, fmt, **kw):
    return Cols(oracle, oracle.synth_image(small_spec(seed, n, fmt=fmt, **kw), transposed=True).copy())


def records_at(pts, world):
    return np.flatnonzero((pts["x"] == world[0]) & (pts["y"] == world[1]) & (pts["z"] == world[2]))


def scan(ctx, gg, f, first=0, box=BOX, cls=None):
    cols = f.columns(True)
    cols.first_index = first
    if cls is None:
        lmin, lmax = pkg.box_to_local(box[0], box[1], list(f.hdr.scale), list(f.hdr.offset))
        ctx.scan_dev(cols, pkg.Predicate.bounds(lmin, lmax), gg)
    else:
        ctx.scan_dev(cols, pkg.Predicate.classification(cls), gg)


def matched(oracle, cols, box=BOX, cls=None):
    oc = oracle.count_collector()
    assert (oracle.search_last_bounds(cols.image, box[0], box[1], oc) if cls is None else oracle.search_last_class(cols.image, cls, oc)) == 0
    n = oc.point_count()
    oc.free()
    return n


_REFS = {}


def cached(key, make):
    """References are computed once and shared by the cases that need them; nobody writes to them."""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------
# (a), (f): a file of K points at one stored position
# ---------------------------------------------------------------------------------------------------------------
TIE_AT = (1234, -777, 55)
COARSE, DENSE = 5.0, 0.5


def ties_ref(oracle, K, fmt, cell):
    def make():
        cols = new_cols(oracle, 7100 + fmt, K, fmt)
        cols.xyz[:] = TIE_AT
        cols.stamp(np.arange(K), 9)
        cols.store()
        og = oracle.grid_collector(BOX[0], BOX[1], cell)
        assert oracle.search_last_bounds(cols.image, BOX[0], BOX[1], og) == 0
        # the construction: one cell; the first of the K in file order holds it, and its neighbour's record would differ
        assert og.point_count() == 1
        assert cols.is_point(og.points()[0], 0) and not cols.is_point(og.points()[0], 1)
        return cols, og
    return cached(("ties", K, fmt, cell), make)


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("K", [4095, 4096, 4097, 3 * 4096 + 1])
def test_stream_deferral_boundary(oracle, ctx, K, fmt):
    """K tied tuples in one bin of a coarse grid are K survivors: the bin is finished by k_fold_stream up to K = surv_cap =
    4096 and handed to k_fold<BIG> from 4097 on (one tile, and three), 16-byte tuples <false, false> and 24-byte ones
    <true, true>; one cell either way, held by point 0.

    With the tile fold on (grid_agg = 1) the same K tuples travel and the same bins defer: pass 0 drops a tuple only when
    its truncated distance differs from the tile's minimum for its key (grid_pass0.hip:221 — "only lets near-ties survive
    together", :83-87), so exact ties are never shed.  (Read off that rule, not off "one tuple per tile and cell", which
    holds for points at different distances only.)"""
    cols, og = ties_ref(oracle, K, fmt, COARSE)
    assert surv_cap(K) == 4096
    f = DevFile(ctx, cols.image, cols.hdr)
    try:
        for agg in (2, 1):
            with options(ctx, grid_agg=agg, grid_stream=1, grid_f2=0):
                gg = ctx.grid_collector(BOX[0], BOX[1], COARSE)
                try:
                    before = counters(ctx)
                    scan(ctx, gg, f)
                    gg.flush()
                    d = since(ctx, before)
                    print("K", K, "fmt", fmt, "agg", agg, "tuples", ctx.get_option("grid_last_tuples"), d)
                    assert ctx.get_option("grid_last_tuples") == K, agg
                    assert ctx.get_option("grid_last_tuple_bytes") == (16 if fmt == 1 else 24)
                    assert d == dict.fromkeys(COUNTERS, 0) | {"grid_folds": 1, "grid_deferred": int(K > surv_cap(K))}, agg
                    assert ctx.get_option("grid_last_f2") == 1
                    assert gg.point_count() == 1
                    check_same(gg, og)
                finally:
                    gg.free()
    finally:
        f.free()


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("f2", [4, 1500])
@pytest.mark.parametrize("K", [DENSE_CHUNK, DENSE_CHUNK + 1])
def test_dense_deferral_boundary(oracle, ctx, K, f2, fmt):
    """K tied tuples in one partition of the second level: k_fold_dense folds a partition of up to 1536 tuples and leaves one
    of 1537 to k_fold<SMALL> (two chunks there); point 0 holds the cell.  f2 = 4: the staged second level, whose region of
    ceil(K / 2048 * 1.3) + 64 = 65 tuples the partition outgrows — the cut is repeated in the counting form, and only the
    attempt that is kept counts its deferrals; f2 = 1500 (above 1024): k_level2_direct from the start."""
    cols, og = ties_ref(oracle, K, fmt, DENSE)
    assert staged_region(K, F1 * 4) < K and 4 <= L2_STAGED_F2 < 1500
    f = DevFile(ctx, cols.image, cols.hdr)
    try:
        with options(ctx, grid_agg=2, grid_f2=f2):
            gg = ctx.grid_collector(BOX[0], BOX[1], DENSE)
            try:
                before = counters(ctx)
                scan(ctx, gg, f)
                gg.flush()
                d = since(ctx, before)
                print("K", K, "f2", f2, "fmt", fmt, "tuples", ctx.get_option("grid_last_tuples"), d)
                assert ctx.get_option("grid_last_tuples") == K
                assert d["grid_dense_deferred"] == int(K > DENSE_CHUNK)
                assert (d["grid_level2_exact"] >= 1) == (f2 == 4) and d["grid_level2"] == 1
                assert d["grid_folds"] == 1 and d["grid_deferred"] == 0 and d["grid_refolds"] == 0
                assert ctx.get_option("grid_last_f2") == f2
                assert gg.point_count() == 1
                check_same(gg, og)
            finally:
                gg.free()
    finally:
        f.free()


# ---------------------------------------------------------------------------------------------------------------
# (b), (c): hot cells among a background
# ---------------------------------------------------------------------------------------------------------------
MIXED_CELL = 4.0           # 25 x 25 x 5 cells over the data: ~6 cells per bin, centres at -58 + 4 i (x, y) and -10 + 4 k (z)
HOT1 = (1403, -600, 200)   # 3 units beside the centre (14, -6, 2) of its cell
HOT1_CLOSER, HOT1_FARTHER = (1401, -600, 200), (1407, -600, 200)  # the same cell: 1 and 7 units beside the centre
HOT2 = (-2999, 2201, -200)  # next to the centre (-30, 22, -2)
HOT2_FILE2 = (-1549, 2401, -500)  # the same cell in the second file's units: (-29.98, 22.01, -2)
NHOT = 6000


def hot_file(oracle, seed, n_bg, hots, fmt, **kw):
    """n_bg seeded points and, scattered among them at random places (fixed seed), `count` copies of each hot position."""
    n = n_bg + sum(count for _, count, _ in hots)
    cols = new_cols(oracle, seed, n, fmt, **kw)
    perm = np.random.default_rng(seed).permutation(n)
    cols.hot, at = [], 0
    for pos, count, tag in hots:
        idx = np.sort(perm[at:at + count])
        at += count
        cols.xyz[idx] = pos
        cols.stamp(idx, tag)
        cols.hot.append(idx)
    return cols.store()


def hot_winner(cols, k, cells, pts):
    """The oracle's record at hot position k is the FIRST of its copies (and the only record there); its cell key."""
    at = records_at(pts, cols.world(cols.xyz[cols.hot[k][0]]))
    assert len(at) == 1 and cols.is_point(pts[at[0]], cols.hot[k][0]) and not cols.is_point(pts[at[0]], cols.hot[k][1])
    return int(cells[at[0]])


def mixed_ref(oracle, fmt, two_files):
    def make():
        if two_files:
            files = [hot_file(oracle, 7200 + fmt, 30_001, [(HOT1, NHOT, 1)], fmt),
                     hot_file(oracle, 7210 + fmt, 30_000, [(HOT2_FILE2, NHOT, 2)], fmt, scale=SCALE2, offset=OFFSET2)]
            hots = [(files[0], 0), (files[1], 0)]
        else:
            files = [hot_file(oracle, 7220 + fmt, 60_001, [(HOT1, NHOT, 1), (HOT2, NHOT, 2)], fmt)]
            hots = [(files[0], 0), (files[0], 1)]
        og = oracle.grid_collector(BOX[0], BOX[1], MIXED_CELL)
        for c in files:
            assert oracle.search_last_bounds(c.image, BOX[0], BOX[1], og) == 0
        cells, pts = og.grid_cells(), og.points()
        wide = sum(og.grid_params()[1]) > 32
        assert len(np.unique(bin_of_keys(cells, wide))) > 2 and len(cells) > 1000   # a fold of many bins, two of them hot
        hot_bins = {int(bin_of_keys([hot_winner(c, k, cells, pts)], wide)[0]) for c, k in hots}
        return files, og, sum(matched(oracle, c) for c in files), len(hot_bins)
    return cached(("mixed", fmt, two_files), make)


@pytest.mark.parametrize("two_files", [False, True])
@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("tuple16", [1, 0])
def test_mixed_fold_some_bins_deferred_the_others_streamed(oracle, ctx, tuple16, fmt, two_files):
    """One fold, both kernels, one winner array: the bins of the two hot cells (6000 ties each, above surv_cap = 4096; one
    bin if both cells hash to it) go through `P.wcount[p] = 0`, the defer list and k_fold<BIG>; the hundreds of other bins
    (~140 tuples each) are finished by k_fold_stream.  16- and 24-byte tuples, one entry and two (files of different scale
    and offset in one fold: the tile -> entry table, the <true, true> kernels)."""
    files, og, m, hot_bins = mixed_ref(oracle, fmt, two_files)
    assert surv_cap(m) == 4096 < NHOT and m // F1 < 4096 and 1 <= hot_bins <= 2
    devs = []
    gg = None
    try:
        with options(ctx, grid_agg=2, grid_tuple16=tuple16, grid_stream=1, grid_f2=0):
            gg = ctx.grid_collector(BOX[0], BOX[1], MIXED_CELL)
            before = counters(ctx)
            first = 0
            for c in files:
                devs.append(DevFile(ctx, c.image, c.hdr))
                scan(ctx, gg, devs[-1], first)
                first += c.n
            gg.flush()
            d = since(ctx, before)
            print("tuple16", tuple16, "fmt", fmt, "two files", two_files, "tuples", ctx.get_option("grid_last_tuples"), "hot bins", hot_bins, d)
            assert ctx.get_option("grid_last_tuples") == m      # grid_agg = 2: every match travels
            assert 1 <= d["grid_deferred"] <= 2 and d["grid_deferred"] == hot_bins
            assert d == dict.fromkeys(COUNTERS, 0) | {"grid_folds": 1, "grid_deferred": hot_bins}
            assert ctx.get_option("grid_last_f2") == 1
            check_same(gg, og)
    finally:
        if gg:
            gg.free()
        for f in devs:
            f.free()


def onto_winners_ref(oracle, fmt, second):
    def make():
        files, _, m_a, hot_bins = mixed_ref(oracle, fmt, False)
        a = files[0]
        if second == "same":
            b = a
        else:
            b = hot_file(oracle, 7300 + fmt, 20_000, [(HOT1_CLOSER if second == "closer" else HOT1_FARTHER, 4097, 3)], fmt)
        og = oracle.grid_collector(BOX[0], BOX[1], MIXED_CELL)
        assert oracle.search_last_bounds(a.image, BOX[0], BOX[1], og) == 0
        count_a, cells_a, pts_a = og.point_count(), og.grid_cells(), og.points()
        key = hot_winner(a, 0, cells_a, pts_a)
        assert oracle.search_last_bounds(b.image, BOX[0], BOX[1], og) == 0
        cells, pts = og.grid_cells(), og.points()
        rec = pts[np.flatnonzero(cells == key)[0]]
        if second == "same":      # every point ties with the winner of its cell or loses: nothing changes
            assert np.array_equal(cells, cells_a) and pts.tobytes() == pts_a.tobytes()
        elif second == "closer":  # the cell goes to the first of B's copies
            assert hot_winner(b, 0, cells, pts) == key and b.is_point(rec, b.hot[0][0]) and not a.is_point(rec, a.hot[0][0])
        else:                     # A's winner stays
            assert a.is_point(rec, a.hot[0][0]) and len(records_at(pts, b.world(HOT1_FARTHER))) == 0
        return a, b, og, count_a, m_a, hot_bins
    return cached(("onto", fmt, second), make)


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("second", ["same", "closer", "farther"])
def test_deferral_onto_earlier_winners(oracle, ctx, second, fmt):
    """A second fold meets the first one's winners (`okeys`; grid_f2 = 1 throughout, so the stream kernel reads the bins both
    times).  The same file again: the 6000 copies tie with the old winner of their cell — survivors —, the bin defers and
    k_fold<BIG> keeps the old winner (order 0).  A file whose 4097 copies are strictly closer to the centre of hot cell 1:
    the first lowers the minimum, all tie with it, the bin defers and the cell goes to B's first copy.  4097 copies farther
    away: each is above the old winner's distance when it is tested, none survives, nothing defers, the old winner stays."""
    a, b, og, count_a, m_a, hot_bins = onto_winners_ref(oracle, fmt, second)
    m_b = m_a if second == "same" else matched(oracle, b)
    assert surv_cap(m_a) == surv_cap(m_b) == 4096
    want = {"same": hot_bins, "closer": 1, "farther": 0}[second]
    fa = DevFile(ctx, a.image, a.hdr)
    fb = fa if b is a else DevFile(ctx, b.image, b.hdr)
    gg = None
    try:
        with options(ctx, grid_agg=2, grid_stream=1, grid_f2=1):
            gg = ctx.grid_collector(BOX[0], BOX[1], MIXED_CELL)
            before = counters(ctx)
            scan(ctx, gg, fa)
            gg.flush()
            d1 = since(ctx, before)
            assert ctx.get_option("grid_last_tuples") == m_a
            assert d1 == dict.fromkeys(COUNTERS, 0) | {"grid_folds": 1, "grid_deferred": hot_bins}
            assert gg.point_count() == count_a
            before = counters(ctx)
            scan(ctx, gg, fb, first=a.n)
            gg.flush()
            d2 = since(ctx, before)
            print("second", second, "fmt", fmt, "tuples", ctx.get_option("grid_last_tuples"), "hot bins", hot_bins, d1, d2)
            assert ctx.get_option("grid_last_tuples") == m_b
            assert d2 == dict.fromkeys(COUNTERS, 0) | {"grid_folds": 1, "grid_deferred": want}
            assert ctx.get_option("grid_last_f2") == 1
            assert gg.point_count() == og.point_count()
            check_same(gg, og)
    finally:
        if gg:
            gg.free()
        fa.free()
        if fb is not fa:
            fb.free()


# ---------------------------------------------------------------------------------------------------------------
# (d): aliased keys in a deferred bin
# ---------------------------------------------------------------------------------------------------------------
ALIAS_GRID = ((-3.0, -3.0, -1.0), (5.0, 5.0, 1.0), 1.0)   # 8 x 8 x 2 cells, far smaller than the data
CLUSTER_AT = (1050, 150, 50)   # the centre of cell (13, 4, 1): beyond the grid in x, masked onto (5, 4, 1) = key 5 | 4 << 3 | 1 << 6
IN_BOX_AT = (260, 130, 40)     # a point of cell (5, 4, 1) itself
ALIASED_KEY = 5 | 4 << 3 | 1 << 6


def aliased_ref(oracle):
    def make():
        cols = hot_file(oracle, 7400, 30_000, [(CLUSTER_AT, 5000, 4), (IN_BOX_AT, 3, 5)], 2)
        for idx in cols.hot:
            cols.cls[idx] = 2     # the class query takes them
        cols.store()
        g0, g1, cell = ALIAS_GRID

        def fold(c):
            og = oracle.grid_collector(g0, g1, cell)
            assert oracle.search_last_class(c.image, 2, og) == 0
            return og

        og = fold(cols)
        assert og.grid_params() == ([8, 8, 2], [3, 3, 1]) and ALIASED_KEY in og.grid_cells()
        # the same points with the cluster moved behind all others: another result — the key's winner depends on the file order
        cluster = np.zeros(cols.n, dtype=bool)
        cluster[cols.hot[0]] = True
        order = np.concatenate([np.flatnonzero(~cluster), np.flatnonzero(cluster)])
        moved = Cols(oracle, cols.image.copy())
        moved.xyz, moved.cls, moved.rgb = cols.xyz[order], cols.cls[order], cols.rgb[order]
        moved.store()
        om = fold(moved)
        assert np.array_equal(om.grid_cells(), og.grid_cells())
        i = np.flatnonzero(og.grid_cells() == ALIASED_KEY)[0]
        assert om.points()[i].tobytes() != og.points()[i].tobytes()
        om.free()
        return cols, og, matched(oracle, cols, cls=2)
    return cached("aliased", make)


def test_aliased_keys_in_a_deferred_bin(oracle, ctx):
    """The geometry of test_grid_massive_aliasing_is_replayed_exactly with a class query: nearly every match lies beyond the
    8 x 8 x 2 grid and aliases onto one of its 128 keys.  5000 copies of a point at the centre of cell (13, 4, 1) — distance
    0 to their OWN centre, so every one of them survives — alias onto the occupied cell (5, 4, 1): its bin defers, k_fold<BIG>
    flags the key, and the replay decides it from all its tuples in file order."""
    cols, og, m = aliased_ref(oracle)
    assert surv_cap(m) == 4096 < 5000
    g0, g1, cell = ALIAS_GRID
    f = DevFile(ctx, cols.image, cols.hdr)
    gg = None
    try:
        with options(ctx, grid_agg=2, grid_stream=1, grid_f2=0):
            gg = ctx.grid_collector(g0, g1, cell)
            assert gg.grid_params() == og.grid_params()
            before = counters(ctx)
            scan(ctx, gg, f, cls=2)
            gg.flush()
            d = since(ctx, before)
            print("tuples", ctx.get_option("grid_last_tuples"), d)
            assert ctx.get_option("grid_last_tuples") == m
            assert d["grid_deferred"] >= 1 and d["grid_folds"] == 1 and d["grid_refolds"] == 0 and d["grid_level2"] == 0
            check_same(gg, og)
    finally:
        if gg:
            gg.free()
        f.free()


# ---------------------------------------------------------------------------------------------------------------
# (e): overflow and deferral in one fold
# ---------------------------------------------------------------------------------------------------------------
FINE = 0.2                     # 600 x 600 x 120 cells of 20 units: 10 + 10 + 7 key bits
FINE_HOT = (1231, -770, 50)    # one unit beside the centre of its cell


def overfull_bin_ref(oracle):
    def make():
        # cells (cx, cy, cz) -> keys as grid_sampling.rs:62-70 packs them, -> bins; one bin's first 6000 cells get a point each
        bits = [10, 10, 7]
        cx, cy, cz = np.meshgrid(np.arange(100, 300), np.arange(100, 300), np.arange(20, 100), indexing="ij")
        cx, cy, cz = cx.ravel(), cy.ravel(), cz.ravel()
        keys = (cx | cy << bits[0] | cz << (bits[0] + bits[1])).astype(np.uint64)
        bins = bin_of_keys(keys, False)
        full = int(bins[0])
        pick = np.flatnonzero(bins == full)[:6000]
        assert len(pick) == 6000 > BIG_LIMIT
        n_bg = 20_000
        n = n_bg + len(pick) + NHOT
        cols = new_cols(oracle, 7500, n, 2)
        perm = np.random.default_rng(7500).permutation(n)
        one_each, hot = np.sort(perm[:len(pick)]), np.sort(perm[len(pick):len(pick) + NHOT])
        cols.xyz[one_each] = np.stack([-6000 + 20 * cx[pick] + 10, -6000 + 20 * cy[pick] + 10, -1200 + 20 * cz[pick] + 10], axis=1)  # cell centres
        cols.xyz[hot] = FINE_HOT
        cols.stamp(hot, 6)
        cols.hot = [hot]
        cols.store()
        og = oracle.grid_collector(BOX[0], BOX[1], FINE)
        assert oracle.search_last_bounds(cols.image, BOX[0], BOX[1], og) == 0
        cells, pts = og.grid_cells(), og.points()
        # the construction, on the oracle's own keys: the chosen cells are there, their bin holds more cells than the big table,
        # no other bin comes near it, and the hot cell's winner is the first of its copies
        assert og.grid_params()[1] == bits and np.isin(keys[pick], cells).all()
        per_bin = np.bincount(bin_of_keys(cells, False), minlength=F1)
        assert per_bin[full] > BIG_LIMIT and np.sort(per_bin)[-2] < 200
        hot_bin = int(bin_of_keys([hot_winner(cols, 0, cells, pts)], False)[0])
        return cols, og, full, hot_bin
    return cached("overfull", make)


def test_refold_of_an_overfull_bin_meets_a_partition_left_by_the_dense_fold(oracle, ctx):
    """Overflow and deferral in one fold, forced direct (grid_f2 = 1).  6000 cells chosen to hash into ONE level-1 bin (more
    than the big table's 5440: k_fold_stream reports the bin, the host repeats the fold) among 20 000 background points, and
    one cell of 6000 ties in another bin (above surv_cap = 4096: deferred to k_fold<BIG> in that first, discarded attempt).
    The repeat cuts every bin into f2 = (5440 * 3 / 2 + 999) / 1000 = 9 partitions — staged, regions of 74 tuples, outgrown by
    the chosen cells' partitions (~670 tuples) and by the hot one: repeated in the counting form — and k_fold_dense leaves
    exactly the hot partition (6000 > 1536 tuples) to k_fold<SMALL>.

    (The uniformly dense file this route is usually reached with — 3 M points at 0.2 m, test_grid_fold_levels_refold_and_
    forced_fanout — costs the oracle 2.2 s for the fold and 3.8 s for each sorted read of its 2.8 M cells; an overfull bin
    made of chosen cells reaches the same route with 32 000 points.)"""
    cols, og, full, hot_bin = overfull_bin_ref(oracle)
    assert surv_cap(cols.n) == 4096 < NHOT and staged_region(cols.n, F1 * 9) < 600
    f = DevFile(ctx, cols.image, cols.hdr)
    gg = None
    try:
        with options(ctx, grid_agg=2, grid_stream=1, grid_f2=1):
            gg = ctx.grid_collector(BOX[0], BOX[1], FINE)
            before = counters(ctx)
            scan(ctx, gg, f)
            gg.flush()
            d = since(ctx, before)
            print("tuples", ctx.get_option("grid_last_tuples"), "f2", ctx.get_option("grid_last_f2"), "bins", full, hot_bin, d)
            assert ctx.get_option("grid_last_tuples") == cols.n
            assert d["grid_refolds"] >= 1 and d["grid_dense_deferred"] >= 1 and ctx.get_option("grid_last_f2") > 1
            assert d == {"grid_folds": 1, "grid_deferred": int(hot_bin != full), "grid_dense_deferred": 1, "grid_refolds": 1, "grid_level2": 1,
                         "grid_level2_exact": 1, "grid_compactions": 0}
            assert ctx.get_option("grid_last_f2") == 9
            check_same(gg, og)
    finally:
        if gg:
            gg.free()
        f.free()


# ---------------------------------------------------------------------------------------------------------------
# (g): block padding
# ---------------------------------------------------------------------------------------------------------------
PAD_SHAPES = {"coarse stream": (20.0, {"grid_stream": 1, "grid_f2": 0}, 1),
              "coarse k_fold": (20.0, {"grid_stream": 0, "grid_f2": 0}, 1),
              "dense f2=7": (0.3, {"grid_stream": 1, "grid_f2": 7}, 7)}


def padded_ref(oracle, cell):
    def make():
        image, hdr = scan_ordered_image(oracle, 7600, 12 * TILE + 1234, 1)
        og = oracle.grid_collector(BOX[0], BOX[1], cell)
        assert oracle.search_last_bounds(image, BOX[0], BOX[1], og) == 0
        assert og.point_count() > 50
        return image, hdr, og
    return cached(("padded", cell), make)


@pytest.mark.parametrize("shape", list(PAD_SHAPES))
@pytest.mark.parametrize("tuple16", [1, 0])
@pytest.mark.parametrize("pad", [0, 1, 3, 64, 4097, 65536])
def test_block_padding_changes_nothing(oracle, ctx, pad, tuple16, shape):
    """grid_block_pad moves every tile block but the first: 16 x pad bytes between the blocks — 24-byte tuples at a 16-byte
    phase when pad is odd, blocks a megabyte apart at 65536.  The scan-ordered file (ties inside and across its 13 tiles)
    gives the oracle's cells and winners through the streaming fold, k_fold<BIG> and the second level, in both tuple sizes."""
    cell, opts, f2 = PAD_SHAPES[shape]
    image, hdr, og = padded_ref(oracle, cell)
    f = DevFile(ctx, image, hdr)
    gg = None
    try:
        with options(ctx, grid_block_pad=pad, grid_tuple16=tuple16, **opts):
            gg = ctx.grid_collector(BOX[0], BOX[1], cell)
            before = counters(ctx)
            scan(ctx, gg, f)
            gg.flush()
            d = since(ctx, before)
            assert ctx.get_option("grid_last_tuple_bytes") == (16 if tuple16 else 24)
            assert d["grid_folds"] == 1 and d["grid_level2"] == int(f2 > 1) and d["grid_refolds"] == 0
            assert ctx.get_option("grid_last_f2") == f2
            check_same(gg, og)
    finally:
        if gg:
            gg.free()
        f.free()
    assert ctx.get_option("grid_block_pad") == 0
