"""The grid collector's fold with more than 4096 pending tiles, against the oracle's SparseGrid: same point count, same sorted cell
keys, every byte of every winner record.  T, the number of 5120-point tiles, is that of the points SCANNED: 4198 here (_grid_trips.py,
proven in test_grid_trips_plan.py) — k_bin_prefix walks a second chunk of 4096 counts with its carry, the window readers refill nine
times (the last window holds 102 fragments), the streaming fold takes 66 batches, and pass 0 makes 16 to 17 trips per workgroup.

21.5 M random points are written on the device by the synthesiser and copied back once; the matches of a thin box (1 %: fragments of
less than two tuples, the bins are copied together first unless the streaming fold reads them) and of a thick one (23 %: above the
2 T F1 tuples from which the readers take the fragments as they lie) are selected with numpy.  A grid's result depends on the
sequence of matching points alone, so the oracle folds an image of the matches only, in file order.

Every case is also run over the first 4096 tiles alone (one chunk of k_bin_prefix, eight full windows), against the oracle's fold of
the matches among those: a lost carry fails the long scan only, a bad body both.
"""
import contextlib
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _grid_trips as gt  # noqa: E402
from _grid_trips import check_same  # noqa: E402
from test_gpu_scan import small_spec  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

N, N1 = gt.MANY_POINTS, gt.ONE_CHUNK_POINTS
T = gt.ntiles(N)
THIN = ((-10.0, -12.5, -2.0), (10.0, 12.5, 2.0))      # 0.2 x 0.25 x 0.2 of the volume
THICK = ((-30.0, -30.0, -6.5), (30.0, 30.0, 6.5))     # 0.6 x 0.6 x 0.65
SCALE, OFFSET = [0.01, 0.01, 0.01], [0.0, 0.0, 0.0]


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


class Corpus:
    def __init__(self, ctx, oracle):
        self.ctx, self.oracle = ctx, oracle
        seed = 4198 + int(os.environ.get("PCQ_TEST_SEED_BASE", "0"))
        spec = small_spec(seed, N, fmt=1)
        self.d_xyz, self.d_cls = ctx.alloc(12 * N + 64), ctx.alloc(N + 64)
        ctx.synth_fill(spec, 0, N, self.d_xyz, self.d_cls)
        self.xyz, self.cls = np.zeros((N, 3), dtype=np.int32), np.zeros(N, dtype=np.uint8)
        ctx.to_host(self.xyz, self.d_xyz)
        ctx.to_host(self.cls, self.d_cls)
        self._sel, self._grids = {}, {}

    def columns(self, first=0, n=N):
        return binding.make_columns(xyz=self.d_xyz + 12 * first, cls=self.d_cls + first, n=n, first_index=first, scale=SCALE, offset=OFFSET)

    def pred(self, box):
        lmin, lmax = pkg.box_to_local(box[0], box[1], SCALE, OFFSET)
        return pkg.Predicate.bounds(lmin, lmax)

    def matches(self, box):
        """Indices of the points inside the box's integer form, in file order"""
        if box not in self._sel:
            lmin, lmax = pkg.box_to_local(box[0], box[1], SCALE, OFFSET)
            sel = np.ones(N, dtype=bool)
            for a in range(3):
                sel &= (self.xyz[:, a] >= lmin[a]) & (self.xyz[:, a] <= lmax[a])
            self._sel[box] = np.flatnonzero(sel)
        return self._sel[box]

    def grid(self, box, cell, n):
        """The oracle's grid of the box's matches among the first n points: a format-1 LAST image of the synthesiser with the
        matches' positions and class bytes written over its columns"""
        if (box, cell, n) not in self._grids:
            idx = self.matches(box)
            idx = idx[:np.searchsorted(idx, n)]
            m, o = len(idx), self.oracle
            image = o.synth_image(small_spec(1, m, fmt=1), transposed=True).copy()
            otp = o.parse_header(image[:400].tobytes()).offset_to_point_data
            image[otp:otp + 12 * m] = np.ascontiguousarray(self.xyz[idx]).view(np.uint8).reshape(-1)
            image[otp + 15 * m:otp + 16 * m] = self.cls[idx]
            og, oc = o.grid_collector(box[0], box[1], cell), o.count_collector()
            assert o.search_last_bounds(image, box[0], box[1], oc) == 0 and oc.point_count() == m   # every point of the image matches
            oc.free()
            assert o.search_last_bounds(image, box[0], box[1], og) == 0
            self._grids[box, cell, n] = (og, m)
        return self._grids[box, cell, n]

    def free(self):
        for og, _ in self._grids.values():
            og.free()
        self.ctx.free(self.d_xyz)
        self.ctx.free(self.d_cls)


@pytest.fixture(scope="module")
def ctx():
    with pkg.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def corpus(ctx, oracle):
    c = Corpus(ctx, oracle)
    yield c
    c.free()


def run(ctx, corpus, box, cell, n, compaction, level2, **opts):
    """One scan of the first n points; the fold takes the path the case names.  Returns the tuples that left pass 0."""
    og, m = corpus.grid(box, cell, n)
    with options(ctx, **opts):
        before = {k: ctx.get_option(k) for k in ("grid_compactions", "grid_refolds", "grid_level2", "grid_folds")}
        gg = ctx.grid_collector(box[0], box[1], cell)
        try:
            ctx.scan_dev(corpus.columns(0, n), corpus.pred(box), gg)
            check_same(gg, og)
            tuples, f2 = ctx.get_option("grid_last_tuples"), ctx.get_option("grid_last_f2")
            print("tiles", gt.ntiles(n), "cell", cell, opts, "matches", m, "tuples", tuples, "cells", og.point_count(), "f2", f2)
            assert 0 < tuples <= m
            assert ctx.get_option("grid_folds") == before["grid_folds"] + 1
            assert ctx.get_option("grid_refolds") == before["grid_refolds"]
            assert ctx.get_option("grid_compactions") == before["grid_compactions"] + compaction
            assert ctx.get_option("grid_level2") == before["grid_level2"] + level2
            assert f2 == opts["grid_f2"] or (opts["grid_f2"] == 0 and (f2 > 1) == bool(level2))
        finally:
            gg.free()
    return tuples


SIZES = pytest.mark.parametrize("n", [N, N1], ids=["4198 tiles", "4096 tiles"])


def test_the_boxes_stand_on_both_sides_of_the_compaction_rule(corpus):
    thin, thick = len(corpus.matches(THIN)), len(corpus.matches(THICK))
    assert T == 4198 and gt.prefix_chunks(T) == 2 and gt.windows(T) == (9, 102) and gt.stream_batches(T) == 66
    assert N // 120 < thin < N // 80 and gt.compacts(T, thin) and gt.compacts(gt.ntiles(N1), thin)
    assert thick >= 1.05 * 2 * T * gt.F1 and not gt.compacts(T, thick)
    # (pass 0's own fold may shed tuples before the rule is applied: the thick cases assert that what is left stays above it)
    # the counts of the second chunk of k_bin_prefix are not all zero: both boxes have matches in the tiles from 4096 on
    assert np.count_nonzero(corpus.matches(THIN) >= N1) > 1000 and np.count_nonzero(corpus.matches(THICK) >= N1) > 100_000


@SIZES
@pytest.mark.parametrize("name,cell,compaction,level2,opts", [
    ("coarse, streamed as it lies", 0.5, 0, 0, dict(grid_f2=1, grid_stream=1)),
    ("coarse, copied together for k_fold<BIG>", 0.5, 1, 0, dict(grid_f2=1, grid_stream=0)),
    ("dense, copied together for the second level", 0.05, 1, 1, dict(grid_f2=8, grid_stream=1)),
    ("the probe decides", 0.05, 0, 0, dict(grid_f2=0, grid_stream=1))], ids=["coarse-stream", "coarse-big", "dense-f2-8", "probe"])
def test_thin_box_short_fragments(ctx, corpus, name, cell, compaction, level2, opts, n):
    """215 k matches in 2.1 M fragments.  The last case: the probe counts the distinct cells of two bins over all T fragments and
    finds a fold that needs no second level; the streaming fold then reads the sparse run."""
    run(ctx, corpus, THIN, cell, n, compaction, level2, **opts)


@SIZES
@pytest.mark.parametrize("name,cell,level2,opts", [
    ("coarse: k_fold<BIG> through nine windows", 0.5, 0, dict(grid_f2=1, grid_stream=0)),
    ("dense: k_level2's windows", 0.1, 1, dict(grid_f2=16, grid_stream=1))], ids=["coarse-big", "dense-f2-16"])
def test_thick_box_fragments_read_as_they_lie(ctx, corpus, name, cell, level2, opts, n):
    tuples = run(ctx, corpus, THICK, cell, n, 0, level2, **opts)
    assert not gt.compacts(gt.ntiles(n), tuples)


def test_thick_box_dense_grid_with_the_fan_out_from_the_probe(ctx, corpus):
    """grid_f2 = 0 with 9800 tuples per bin: k_probe_distinct's estimate over all T fragments of two bins sets the fan-out"""
    run(ctx, corpus, THICK, 0.1, N, 0, 1, grid_f2=0, grid_stream=1)


def test_thick_box_scanned_as_two_runs_into_one_collector(ctx, corpus):
    """2100 tiles, then the rest, with first_index continuing: the second run's first tile lies beyond 2048 (k_dir_transpose's run
    search), and one fold reads both runs' fragments through the same windows"""
    cell, first = 0.5, 2100 * gt.TILE
    og, _ = corpus.grid(THICK, cell, N)
    with options(ctx, grid_f2=1, grid_stream=0):
        folds, compactions = ctx.get_option("grid_folds"), ctx.get_option("grid_compactions")
        gg = ctx.grid_collector(THICK[0], THICK[1], cell)
        try:
            ctx.scan_dev(corpus.columns(0, first), corpus.pred(THICK), gg)
            ctx.scan_dev(corpus.columns(first, N - first), corpus.pred(THICK), gg)
            check_same(gg, og)
            assert ctx.get_option("grid_folds") == folds + 1 and ctx.get_option("grid_compactions") == compactions
        finally:
            gg.free()
