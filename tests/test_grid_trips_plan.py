"""The corpora of _grid_trips.py proven on the CPU: for devices of 64, 256 and 304 CUs each one reaches the trips, chunks and windows
it is for, the proofs fail for half the tiles and for a doubled workgroup cap, three mistaken back-off models give other tuple counts
than the right one, and the oracle alone finds in the deep-trip corpus the cells its construction predicts.  The constants the
module restates are read back out of the sources: a retuned tile, window or back-off breaks this test rather than silently
shrinking what test_gpu_grid_trips.py and test_gpu_grid_many_tiles.py cover.
"""
import os
import re

import numpy as np
import pytest

import _grid_trips as gt
from _pipeline_plan import CU_COUNTS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adhoc-queries-pointclouds_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_restated_constants_are_the_sources():
    common = source("grid_common.h")
    nt, items = map(int, re.search(r"constexpr int P0_NT = (\d+), P0_ITEMS = (\d+);", common).groups())
    assert "constexpr int P0_TILE = P0_NT * P0_ITEMS;" in common and nt * items == gt.TILE
    assert 1 << int(re.search(r"constexpr int F1_BITS = (\d+);", common).group(1)) == gt.F1 and "constexpr int F1 = 1 << F1_BITS;" in common
    assert int(re.search(r"constexpr int BIG_FB = (\d+);", common).group(1)) == gt.BIG_FB
    assert int(re.search(r"for \(uint32_t c0 = 0; c0 < T; c0 \+= (\d+)\)", source("grid_dir.hip")).group(1)) == gt.PREFIX_CHUNK
    assert "fragments 64 at a time" in source("grid_fold_stream.hip") and gt.STREAM_BATCH == 64
    host = source("grid_host.hip")
    # one workgroup per CU, never more than tiles; the option only lowers it
    assert "const unsigned per_cu = ntiles < (uint32_t)ctx->num_cus ? ntiles : (unsigned)ctx->num_cus;" in host
    assert "const unsigned nblocks = ctx->grid_p0_blocks > 0 && (unsigned)ctx->grid_p0_blocks < per_cu ? (unsigned)ctx->grid_p0_blocks : per_cu;" in host
    assert "dim3(nblocks), dim3(P0_NT)" in host
    assert "if (T > 2u * BIG_FB && m < 2ull * T * F1 && !stream_reads_bins) {" in host
    p0 = source("grid_pass0.hip")
    assert "for (; tile < ntiles; tile += gridDim.x, parity ^= 1) {" in p0
    assert "const bool agg = agg_mode == 1 || (agg_mode == 0 && agg_skip == 0);" in p0
    rule = re.search(r"if \(agg && agg_mode == 0\) \{\s*if \(total \* (\d+) > matched \* (\d+)\) \{[^\n]*\n\s*agg_backoff = agg_backoff < (\d+) \? agg_backoff \* 2 : (\d+);\s*"
                     r"agg_skip = agg_backoff;\s*\} else \{\s*agg_backoff = 1;\s*\}\s*\} else if \(agg_skip\) \{\s*agg_skip--;\s*\}", p0)
    assert rule, "the back-off of k_p0_part has changed: restate it in _grid_trips.backoff_walk"
    assert tuple(map(int, rule.groups())) == (gt.PAYS_NUM, gt.PAYS_DEN, gt.BACKOFF_CAP, gt.BACKOFF_CAP)
    assert "uint32_t agg_skip = 0, agg_backoff = 1, parity = 0;" in p0


# ---------------------------------------------------------------------------------------------------------------------------------
# pass 0 at the device's own geometry
# ---------------------------------------------------------------------------------------------------------------------------------
def third_trip_proof(n, cus, cap=0):
    """What the trips corpus is for: 37 workgroups make a third trip, the 38th's third tile is the short one, nobody a fourth"""
    tiles = gt.ntiles(n)
    w = gt.workgroups(tiles, cus, cap)
    mine = gt.trips(tiles, w)
    third = [g for g in range(w) if len(mine[g]) >= 3 and gt.tile_points(n, mine[g][2]) == gt.TILE]
    short = [g for g in range(w) if len(mine[g]) >= 3 and gt.tile_points(n, mine[g][2]) < gt.TILE]
    return (w == cus and third == list(range(gt.EXTRA)) and short == [gt.EXTRA] and max(map(len, mine)) == 3
            and gt.tile_points(n, mine[gt.EXTRA][2]) == gt.TAIL)


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_the_trips_corpus_reaches_a_third_trip_and_the_short_tile_on_it(cus):
    n = gt.trips_points(cus)
    assert third_trip_proof(n, cus)
    if cus == 256:
        assert n == 2_812_114 and gt.ntiles(n) == 550
    # ... and the proof is not vacuous: half the tiles make no third trip, a doubled workgroup cap (a device of twice the CUs) neither
    assert not third_trip_proof(gt.ntiles(n) // 2 * gt.TILE + gt.TAIL, cus)
    assert not third_trip_proof(n, 2 * cus)
    # the kinds corpus on three workgroups: 13 to 14 trips each, the short tile last
    tiles = gt.ntiles(gt.KindsCorpus.N)
    assert sorted(set(map(len, gt.trips(tiles, gt.workgroups(tiles, cus, 3))))) == [13, 14]


# ---------------------------------------------------------------------------------------------------------------------------------
# the fragment loops
# ---------------------------------------------------------------------------------------------------------------------------------
def fragment_proof(n):
    T = gt.ntiles(n)
    nwin, last = gt.windows(T)
    return gt.prefix_chunks(T) >= 2 and nwin >= 9 and 0 < last < gt.BIG_FB and T > 2 * gt.BIG_FB and T % gt.STREAM_BATCH != 0


def test_the_many_tiles_corpus_reaches_a_second_prefix_chunk_and_nine_windows():
    n, T = gt.MANY_POINTS, gt.MANY_TILES
    assert n == 21_489_874 and gt.ntiles(n) == T + 1 == 4198   # (the 1234 points are a tile of their own)
    assert fragment_proof(n)
    assert gt.windows(T + 1) == (9, 102) and gt.stream_batches(T + 1) == 66 and gt.prefix_chunks(T + 1) == 2
    assert gt.prefix_chunks(gt.ntiles(gt.ONE_CHUNK_POINTS)) == 1 and gt.windows(gt.ntiles(gt.ONE_CHUNK_POINTS)) == (8, gt.BIG_FB)
    assert not fragment_proof(gt.ntiles(n) // 2 * gt.TILE)   # half the tiles: one chunk, five windows
    # thin: short fragments are copied together; thick: 5 % above the rule's edge, they are not
    thin, thick = n // 100, int(1.05 * 2 * (T + 1) * gt.F1)
    assert gt.compacts(T + 1, thin) and not gt.compacts(T + 1, thick) and thick < n // 4
    # the two runs of the thick box: the second starts at a tile beyond 2048
    assert 2100 > 2048 and (T + 1) - 2100 > 2048


# ---------------------------------------------------------------------------------------------------------------------------------
# the back-off
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_workgroup_walks_the_whole_back_off():
    c = gt.deep_corpus()
    assert len(c.kinds) == gt.DEEP_TILES and c.n == 79 * gt.TILE + gt.TAIL
    assert all(c.folded[t] == gt.FOLDED[c.kinds[t]] and c.matched[t] == (0 if c.kinds[t] == "E" else gt.TILE) for t in range(gt.DEEP_TILES - 1))
    out, trace = gt.backoff_walk(c.matched, c.folded, 0)
    attempted = [t for t, (agg, _) in enumerate(trace) if agg]
    assert attempted == sorted(gt.DEEP_ATTEMPTS)
    assert all(c.kinds[t] == k for t, k in gt.DEEP_ATTEMPTS.items())
    failing = [t for t in attempted if out[t] * gt.PAYS_NUM > c.matched[t] * gt.PAYS_DEN]
    assert failing == [0, 4, 7, 12, 21, 38, 55, 75]
    assert [trace[t][1] for t in failing[:-1]] == gt.DEEP_FAILS_AT   # every back-off value, 16 twice
    assert set(b for _, b in trace) == {1, 2, 4, 8, 16}
    assert trace[72] == (True, 16) and trace[73] == (True, 1)        # the reset from 16, a table tile behind a table tile
    assert trace[3] == (True, 2) and c.matched[3] == 0 and trace[4] == (True, 1)   # the empty tile pays
    assert (out[74], out[75]) == (3840, 3841) and trace[75] == (True, 1) and trace[76][0] is False and trace[77][0] is False
    assert trace[78] == (True, 2) and out[78] == 1                   # a table tile behind a tile without one
    assert c.matched[79] == gt.TAIL and out[79] == 1                 # the short tile folds
    # the tiles left alone are clusters and spread tiles both
    alone = [c.kinds[t] for t, (agg, _) in enumerate(trace) if not agg]
    assert alone.count("C") >= 20 and alone.count("S") >= 20
    # the threshold tiles stand on both sides of the rule
    assert not 3840 * gt.PAYS_NUM > gt.TILE * gt.PAYS_DEN and 3841 * gt.PAYS_NUM > gt.TILE * gt.PAYS_DEN


@pytest.mark.parametrize("w", [1, 2, 7])
def test_three_mistaken_back_off_models_give_other_tuple_counts(w):
    c = gt.deep_corpus()
    right = c.expected_tuples(w, 0)
    assert c.expected_tuples(w, 1) == sum(c.folded) < right < c.expected_tuples(w, 2) == sum(c.matched)
    for model in ("no_reset", "skip_from_attempt", "empty_fails"):
        assert c.expected_tuples(w, 0, model) != right, model
    # every workgroup makes many trips, and the short tile is somebody's last
    assert min(map(len, gt.trips(gt.DEEP_TILES, w))) >= gt.DEEP_TILES // 7


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_the_workgroup_cap_only_lowers(cus):
    for cap, want in ((0, min(gt.DEEP_TILES, cus)), (1, 1), (2, 2), (7, 7), (cus + 5, min(gt.DEEP_TILES, cus)), (65536, min(gt.DEEP_TILES, cus))):
        assert gt.workgroups(gt.DEEP_TILES, cus, cap) == want


def test_the_oracle_alone_finds_the_cells_of_the_deep_corpus(oracle):
    """One cell per cluster and one per spread point; every cluster's winner is the point on its centre"""
    c = gt.deep_corpus()
    assert c.clusters == sum(k in "CPN" for k in c.kinds) and c.spread == sum(gt.SPREAD_IN[k] for k in c.kinds)
    og = oracle.grid_collector(gt.DEEP_BMIN, gt.DEEP_BMAX, gt.DEEP_CELL)
    try:
        assert oracle.search_last_bounds(c.image(), gt.DEEP_BMIN, gt.DEEP_BMAX, og) == 0
        assert og.point_count() == c.cells == c.clusters + c.spread
        pts = og.points()
        on_centre = np.ones(len(pts), dtype=bool)
        for a, name in enumerate("xyz"):
            on_centre &= np.mod(pts[name] - gt.DEEP_BMIN[a], gt.DEEP_CELL) == gt.DEEP_CELL / 2
        assert int(on_centre.sum()) == c.clusters
    finally:
        og.free()
    # the matches, counted in numpy: everything but the empty tile
    lo, hi = np.asarray(gt.DEEP_BMIN) / gt.DEEP_SCALE[0], np.asarray(gt.DEEP_BMAX) / gt.DEEP_SCALE[0]
    inside = np.all((c.xyz >= lo) & (c.xyz <= hi), axis=1)
    assert [int(inside[t * gt.TILE:(t + 1) * gt.TILE].sum()) for t in range(gt.DEEP_TILES)] == c.matched
