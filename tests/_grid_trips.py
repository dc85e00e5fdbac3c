"""The grid collector beyond one trip of its tile and fragment loops: the corpora, their launch arithmetic and the model of pass 0's
back-off.  Every loop of csrc/grid_*.hip is sized by T, the number of pending 5120-point tiles — a function of the points SCANNED:

  k_p0_part (grid_pass0.hip)   min(ntiles, CUs) workgroups (grid_host.hip), workgroup w takes the tiles w, w + W, ...; from trip to
                               trip it carries the prefetched inputs of the next tile, two match counters used in turn, the tile
                               fold's back-off, a barrier taken only in front of a tile that starts with the duplicate table, and it
                               meets the short last tile on a later trip
  k_bin_prefix (grid_dir.hip)  a bin's T counts in chunks of 4096 with a carry
  k_fold<BIG>, k_level2        a window of BIG_FB = 512 fragments of the bin's list, refilled; k_fold_stream: batches of 64

Restated from the sources (test_grid_trips_plan.py reads them back): P0_TILE, F1, BIG_FB (grid_common.h), the 4096 of k_bin_prefix,
the workgroup count (grid_host.hip), the back-off (grid_pass0.hip: `agg`, the `total * 4 > matched * 3` rule, the cap of 16).

Three corpora.
  trips(cus)    (2 cus + 37) tiles and 1234 points in scan order (scan_ordered_image): workgroups 0 .. 36 make a third trip and
                workgroup 37's third tile is the short one.
  deep          80 tiles of four sorts in an order that takes ONE workgroup's back-off through 1, 2, 4, 8, 16, 16 and a reset (DeepCorpus);
                run on 1, 2 and 7 workgroups through the `grid_p0_blocks` option; the tuples that leave pass 0 follow from the model.
  many tiles    4096 + 64 + 37 tiles and 1234 points: T in the second chunk of k_bin_prefix, nine BIG_FB windows with a partial last.
"""
import functools
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import _time_images as ti  # noqa: E402

TILE = 5120          # P0_TILE
F1 = 512             # level-1 bins
BIG_FB = 512         # fragments in a reader's window
PREFIX_CHUNK = 4096  # k_bin_prefix: counts per trip
STREAM_BATCH = 64    # k_fold_stream: fragments per batch
BACKOFF_CAP = 16
PAYS_NUM, PAYS_DEN = 4, 3   # `total * 4 > matched * 3`: the attempt did not pay
TAIL = 1234
EXTRA = 37


# ---------------------------------------------------------------------------------------------------------------------------------
# launch arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def ntiles(n):
    return (n + TILE - 1) // TILE


def workgroups(tiles, cus, cap=0):
    """grid_host.hip: min(ntiles, CUs); the option grid_p0_blocks (cap > 0) may only lower it"""
    w = min(tiles, cus)
    return min(cap, w) if cap > 0 else w


def trips(tiles, w):
    """Per workgroup: the tiles it takes, in order (tile % W == workgroup, trip = tile // W)"""
    return [list(range(g, tiles, w)) for g in range(w)]


def tile_points(n, t):
    return min(TILE, n - t * TILE)


def windows(T, fb=BIG_FB):
    """(refills of a window of fb fragments over a list of T, fragments of the last one)"""
    w = (T + fb - 1) // fb
    return w, T - (w - 1) * fb


def prefix_chunks(T):
    return (T + PREFIX_CHUNK - 1) // PREFIX_CHUNK


def stream_batches(T):
    return (T + STREAM_BATCH - 1) // STREAM_BATCH


def compacts(T, m):
    """grid_host.hip: short fragments are copied together first"""
    return T > 2 * BIG_FB and m < 2 * T * F1


def trips_points(cus):
    return (2 * cus + EXTRA) * TILE + TAIL


MANY_TILES = PREFIX_CHUNK + 64 + EXTRA
MANY_POINTS = MANY_TILES * TILE + TAIL
ONE_CHUNK_POINTS = PREFIX_CHUNK * TILE


# ---------------------------------------------------------------------------------------------------------------------------------
# the back-off of k_p0_part, per workgroup (grid_pass0.hip: `const bool agg = ...` at the head of a trip, the update behind the copy-out)
# ---------------------------------------------------------------------------------------------------------------------------------
def backoff_walk(matched, folded, mode=0, model="right"):
    """One workgroup over its tiles (matched[i] points pass the predicate, folded[i] of them survive the tile's own fold): the tuples
    that leave per tile, and per tile (attempted, back-off before the attempt).  mode: grid_agg (0 while it pays, 1 always, 2 never).
    model: "right", or one of three mistakes — "no_reset" (a paying attempt leaves the back-off where it is), "skip_from_attempt" (the
    tiles left alone are counted from the attempt itself, one fewer), "empty_fails" (a tile without a match counts as not paying)."""
    skip, backoff = 0, 1
    out, trace = [], []
    for m, f in zip(matched, folded):
        agg = mode == 1 or (mode == 0 and skip == 0)
        trace.append((agg, backoff))
        total = f if agg else m
        out.append(total)
        if agg and mode == 0:
            fails = total * PAYS_NUM > m * PAYS_DEN
            if model == "empty_fails" and m == 0:
                fails = True
            if fails:
                backoff = backoff * 2 if backoff < BACKOFF_CAP else BACKOFF_CAP
                skip = backoff - 1 if model == "skip_from_attempt" else backoff
            elif model != "no_reset":
                backoff = 1
        elif skip:
            skip -= 1
    return out, trace


def tuples_leaving(matched, folded, w, mode=0, model="right"):
    """The sum over the workgroups of a launch of w: what grid_last_tuples reads after the fold"""
    matched, folded = list(matched), list(folded)
    total = 0
    for mine in trips(len(matched), w):
        total += sum(backoff_walk([matched[t] for t in mine], [folded[t] for t in mine], mode, model)[0])
    return total


# ---------------------------------------------------------------------------------------------------------------------------------
# scan-ordered files
# ---------------------------------------------------------------------------------------------------------------------------------
def scan_order(xyz, seed, snap_step=512, snap_fraction=0.5):
    """Points sorted along x inside y strips (scan lines, boustrophedon), half of them snapped to a coarse lattice — runs of identical
    positions with different attributes: equal distances, the first in file order must win — and with the last point of every tile
    repeated as the first point of the next one (a tie across the boundary)."""
    n = len(xyz)
    xyz = xyz.copy()
    rng = np.random.default_rng(seed)
    snap = rng.random(n) < snap_fraction
    xyz[snap] = xyz[snap] // snap_step * snap_step
    strip = xyz[:, 1] // 400
    order = np.lexsort((np.where(strip % 2 == 0, xyz[:, 0], -xyz[:, 0]), strip))
    xyz = xyz[order]
    for k in range(TILE, n, TILE):
        xyz[k] = xyz[k - 1]
    return xyz


def scan_ordered_image(oracle, seed, n, fmt, snap_step=512, snap_fraction=0.5):
    """A LAST image of the oracle's synthesiser (formats 1 and 2) with its positions put in scan order (scan_order)"""
    specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")
    seed += int(os.environ.get("PCQ_TEST_SEED_BASE", "0"))  # a soak run: other seeds than the committed ones
    spec = specs._spec(seed, n, fmt, (0.01, 0.01, 0.01), (0.0, 0.0, 0.0), (-5000, -5000, -1000), (10001, 10001, 2001), zo=None,
                       classes=[(1, 0.5), (2, 0.3), (6, 0.2)])
    image = oracle.synth_image(spec, transposed=True).copy()
    hdr = oracle.parse_header(image[:400].tobytes())
    otp = hdr.offset_to_point_data
    xyz = image[otp:otp + 12 * n].view("<i4").reshape(n, 3).copy()
    xyz = scan_order(xyz, seed, snap_step, snap_fraction)
    image[otp:otp + 12 * n] = np.frombuffer(np.ascontiguousarray(xyz).tobytes(), dtype=np.uint8)
    return image, hdr


def last_columns(image, hdr):
    """(xyz [n, 3] i32, class bytes) of a LAST image of format 0 .. 5"""
    n, otp = hdr.number_of_points, hdr.offset_to_point_data
    return image[otp:otp + 12 * n].view("<i4").reshape(n, 3), image[otp + 15 * n:otp + 16 * n]


class KindsCorpus:
    """40 tiles and 1234 points in scan order with class bytes, colours and GPS times, as arrays; images by _time_images.  On three
    workgroups every one makes 13 or 14 trips."""
    N = 40 * TILE + TAIL

    def __init__(self, seed=20270):
        seed += int(os.environ.get("PCQ_TEST_SEED_BASE", "0"))
        n = self.n = self.N
        rng = np.random.default_rng(seed)
        xyz = np.stack([rng.integers(-5000, 5001, n), rng.integers(-5000, 5001, n), rng.integers(-1000, 1001, n)], axis=1).astype(np.int32)
        self.xyz = scan_order(xyz, seed)
        self.cls = rng.choice(np.array([1, 2, 6], dtype=np.uint8), n, p=[0.5, 0.3, 0.2])
        self.rgb = rng.integers(1, 65536, (n, 3)).astype(np.uint16)
        self.t = np.sort(rng.uniform(1000.0, 2000.0, n))
        self.t[rng.integers(0, n, 50)] = np.nan
        self.scale, self.offset = (0.01, 0.01, 0.01), (100.0, -200.0, 7.5)   # (one scale: the integer box of a world box is that box)

    @functools.lru_cache(maxsize=None)
    def image(self, layout, fmt):
        return (ti.last_image if layout == "last" else ti.las_image)(fmt, self.xyz, self.cls, self.rgb, self.t, scale=self.scale, offset=self.offset)


@functools.lru_cache(maxsize=1)
def kinds_corpus():
    return KindsCorpus()


# ---------------------------------------------------------------------------------------------------------------------------------
# the deep-trip corpus
# ---------------------------------------------------------------------------------------------------------------------------------
# Scale 2^-10, offset 0, cells of 64.0 from an integer corner: a cell is 65536 units wide and its centre is the unit 32768 of it, so a
# point can lie on the centre exactly (distance 0) and every distance is exact in binary64.  128 x 128 x 32 cells, all inside the box:
# no key aliases.  Every side of the box is below 2^24 units: 16-byte tuples.
DEEP_SCALE = (2.0 ** -10,) * 3
DEEP_OFFSET = (0.0, 0.0, 0.0)
DEEP_CELL = 64.0
DEEP_DIMS = (128, 128, 32)
DEEP_BMIN = (-4096.0, -4096.0, -1024.0)
DEEP_BMAX = (4096.0, 4096.0, 1024.0)
UNITS = 65536        # per cell
CENTRE = UNITS // 2

# C: a cluster tile — all points in one cell, one on the centre, the others at pairwise different distances (k units along x, k = 1 ..:
#    (k / 1024)^2 differs from its neighbour's by 2 / k > 2^-12 of itself, the table word drops 13 of 52 mantissa bits); 1 tuple
#    survives the tile's fold.
# S: a spread tile — every point in a cell of its own: all survive, the attempt does not pay.
# P: 3839 spread points and a cluster of 1281: 3840 survive of 5120; 3840 * 4 > 5120 * 3 is false, it pays.
# N: 3840 spread points and a cluster of 1280: 3841 survive, it does not pay.
#    (The centre point's table word is (0 + 1) << 13 | place, the smallest a tuple that is not aliased can have: the cluster wins its
#    slot against any spread point hashed there, which is then kept as a tuple of another key.)
# E: no point inside the box: matched = 0 counts as paying.
# The order below, on ONE workgroup: an attempt fails at back-off 1 (tile 0; 2 tiles left alone), the empty tile resets it (3), attempts
# fail at 1, 2, 4, 8, 16 and 16 (tiles 4, 7, 12, 21, 38, 55), a cluster resets (72), a table tile directly behind a table tile (73),
# both threshold tiles (74 pays, 75 does not: tiles 76, 77 left alone), a table tile behind a tile without one (78), and the short
# tile (79 + TAIL points: a cluster).  The tiles left alone are clusters and spread tiles in a seeded mix: where exactly an attempt
# lands shows in the tuples that leave.
DEEP_ATTEMPTS = {0: "S", 3: "E", 4: "S", 7: "S", 12: "S", 21: "S", 38: "S", 55: "S", 72: "C", 73: "C", 74: "P", 75: "N", 78: "C", 79: "C"}
DEEP_FAILS_AT = [1, 1, 2, 4, 8, 16, 16]   # the back-off in front of each failing attempt of tiles 0 .. 71
DEEP_TILES = 80
SPREAD_IN = {"C": 0, "S": TILE, "P": 3839, "N": 3840, "E": 0}
FOLDED = {"C": 1, "S": TILE, "P": 3840, "N": 3841, "E": 0}


def deep_kinds(seed=5):
    rng = np.random.default_rng(seed)
    kinds = [DEEP_ATTEMPTS.get(t) or ("C" if rng.random() < 0.5 else "S") for t in range(DEEP_TILES)]
    kinds[1], kinds[2] = "C", "C"
    return kinds


class DeepCorpus:
    def __init__(self, tiles=None, tail=TAIL, seed=77):
        self.kinds = kinds = deep_kinds() if tiles is None else list(tiles)
        self.n = n = (len(kinds) - 1) * TILE + tail
        rng = np.random.default_rng(seed)
        ncells = int(np.prod(DEEP_DIMS))
        cells = rng.permutation(ncells)   # every cluster and every spread point draws its own cell
        used = 0
        xyz = np.empty((n, 3), dtype=np.int64)
        self.matched, self.folded, self.clusters, self.spread = [], [], 0, 0
        corner = np.asarray(DEEP_BMIN) / DEEP_SCALE[0]
        for t, kind in enumerate(kinds):
            a, npts = t * TILE, min(TILE, n - t * TILE)
            ns = min(SPREAD_IN[kind], npts)
            nc = npts - ns
            place = rng.permutation(npts)   # the cluster's points and the spread ones mixed; the centre point anywhere
            block = np.empty((npts, 3), dtype=np.int64)
            if kind == "E":
                c = np.stack(np.unravel_index(cells[used:used + npts], DEEP_DIMS), axis=1)
                used += npts
                block[:] = c * UNITS + rng.integers(1, UNITS, (npts, 3))
                block[:, 2] += DEEP_DIMS[2] * UNITS   # above the box
                self.matched.append(0), self.folded.append(0)
            else:
                if nc:
                    c = np.asarray(np.unravel_index(cells[used], DEEP_DIMS))
                    used += 1
                    block[place[:nc]] = c * UNITS + CENTRE
                    block[place[:nc], 0] += np.arange(nc)   # k = 0: the centre itself
                    self.clusters += 1
                if ns:
                    c = np.stack(np.unravel_index(cells[used:used + ns], DEEP_DIMS), axis=1)
                    used += ns
                    off = rng.integers(1, UNITS, (ns, 3))
                    off[:, 0] |= 1   # never the centre
                    block[place[nc:]] = c * UNITS + off
                    self.spread += ns
                self.matched.append(npts)
                self.folded.append((1 if nc else 0) + ns)   # the cluster's centre point and every spread point
            xyz[a:a + npts] = block + corner.astype(np.int64)
        assert used <= ncells
        self.xyz = xyz.astype(np.int32)
        self.cls = rng.choice(np.array([1, 2, 6], dtype=np.uint8), n)
        self.cells = self.clusters + self.spread

    @functools.lru_cache(maxsize=None)
    def image(self):
        """LAST, format 1"""
        return ti.last_image(1, self.xyz, self.cls, None, np.zeros(self.n), scale=DEEP_SCALE, offset=DEEP_OFFSET)

    def expected_tuples(self, w, mode, model="right"):
        return tuples_leaving(self.matched, self.folded, w, mode, model)


@functools.lru_cache(maxsize=1)
def deep_corpus():
    return DeepCorpus()


def check_same(gg, og):
    """Same point count, same sorted cell keys, every byte of every winner record"""
    assert gg.point_count() == og.point_count()
    gp, gk = gg.points(), gg.grid_cells()
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], og.grid_cells())
    assert gp[order].tobytes() == og.points().tobytes()  # per cell: the same winner, every byte
