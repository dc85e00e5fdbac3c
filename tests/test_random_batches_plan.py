"""The committed seeds of _random_batches.py and of _random_resident.py proven on the CPU, before a GPU sees them: every case
satisfies every precondition of every batched entry (include/pcq.h) and of every resident count query (include/pcq_query.h) — a
refusal on the GPU is then a failure, not a skipped seed — and the seed ranges reach what they are there for.  These are conditions, not measurements: the generator was tuned until they held, and a change of the
generator that loses one fails here.
"""
import functools
import hashlib

import numpy as np
import pytest

import _random_batches as rb
import _random_resident as rr
from _random_batches import I32_MAX, I32_MIN


# What the first ten entries of each module drew at commit c1949bf ("Ground-only mean-height raster: a class set in the z-sum raster
# pass"), the last one before the mean-height entries joined them: SHA-256 over every seed's data, queries and answers
# (batches_digest, resident_digest), computed there with these two functions.  The later entries draw from generators of their own.
BATCHES_DIGEST_AT_C1949BF = "ca415a8ab0ae9fdf23a5e3e7765e5e0d878217b1999cffae0fdd6c9dae32da37"
RESIDENT_DIGEST_AT_C1949BF = "0c829a68dbc6e09a800276862e4c2bb039a443d5d098f66bdf5473de95aef589"
BATCHES_TEN = ("box", "class", "box_class", "box_time", "multi", "class_hist", "time_hist", "raster", "zrange", "polygon")
RESIDENT_TEN = ("bounds", "class", "bounds_class", "bounds_time", "many", "by_class", "by_time", "raster", "zrange", "polygon")


def _put(h, *things):
    """Arrays as their dtype, shape and bytes; everything else (integers, floats, strings, nested lists of them) as its repr"""
    for x in things:
        if isinstance(x, np.ndarray):
            h.update(repr((x.dtype.str, x.shape)).encode() + np.ascontiguousarray(x).tobytes())
        elif isinstance(x, (list, tuple)) and any(isinstance(v, np.ndarray) for v in x):
            _put(h, len(x), *x)
        else:
            h.update(repr(x).encode())


def batches_digest(cs):
    h = hashlib.sha256()
    for c in cs:
        _put(h, c.seed + rb.SEED_BASE, c.n, c.S, c.cphase, c.tphase, c.poff, c.psize, c.coff, c.csize, c.toff, c.tsize, c.dist, c.xyz, c.class_values, c.cls,
             c.edges, c.nq, c.raster_dims, c.zrange_dims, c.nverts, c.t, c.ranges, c.qclass, c.cclass, sorted(c.box.items()), c.multi, c.raster,
             c.zrange, c.polygon, c.passing)
        for e in BATCHES_TEN:
            _put(h, e, c.share[e], c.mask.get(e, ()))
    return h.hexdigest()


def resident_digest(cs):
    h = hashlib.sha256()
    for c in cs:
        _put(h, c.seed + rr.SEED_BASE, len(c.files))
        for f in c.files:
            _put(h, f.fmt, f.n, f.scale, f.offset, f.xyz, f.cls, f.t, f.world, f.hmin, f.hmax, f.hidden, f.lying)
        for e in RESIDENT_TEN:
            _put(h, e, sorted((k, v) for k, v in vars(c.q[e]).items() if not isinstance(v, np.ndarray)),
                 [v for k, v in sorted(vars(c.q[e]).items()) if isinstance(v, np.ndarray)])
            _put(h, [k for k, v in sorted(c.answer[e].items())], [np.asarray(v) for k, v in sorted(c.answer[e].items())])
        _put(h, [e for e in c.lie_decides if e in RESIDENT_TEN])
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def cases():
    return [rb.draw(seed) for seed in rb.SEEDS]


def test_the_first_ten_entries_draw_what_they_drew_before_the_mean_height_raster():
    """(the committed seeds, also in a soak run, which moves every other test to other seeds)"""
    cs = cases() if rb.SEED_BASE == 0 else [rb.draw(seed - rb.SEED_BASE) for seed in rb.SEEDS]
    assert batches_digest(cs) == BATCHES_DIGEST_AT_C1949BF


def test_a_draw_is_a_function_of_its_seed():
    a, b = rb.draw(5), cases()[5]
    assert a.n == b.n and all(np.array_equal(x, y) for x, y in zip(a.xyz, b.xyz)) and np.array_equal(a.edges, b.edges)
    assert all(np.array_equal(a.share[e], b.share[e]) for e in rb.ENTRIES if e != "zrange")
    assert a.n != cases()[6].n


def check_raster(rows, dims, cells_max):
    nx, ny = dims
    assert nx >= 1 and ny >= 1 and nx * ny <= cells_max
    for lo, hi, cw in rows:
        assert all(1 <= w <= 2**32 - 1 for w in cw)
        if rb.box_is_empty(lo, hi):
            continue
        for a in range(2):
            assert I32_MIN <= lo[a] <= I32_MAX
            assert (min(hi[a], I32_MAX) - lo[a]) // cw[a] < dims[a]


@pytest.mark.parametrize("seed", rb.SEEDS)
def test_every_precondition_of_every_entry(seed):
    c = cases()[seed]
    S = c.S
    assert 1 <= S <= rb.S_MAX and sum(c.n) <= rb.CAP
    # layouts: positions 16-byte aligned, class bytes anywhere, times 8-byte aligned, pieces apart
    for off, size, unit, phase in ((c.poff, c.psize, 12, [0] * S), (c.coff, c.csize, 1, c.cphase), (c.toff, c.tsize, 8, c.tphase)):
        assert all(o % 16 == ph for o, ph in zip(off, phase))
        ends = [o + n * unit for o, n in zip(off, c.n)]
        assert all(e <= o for e, o in zip(ends, off[1:])) and ends[-1] <= size
    assert all(ph in (0, 8) for ph in c.tphase) and all(0 <= ph < 16 for ph in c.cphase)
    for k in range(S):
        assert c.xyz[k].dtype == np.int32 and c.xyz[k].shape == (c.n[k], 3)
        assert c.cls[k].dtype == np.uint8 and len(c.cls[k]) == c.n[k] and c.t[k].dtype == np.float64 and len(c.t[k]) == c.n[k]
        assert 0 <= c.qclass[k] < 256 and 0 <= c.cclass[k] < 256
    # every box fits the predicate's i64 fields
    for e in rb.ENTRIES:
        for k in range(S):
            for lo, hi in rb.boxes_of(c, e, k):
                assert all(-2**63 <= v < 2**63 for v in (*lo, *hi))
    assert 1 <= c.nq <= rb.MULTI_BOX_MAX and all(len(row) == c.nq for row in c.multi)
    e = c.edges
    assert 1 <= len(e) - 1 <= rb.TIME_BINS_MAX and not np.isnan(e).any() and np.all(e[:-1] <= e[1:])
    check_raster(c.raster, c.raster_dims, rb.RASTER_CELLS_MAX)
    check_raster(c.zrange, c.zrange_dims, rb.ZRANGE_CELLS_MAX)
    check_raster(c.zsum, c.zsum_dims, rb.ZSUM_CELLS_MAX)
    assert 3 <= c.nverts <= rb.POLYGON_VERTS_MAX
    for lo, hi, verts in c.polygon:
        assert len(verts) == c.nverts and all(I32_MIN <= v <= I32_MAX for xy in verts for v in xy)
        if rb.box_is_empty(lo, hi):
            continue
        for a in range(2):
            vs = [xy[a] for xy in verts]
            assert max(min(hi[a], I32_MAX), *vs) - min(max(lo[a], I32_MIN), *vs) <= rb.SPAN_MAX


def test_the_layouts_occur():
    cs = cases()
    seen = {n for c in cs for n in c.n}
    assert set(rb.N_LIST) <= seen and max(seen) > 4096 + 16 and any(n not in rb.N_LIST for n in seen)
    assert {ph for c in cs for ph, n in zip(c.cphase, c.n) if n} == set(range(16))
    assert {ph for c in cs for ph, n in zip(c.tphase, c.n) if n} == {0, 8}
    assert {d for c in cs for d, n in zip(c.dist, c.n) if n >= 64} == set(rb.DISTS)
    assert any(len({d for d, n in zip(c.dist, c.n) if n}) >= 3 for c in cs)  # mixed within a case
    assert {c.nverts for c in cs} >= {3, rb.POLYGON_VERTS_MAX} and {c.nq for c in cs} == set(range(1, 9))
    assert {1, rb.TIME_BINS_MAX} <= {len(c.edges) - 1 for c in cs}
    assert any(np.isinf(c.edges[0]) for c in cs) and any(np.isinf(c.edges[-1]) for c in cs)
    assert any(np.signbit(c.edges[0]) and c.edges[0] == 0 for c in cs) and any((np.diff(c.edges) == 0).any() for c in cs)


def test_the_limits_of_i32_pass_a_box_on_every_axis():
    for a in range(3):
        for v in (I32_MIN, I32_MAX):
            assert any((p[:, a] == v).any() for c in cases() for p in c.passing), (a, v)


def test_the_planted_times_decide_answers():
    """A time on the last edge, inside its box: what tells a half-open last bin from a closed one; and times one double below a
    range's end and on it"""
    on_last = on_end = below_end = 0
    for c in cases():
        for k in range(c.S):
            sel = rb.pp.in_box(c.xyz[k], *c.box["time_hist"][k])
            on_last += int((c.t[k][sel] == c.edges[-1]).sum()) if c.edges[-1] > c.edges[0] else 0
            sel = rb.pp.in_box(c.xyz[k], *c.box["box_time"][k])
            t0, t1 = c.ranges[k]
            if t0 < t1:
                on_end += int((c.t[k][sel] == t1).sum())
                below_end += int((c.t[k][sel] == np.nextafter(t1, -np.inf)).sum())
    assert on_last >= 10 and on_end >= 10 and below_end >= 10


@pytest.mark.parametrize("entry", rb.ENTRIES)
def test_the_answers_are_worth_asking_for(entry):
    cs = cases()
    zero = sum(not rb.live(c, entry).any() for c in cs)
    cap = 10 if entry in rb.FIRST_TEN else 4  # (an entry that joined later: at most a quarter of its seeds)
    assert cap * zero <= len(cs), f"{zero} of {len(cs)} cases leave the answer untouched"
    if entry == "zrange":
        more = sum(int((c.share[entry][0] != I32_MAX).sum()) > 1 for c in cs)
    elif entry == "zsum":
        more = sum(int(rb.answer(c, entry)[0].sum()) > 1 for c in cs)
    else:
        more = sum(int(rb.answer(c, entry).sum()) > 1 for c in cs)
    assert 2 * more >= len(cs), f"only {more} of {len(cs)} cases have more than a single match"
    between = 0
    for c in cs:
        lv, dd = rb.live(c, entry), rb.dead(c, entry)
        between += any(dd[j] and lv[:j].any() and lv[j + 1:].any() for j in range(c.S))
    assert between >= 1, "no case with an empty-predicate segment between two live ones"


@pytest.mark.parametrize("entry", rb.COUNTS_WITH_STEPS)
def test_matches_from_whole_steps_and_from_leftovers(entry):
    both = 0
    for c in cases():
        tiles = left = 0
        for k, m in enumerate(c.mask[entry]):
            whole = c.n[k] // rb.K1_STEP * rb.K1_STEP
            tiles += int(m[:whole].sum())
            left += int(m[whole:].sum())
        both += tiles > 0 and left > 0
    assert both >= 1


def test_the_mean_height_raster_reaches_what_it_is_for():
    """The entry that joined later, over its 48 seeds: the shapes at the limit and the small ones, sums of both signs and beyond 32
    bits (the "wide" positions plant INT32_MIN / INT32_MAX on z), a cell that a whole wave adds into, matches from whole steps and
    from leftovers, and at most a quarter of the seeds with nothing to add"""
    cs = cases()
    shapes = {c.zsum_dims for c in cs}
    assert {(2048, 1), (1, 2048), (64, 32), (3, 5), (1, 1)} <= shapes and any(d not in rb.ZSUM_SHAPES for d in shapes)
    assert any(any(w not in rb.CELL_WIDTHS for _, _, cw in c.zsum for w in cw) for c in cs)
    negative = wide = crowded = both = zero = 0
    for c in cs:
        cnt, zsum = rb.answer(c, "zsum")
        assert cnt.dtype == zsum.dtype == np.int64 and not zsum[cnt == 0].any()
        assert abs(int(np.abs(c.share["zsum"][1]).sum())) < 2**62  # (numpy's int64 is the exact value)
        zero += not cnt.any()
        negative += bool((zsum[cnt > 0] < 0).any())
        wide += bool((np.abs(zsum) > 2**32).any())
        crowded += bool((cnt >= 64).any())
        tiles = sum(int(m[:c.n[k] // rb.K1_STEP * rb.K1_STEP].sum()) for k, m in enumerate(c.mask["zsum"]))
        left = sum(int(m[c.n[k] // rb.K1_STEP * rb.K1_STEP:].sum()) for k, m in enumerate(c.mask["zsum"]))
        both += tiles > 0 and left > 0
    assert 4 * zero <= len(cs), f"{zero} of {len(cs)} seeds add nothing"
    assert negative >= 1 and wide >= 1 and crowded >= 1 and both >= 1, (negative, wide, crowded, both)


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin for the resident queries (_random_resident.py)
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resident_cases():
    return [rr.case(seed) for seed in rr.SEEDS]


def test_resident_first_ten_entries_draw_what_they_drew_before_the_mean_height_rasters():
    cs = resident_cases() if rr.SEED_BASE == 0 else [rr.draw(seed - rr.SEED_BASE) for seed in rr.SEEDS]
    assert resident_digest(cs) == RESIDENT_DIGEST_AT_C1949BF


@pytest.mark.parametrize("seed", rr.SEEDS)
def test_resident_no_call_is_refused(seed):
    """refusal() restates the rules by which host/resident.cpp refuses a call; the files are what the loader accepts"""
    c = resident_cases()[seed]
    assert 2 <= len(c.files) <= 6
    for f in c.files:
        assert f.fmt in rr.TIME_FORMATS and f.xyz.shape == (f.n, 3) and f.xyz.dtype == np.int32 and len(f.cls) == len(f.t) == f.n
        assert all(s in rr.SCALES for s in f.scale) and all(o in rr.OFFSETS for o in f.offset)
        assert np.all(f.hmin <= f.hmax)
        assert f.lying == bool(f.n and (np.any(f.world < f.hmin) or np.any(f.world > f.hmax)))
    for e in rr.ENTRIES:
        assert rr.refusal(c.files, e, c.q[e]) is None, e
    assert 1 <= len(c.q["many"].bmin) <= 20 and 3 <= len(c.q["polygon"].xy) <= rr.POLYGON_VERTS_MAX
    assert all(0 <= v < 256 for v in c.q["zmean_classes"].classes) and len(set(c.q["zmean_classes"].classes)) == len(c.q["zmean_classes"].classes)
    for e, limit in (("raster", rr.RASTER_CELLS_MAX), ("zrange", rr.ZRANGE_CELLS_MAX), ("zmean", rr.ZSUM_CELLS_MAX),
                     ("zmean_classes", rr.ZSUM_CELLS_MAX)):  # more cells than a launch holds
        assert limit < c.q[e].nx * c.q[e].ny <= rr.QUERY_RASTER_CELLS_MAX
        for f, lmin, lmax in rr.survivors(c.files, *rr.raster_world_box(c.q[e])):  # a whole multiple of every surviving file's steps
            assert all(rr.steps_of(c.q[e].cell, f.scale[a]) is not None for a in range(2))
            assert all(I32_MIN <= lmin[a] <= I32_MAX for a in range(2))
            assert np.isfinite(f.scale[2]) and f.scale[2] > 0 and f.n < 2**32


def test_resident_seeds_reach_what_they_are_for():
    cs = resident_cases()
    assert {n for c in cs for f in c.files for n in [f.n]} >= {0, 1, 63, 64, 65, 255, 256, 511, 512, 513, 1023, 1024, 1025}
    assert any(c.q["raster"].nx > rr.RASTER_CELLS_MAX for c in cs), "no density raster whose rows are cut into pieces"
    assert any(c.q["zrange"].nx > rr.ZRANGE_CELLS_MAX for c in cs), "no height raster whose rows are cut into pieces"
    assert any(len(c.q["many"].bmin) > rr.MULTI_BOX_MAX for c in cs) and any(len(c.q["many"].bmin) > 2 * rr.MULTI_BOX_MAX for c in cs)
    assert any(len(c.q["by_time"].edges) - 1 > 1024 for c in cs)
    assert any(len(set(f.scale)) > 1 for c in cs for f in c.files) and any(len(set(f.scale)) == 1 for c in cs for f in c.files)
    assert any(len({(f.scale[2], f.offset[2]) for f in c.files if f.n}) >= 3 for c in cs)  # z lattices merged on the host
    lies = [c.seed for c in cs if c.lie_decides]
    assert lies, "no seed in which a header that hides points decides an answer"
    missed = [c.seed for c in cs for e in ("bounds", "many") if np.any(np.asarray(c.answer[e]["scanned"]) < sum(f.n for f in c.files))]
    assert missed, "no box that misses a header"


@pytest.mark.parametrize("entry", rr.ENTRIES)
def test_resident_answers_are_worth_asking_for(entry):
    cs = resident_cases()
    zero = sum(rr.total(c.answer[entry]) == 0 for c in cs)
    cap = 10 if entry in rr.FIRST_TEN else 4  # (the later entries: at most a quarter — the empty class set is drawn on purpose)
    assert cap * zero <= len(cs), f"{zero} of {len(cs)} cases leave the answer empty"


@pytest.mark.parametrize("entry", ["zmean", "zmean_classes"])
def test_resident_mean_height_seeds_reach_what_they_are_for(entry):
    """Some seed merges at least three z lattices, some seed has a cell that two groups reach (there the order of the merge and the
    rounding of the two products decide the bits), some seed a NaN cell next to a reached one; rows longer than a launch occur; with
    a class set: every kind of set occurs, and some set removes some but not all points of a reached cell"""
    cs = resident_cases()
    lattices = shared = nan_beside = long_rows = partly = reordered = fused = 0
    for c in cs:
        qu = c.q[entry]
        classes = qu.classes if entry == "zmean_classes" else None
        count, zmean, scanned, per_group = rr.zmean_answer(c.files, qu, classes)
        # two mutants of the merge, exact in rationals: the groups in the reverse order, and scale * sum contracted into the add
        # (one rounding of scale * sum + a instead of two; offset * cnt is exact for these offsets, so the other contraction is none)
        groups, _ = rr.zmean_groups(c.files, qu, classes)
        order, contracted = rr.zmean_mutants(groups, len(count))
        reordered += order > 0
        fused += contracted > 0
        assert np.array_equal(np.isnan(zmean), count == 0) and np.array_equal(count, c.answer[entry]["count"])
        assert np.array_equal(zmean.view(np.uint64), c.answer[entry]["zmean"].view(np.uint64))
        lattices += len(per_group) >= 3
        shared += bool(len(per_group) >= 2 and (np.sum([g > 0 for g in per_group], axis=0) >= 2).any())
        grid = (count > 0).reshape(qu.ny, qu.nx)
        nan_beside += bool((grid[:, 1:] != grid[:, :-1]).any() or (grid[1:] != grid[:-1]).any())
        long_rows += qu.nx > rr.ZSUM_CELLS_MAX
        if classes is not None:
            every = rr.zmean_answer(c.files, qu, None)[0]
            partly += bool(((count > 0) & (count < every)).any())
            assert (count <= every).all() and (len(classes) < 256 or np.array_equal(count, every)) and (len(classes) or not count.any())
    assert lattices >= 1 and shared >= 1 and nan_beside >= 1 and long_rows >= 1, (lattices, shared, nan_beside, long_rows)
    # (the class-filtered entry runs the same merge; its sets leave fewer lattices in a cell, and no committed seed of its own
    # has a mean that the order decides)
    assert fused >= 2 and (reordered >= 2 or entry == "zmean_classes"), \
        f"the merge's order decides a mean in {reordered} seeds, the rounding of scale * sum in {fused}"
    if entry == "zmean_classes":
        assert partly >= 1
        assert {c.q[entry].kind for c in cs} == set(rr.SET_KINDS)
