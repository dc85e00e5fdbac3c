"""The many-segment set of _many_segments.py proven on the CPU: for devices of 64, 256 and 304 CUs and every batched kind, the set has
more segments than the kind's grid has workgroups, the leftover loop makes at least two passes, a seek jumps over the whole run of
zero-step segments, and the part of numpy's answer that only a second or later pass can deliver is there.  The helper's launch
constants are read back out of the kernels' sources: a retune of a grid breaks this test rather than silently shrinking what
test_gpu_many_segments.py covers.
"""
import functools
import os
import re

import numpy as np
import pytest

import _many_segments as ms
from _pipeline_plan import CU_COUNTS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adhoc-queries-pointclouds_amd", "csrc")


@functools.lru_cache(maxsize=None)
def shares(cus, name):
    return ms.shares(ms.data(cus), name)


@functools.lru_cache(maxsize=None)
def source_constants():
    """`constexpr <type> NAME = <integer expression>;` of the kernels' sources (not the lab's) for the names the launch arithmetic
    uses, each defined once"""
    wanted = re.compile(r"\w+_WAVES_PER_CU|\w+_LDS_PER_CU|K1_TILES|TILE_POINTS|K2_LOADS")
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        with open(os.path.join(CSRC, f)) as fh:
            for name, expr in re.findall(r"^constexpr\s+\w+\s+(\w+)\s*=\s*([0-9 *]+);", fh.read(), flags=re.M):
                if not wanted.fullmatch(name):
                    continue
                assert name not in out, f"{name} is defined twice"
                out[name] = int(np.prod([int(x) for x in expr.split("*")]))
    return out


def test_the_restated_constants_are_the_sources():
    c = source_constants()
    assert c["K1_TILES"] * c["TILE_POINTS"] == ms.K1_STEP
    assert 64 * c["K2_LOADS"] * 16 == ms.CLASS_STEP
    assert c["RASTER_LDS_PER_CU"] == c["ZRANGE_LDS_PER_CU"] == ms.LDS_PER_CU
    by_kind = {"box": c["K1_WAVES_PER_CU"], "box_class": c["K1_WAVES_PER_CU"], "box_time": c["K1_WAVES_PER_CU"], "class": c["K2_WAVES_PER_CU"],
               "multi3": c["MULTI_WAVES_PER_CU"], "multi8": c["MULTI_WAVES_PER_CU"], "class_hist": c["CLASS_HIST_WAVES_PER_CU"],
               "time_hist": c["TIME_HIST_WAVES_PER_CU"], "raster": ms.raster_waves(ms.CELLS, 4, c["RASTER_WAVES_PER_CU"], c["RASTER_LDS_PER_CU"]),
               "zrange": ms.raster_waves(ms.CELLS, 8, c["ZRANGE_WAVES_PER_CU"], c["ZRANGE_LDS_PER_CU"]), "polygon": c["POLYGON_WAVES_PER_CU"]}
    assert {k.name: k.waves for k in ms.KINDS} == by_kind
    # the set is sized by the widest grid, and the LDS limit does not bind at 16 x 8 cells
    assert max(by_kind.values()) == ms.WIDEST and by_kind["raster"] == c["RASTER_WAVES_PER_CU"] and by_kind["zrange"] == c["ZRANGE_WAVES_PER_CU"]


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_the_layout(cus):
    p = ms.plan(cus)
    S = p.S
    assert S == 2 * 16 * cus + 37 and len(p.special) == 4
    big = 8 * cus + 1
    for kind in ms.KINDS:
        st = p.seg_steps(kind)
        assert [int(st[i]) for i in (0, S // 3, 2 * S // 3, S - 1)] == [big, 2, 1, big], kind.name
        assert int(st.sum()) == 2 * big + 3 and np.all(st[p.zero_step] == 0)
        rest = p.seg_n(kind)[[0, S - 1]] - st[[0, S - 1]] * kind.step
        assert rest[0] != rest[1] and np.all(rest > 0)
    rest = p.n % ms.K1_STEP
    assert len({int(rest[i]) for i in p.special}) == 4 and all(0 < rest[i] < ms.K1_STEP for i in p.special)
    assert [int(x) for x in p.n[p.zero_step][:8]] == [1, 3, 63, 64, 65, 200, 511, 0] and set(p.n[p.zero_step].tolist()) == set(ms.CYCLE)
    # the pieces: positions 16-byte aligned, class bytes at every phase, times at 0 and 8
    assert all(o % 16 == 0 for o in p.poff)
    assert {o % 16 for o, n in zip(p.coff, p.nc) if n} == set(range(16))
    assert {o % 16 for o, n in zip(p.toff, p.n) if n} == {0, 8}
    # the point data stays near 2 (8 cus + 1) 512 + 130 S
    assert p.points() <= 2 * big * 512 + 130 * S
    # empty predicates: every fourth zero-step segment of the upper half, the last 64 segments live
    e = np.flatnonzero(p.empty)
    assert len(e) > cus and e.min() >= S // 2 and e.max() < S - ms.LIVE_TAIL and np.all(np.diff(e) % 4 == 0) and np.all(p.zero_step[e])


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_more_segments_than_workgroups_and_a_seek_over_the_run(cus):
    p = ms.plan(cus)
    seeking = set()
    for kind in ms.KINDS:
        g = p.grid(kind)
        assert g == cus * kind.waves < p.S, kind.name                      # the steps + segments bound does not bind
        assert p.steps(kind) > g, kind.name
        passes = p.passes(kind)
        assert passes.min() >= 2 and len(set(passes.tolist())) == 2, (kind.name, set(passes.tolist()))
        assert passes.sum() == p.S
        sch = p.schedule(kind)
        jumps = ms.longest_jumps(sch)
        assert max(jumps.values()) >= p.S - 4, (kind.name, jumps)
        seeking |= {c for c, over in jumps.items() if over >= p.S - 4}
        if g > 8 * cus + 1:  # a workgroup whose FIRST step lies in segment S // 3: its first seek lands inside the run
            assert any(len(s) and s[0] == p.S // 3 for s in sch.seg), kind.name
    assert seeking == {"A", "B"}
    assert p.passes(ms.KIND["polygon"]).tolist().count(3) == 37


@pytest.mark.parametrize("name", [k.name for k in ms.KINDS])
@pytest.mark.parametrize("cus", CU_COUNTS)
def test_the_later_passes_are_not_vacuous(cus, name):
    """What only the second and later passes of the leftover loop deliver: the share of the zero-step segments with index >= grid
    (all of their points are leftovers)"""
    p, kind = ms.plan(cus), ms.KIND[name]
    g = p.grid(kind)
    later = p.zero_step & (np.arange(p.S) >= g)
    sh = shares(cus, name)
    if name == "zrange":
        zmin, zmax = ms.answer(sh, later)
        assert ((zmin != ms.I32_MAX) & (zmax != ms.I32_MIN)).sum() >= 3
        firsts = ms.answer(sh, ~later)
        assert (zmin < firsts[0]).any() or (zmax > firsts[1]).any()  # some cell's extreme comes from a later pass alone
        live = (sh[0] != ms.I32_MAX).any(axis=1)
    else:
        part = ms.answer(sh, later)
        assert part.sum() > 0 and np.all(part >= 0)
        if kind.words > 8:
            assert (part > 0).sum() >= 3
        elif kind.words > 1:
            assert np.all(part > 0)  # every query, every bin
        live = sh.sum(axis=1) > 0
        # third passes too, and every size of the cycle
        third = p.zero_step & (np.arange(p.S) >= 2 * g)
        assert ms.answer(sh, third).sum() > 0
        for n in ms.CYCLE[1:]:
            assert ms.answer(sh, later & (p.seg_n(kind) == n)).sum() > 0, n
    if name != "class":  # (its predicates are never empty and its loop has no `continue`)
        assert ms.behind_an_empty(p, kind, live), "no live segment behind an empty one"
    if name == "time_hist":  # the leftovers' NaN, the value below the first edge and the last edge itself pass the box somewhere
        d = ms.data(cus)
        sel = ms.in_box(d) & later[d.seg]
        assert np.isnan(d.t[sel]).any() and (d.t[sel] < ms.EDGES[0]).any() and (d.t[sel] == ms.EDGES[-1]).any()


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_another_segments_constants_change_the_answer(cus):
    """Segment k's leftovers under the constants of segment k + grid (what a stride slip would apply): the box count of the
    zero-step segments beyond the grid collapses"""
    import copy
    d, p = ms.data(cus), ms.plan(cus)
    g = p.grid(ms.KIND["box"])
    right = ms.answer(shares(cus, "box"), p.zero_step)
    slipped = copy.copy(d)
    slipped.lo, slipped.hi = np.roll(d.lo, -g, axis=0), np.roll(d.hi, -g, axis=0)
    assert ms.answer(ms.shares(slipped, "box"), p.zero_step)[0] < right[0] // 2
    # and the changed table of the GPU test changes the answer of segment S - 2 alone
    ch = d.changed(p.S - 2)
    for name in ("box", "polygon"):
        a, b = shares(cus, name), ms.shares(ch, name) if name == "box" else None
        if name == "polygon":
            assert ms.polygon_segment(ch, p.S - 2) != a[p.S - 2, 0] > 0
        else:
            diff = np.flatnonzero((a != b).any(axis=1))
            assert diff.tolist() == [p.S - 2] and b[p.S - 2, 0] > 0
