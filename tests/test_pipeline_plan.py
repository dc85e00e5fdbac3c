"""The plans of test_gpu_pipeline_depth.py reach what they claim, for 64, 256 and 304 compute units: no GPU needed.

The launch arithmetic and the schedules are _pipeline_plan's restatement; here the planned sizes are put through it, and the
step-coded builders' properties are checked on the finished arrays, apart from the builders' own assertions.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402

FAMILIES = (pp.K1, pp.K2, pp.K3)


@pytest.mark.parametrize("cus", pp.CU_COUNTS)
@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_per_file_sizes_reach_depths_5_6_and_3_4(fam, cus):
    g = pp.full_grid(fam, cus)
    deep = pp.depth_report(pp.schedule(pp.per_file_grid(fam, cus, pp.deep_steps(g)), pp.deep_steps(g)))
    assert deep["depths"] == {6: g // 3, 5: g - g // 3}
    assert deep["both_exits_deep"] and deep["exit_a"] == 5 and deep["exit_b"] == 6
    shallow = pp.depth_report(pp.schedule(pp.per_file_grid(fam, cus, pp.shallow_steps(g)), pp.shallow_steps(g)))
    assert shallow["depths"] == {4: g - 1, 3: 1}
    assert not shallow["both_exits_deep"]


@pytest.mark.parametrize("cus", pp.CU_COUNTS)
def test_layouts_give_the_planned_steps_at_every_phase(cus):
    """The element counts the GPU tests derive from (head, steps, rest) come back out of the launch arithmetic."""
    for steps in (pp.deep_steps(4 * cus), pp.shallow_steps(4 * cus)):
        for phase in range(16):
            head = (16 - phase) % 16
            assert pp.class_layout(0x7000 + phase, head + pp.K2.step * steps + 347) == (head, 256 * steps + 21, steps)
        for phase in (0, 8):
            assert pp.time_layout(0x7000 + phase, phase // 8 + pp.K3.step * steps + 75) == (phase // 8, 256 * steps + 37, steps)
    for steps in (pp.deep_steps(3 * cus), pp.shallow_steps(3 * cus)):
        for phase in (0, 4, 8, 12):
            assert pp.k1_layout(0x7000 + phase, phase // 4 + pp.K1.step * steps + 269) == (phase // 4, 2 * steps + 1, steps)
    assert pp.class_layout(0x7003, 5) == (5, 0, 0) and pp.class_layout(0x7000, 0) == (0, 0, 0)
    assert pp.time_layout(0x7008, 1) == (1, 0, 0) and pp.k1_layout(0x700c, 2) == (2, 0, 0)
    assert pp.per_file_grid(pp.K2, cus, 7) == 8 and pp.batch_grid(pp.K1, cus, 10, 5) == 15


def batch_schedule(fam, cus):
    g = pp.full_grid(fam, cus)
    plan = pp.batch_plan(g)
    if fam is pp.K2:
        off, _ = pp.carve([pp.class_segment_bytes(s) for s in plan], [s.phase for s in plan])
        ns = [pp.class_segment_bytes(s) for s in plan]
        steps = [pp.class_layout(o, n)[2] for o, n in zip(off, ns)]
    else:
        ns = [pp.point_segment_points(s) for s in plan]
        steps = [n // pp.K1.step for n in ns]
    assert steps == [s.steps for s in plan]
    return plan, ns, pp.schedule(pp.batch_grid(fam, cus, sum(steps), len(plan)), sum(steps), steps, ns)


@pytest.mark.parametrize("cus", pp.CU_COUNTS)
@pytest.mark.parametrize("fam", (pp.K1, pp.K2), ids=lambda f: f.name)
def test_batch_plan_shows_every_crossing_kind(fam, cus):
    g = pp.full_grid(fam, cus)
    plan, ns, sch = batch_schedule(fam, cus)
    rep = pp.depth_report(sch)
    assert sch.grid == g and sch.total >= pp.deep_steps(g)
    assert min(rep["depths"]) >= 5 and rep["both_exits_deep"], rep["depths"]
    assert rep["cross_into_a"] and rep["cross_into_b"]
    assert rep["skips_stepped"] and rep["skips_zero_step"] and rep["skips_empty"], rep["skipped"]
    assert pp.EMPTY_BOX_SEGMENT in rep["skipped"] and plan[pp.EMPTY_BOX_SEGMENT].steps > 0
    assert 0 in ns and 1 in ns and all(s.steps % g for s in plan if s.steps > g // 4)
    if fam is pp.K2:  # the heads the kernel sees, clamped to n
        off, _ = pp.carve(ns, [s.phase for s in plan])
        assert sorted({pp.class_layout(o, n)[0] for o, n in zip(off, ns)}) == list(range(16))


def test_schedule_of_a_small_batch_by_hand():
    """Grid 4, segments of 3, 0 (n = 5), 0 (n = 0) and 7 steps: workgroup 2 goes 2 (segment 0), 6, (segment 3)."""
    sch = pp.schedule(4, 10, [3, 0, 0, 7], [30, 5, 0, 70])
    assert [u.tolist() for u in sch.steps] == [[0, 4, 8], [1, 5, 9], [2, 6], [3, 7]]
    assert [s.tolist() for s in sch.seg] == [[0, 3, 3], [0, 3, 3], [0, 3], [3, 3]]
    rep = pp.depth_report(sch)
    assert rep["depths"] == {3: 2, 2: 2} and rep["exit_a"] == 3 and rep["exit_b"] == 2
    assert rep["cross_into_b"] and not rep["cross_into_a"] and rep["skipped"] == {1, 2}
    assert rep["skips_zero_step"] and rep["skips_empty"] and not rep["skips_stepped"]
    assert pp.tile_begin([3, 0, 0, 7]).tolist() == [0, 3, 3, 3]


def per_step_counts(body_matches, step):
    return body_matches.reshape(-1, step).sum(axis=1)


def distinct_per_workgroup(counts_by_query, g):
    """counts_by_query[r][s]: the matches of query value r in step s, counted on the finished array."""
    for c in counts_by_query:
        for w in range(g):
            mine = c[w::g]
            mine = mine[mine > 0]
            assert len(np.unique(mine)) == len(mine), w


@pytest.mark.parametrize("cus", pp.CU_COUNTS)
def test_count_formula_is_distinct_and_fits(cus):
    for fam in FAMILIES:
        g = pp.full_grid(fam, cus)
        s = np.arange(sum(x.steps for x in pp.batch_plan(g)))
        pp.check_counts(s, pp.planted(s, g), g, 3, min(f.step for f in FAMILIES))
        pp.check_counts(s, pp.planted(s, g), g, 1, min(f.step for f in FAMILIES))
    with pytest.raises(AssertionError):
        pp.check_counts(np.arange(80), 1 + np.arange(80) % 37, 2, 1, 512)  # steps 0 and 74 of workgroup 0: both 1


def test_builders_plant_what_they_promise():
    """On the finished arrays (64 CUs): every step holds matches of its own query value alone, as many as m(s), distinct
    along each workgroup's list; head, leftover and tail hold matches; and the walked faults move the total."""
    rng = np.random.default_rng(7)
    g = pp.full_grid(pp.K2, 64)
    steps, head, rest = pp.deep_steps(g), 7, 347
    a = pp.class_file(rng, g, steps, head, rest, (2, 6, 9), (1,))
    body = a[head:head + pp.K2.step * steps]
    by_q = [per_step_counts(body == c, pp.K2.step) for c in (2, 6, 9)]
    for r in range(3):
        assert np.array_equal(by_q[r] > 0, np.arange(steps) % 3 == r)
    assert np.array_equal(by_q[0] + by_q[1] + by_q[2], pp.planted(np.arange(steps), g))
    distinct_per_workgroup(by_q, g)
    assert (a[:head] != 1).any() and (a[head + pp.K2.step * steps:-11] != 1).any() and a[-1] != 1
    assert pp.class_count(a, 1) + sum(pp.class_count(a, c) for c in (2, 6, 9)) == len(a)
    sch = pp.schedule(pp.per_file_grid(pp.K2, 64, steps), steps)
    for r in range(3):
        want = int(by_q[r].sum())
        assert pp.walk(sch, by_q[r]) == want
        assert pp.walk(sch, by_q[r], skip_b_from=4) < want and pp.walk(sch, by_q[r], eval_tail_prefetch=True) > want

    ranges = ((100.0, 200.0), (300.0, 400.0), (500.0, 600.0))
    g = pp.full_grid(pp.K3, 64)
    steps = pp.shallow_steps(g)
    t = pp.time_file(rng, g, steps, 1, 75, ranges)
    body = t[1:1 + pp.K3.step * steps]
    by_q = [per_step_counts(pp.in_range(body, a_, b_), pp.K3.step) for a_, b_ in ranges]
    assert np.array_equal(by_q[0] + by_q[1] + by_q[2], pp.planted(np.arange(steps), g))
    distinct_per_workgroup(by_q, g)
    assert np.isnan(t).any() and all((t == b_).any() and (t == a_).any() and (t == np.nextafter(b_, -np.inf)).any() for a_, b_ in ranges)
    assert pp.in_range(t[:1], -np.inf, np.inf).all() and pp.time_count(t[1 + pp.K3.step * steps:], -np.inf, np.inf) > 0

    g = pp.full_grid(pp.K1, 64)
    steps, q = pp.deep_steps(g), pp.PointQueries()
    xyz, cls, t = pp.points_file(rng, g, steps, 1, 269, q)
    lo, hi = 1, 1 + pp.K1.step * steps
    m = pp.planted(np.arange(steps), g)
    box = pp.in_box(xyz, *q.box)
    sub = [pp.in_box(xyz, *bx) for bx in q.sub]
    assert np.array_equal(sum(per_step_counts(s_[lo:hi], pp.K1.step) for s_ in sub), m)
    both_c = [box & (cls == c) for c in q.classes]
    both_t = [box & pp.in_range(t, a_, b_) for a_, b_ in q.ranges]
    for r in range(3):  # the matches of a combined query are the planted points, and they alone
        assert np.array_equal(both_c[r], sub[r]) and np.array_equal(both_t[r], sub[r])
    distinct_per_workgroup([per_step_counts(s_[lo:hi], pp.K1.step) for s_ in sub], g)
    # the background passes exactly one test: box alone about as often as class (time) alone
    rest_ = ~(sub[0] | sub[1] | sub[2])
    col_c, col_t = np.isin(cls, q.classes), sum(pp.in_range(t, a_, b_) for a_, b_ in q.ranges) > 0
    assert np.array_equal(box[rest_], ~col_c[rest_]) and np.array_equal(box[rest_], ~col_t[rest_])
    assert 0.4 < box[rest_].mean() < 0.6
    assert sub[0][:1].any() or sub[1][:1].any() or sub[2][:1].any()  # the peeled point
    assert any(s_[hi:].any() for s_ in sub)


def test_class_batch_segments_carry_their_neighbours_classes():
    """A segment's own class is planted by the GLOBAL step; its background is its neighbours' queried classes."""
    rng = np.random.default_rng(8)
    g = pp.full_grid(pp.K2, 64)
    plan = pp.batch_plan(g)
    begin = pp.tile_begin([s.steps for s in plan])
    k = 4
    seg = plan[k]
    head = (16 - seg.phase) % 16
    a = pp.class_file(rng, g, seg.steps, head, seg.rest, (10 + k,), (10 + k - 1, 10 + k + 1), first_step=int(begin[k]))
    per = per_step_counts(a[head:head + pp.K2.step * seg.steps] == 10 + k, pp.K2.step)
    assert np.array_equal(per, pp.planted(begin[k] + np.arange(seg.steps), g))
    assert pp.class_count(a, 10 + k - 1) > len(a) // 3 and pp.class_count(a, 10 + k + 1) > len(a) // 3
