"""The collector model of _collector_model.py against the oracle's own searches, and the coverage of the committed
scenarios (no GPU).

The first pins the model's numpy selection and its record layout to the oracle — not to the code under test: one LAST and
one LAS image through the oracle's file searches into a count, a buffer and a grid collector, and the model's answer for
the same single scan, byte for byte.  The second computes, from the operation lists of the committed seeds alone, what
test_gpu_collector_lifecycle.py is there to reach; a condition that fails means the generator is too narrow.
"""
import numpy as np
import pytest

import _collector_model as cm

BOX = ((30.0, 20.0, 5.0), (90.0, 100.0, 25.0))


@pytest.mark.parametrize("layout", ["last", "las"])
def test_model_agrees_with_the_oracle_searches(oracle, layout):
    rng = np.random.default_rng(5)
    ds = cm.make_dataset(rng, "d", 20_011, cm.SCALES[2], cm.OFFSETS[2], layout=layout, colour=True)
    image = ds.image()
    lmin, lmax = oracle.box_to_local(BOX[0], BOX[1], list(ds.scale), list(ds.offset))
    t0, t1 = float(ds.t[3000]), float(ds.t[9000])
    searches = [
        ({"kind": "BOUNDS", "lmin": lmin, "lmax": lmax},
         (lambda c: oracle.search_last_bounds(image, BOX[0], BOX[1], c)) if layout == "last" else (lambda c: oracle.search_las_bounds(image, BOX[0], BOX[1], c)[0])),
        ({"kind": "CLASS", "cls": 6},
         (lambda c: oracle.search_last_class(image, 6, c)) if layout == "last" else (lambda c: oracle.search_las_class(image, 6, c))),
        ({"kind": "TIME", "start": t0, "end": t1}, lambda c: oracle.search_time(image, layout, t0, t1, c)),
        ({"kind": "BOUNDS_CLASS", "lmin": lmin, "lmax": lmax, "cls": 2}, lambda c: oracle.search_bounds_class(image, layout, BOX[0], BOX[1], 2, c)),
        ({"kind": "BOUNDS_TIME", "lmin": lmin, "lmax": lmax, "start": t0, "end": t1},
         lambda c: oracle.search_bounds_time(image, layout, BOX[0], BOX[1], t0, t1, c)),
    ]
    for p, search in searches:
        sel = cm.select(ds, p)
        assert 100 < int(sel.sum()) < ds.n, p
        recs = cm.records(ds, p, sel, True)
        for kind in ("count", "buffer", "grid"):
            oc = {"count": oracle.count_collector, "buffer": oracle.buffer_collector,
                  "grid": lambda: oracle.grid_collector(cm.GRID_BOX[0], cm.GRID_BOX[1], 1.0)}[kind]()
            model = cm.Model(oracle, kind, 1.0)
            try:
                assert search(oc) == 0, (p, oracle.err())
                model.scan(recs)
                assert model.point_count() == oc.point_count(), (p, kind)
                assert model.points().tobytes() == oc.points().tobytes(), (p, kind)
                if kind == "grid":
                    assert np.array_equal(model.og.grid_cells(), oc.grid_cells()) and model.og.grid_params() == oc.grid_params()
                    assert 0 < oc.point_count() < len(recs)  # (cells shared by several matches: the grid's rule decided)
            finally:
                oc.free()
                model.free()


def test_world_space_box_selects_what_the_integer_box_selects():
    """BOUNDS_F64 has no oracle search over LAS / LAST images: on a grid of exactly representable positions (scale 1/128) it
    must select what the integer box with the same faces selects."""
    rng = np.random.default_rng(6)
    ds = cm.make_dataset(rng, "d", 10_007, cm.SCALES[0], cm.OFFSETS[0])
    lmin, lmax = [2000, 3000, 500], [9000, 12000, 3000]
    a = cm.select(ds, {"kind": "BOUNDS", "lmin": lmin, "lmax": lmax})
    b = cm.select(ds, {"kind": "BOUNDS_F64", "wmin": [v / 128 for v in lmin], "wmax": [v / 128 for v in lmax]})
    assert np.array_equal(a, b) and 100 < int(a.sum()) < ds.n


@pytest.fixture(scope="module")
def coverage():
    total = {"combos": {}, "events": [], "recreate": set(), "phase": set(), "growths": [], "fold_mixed": 0, "recut": set(),
             "grid_caller_read": 0, "tuple_bytes": set(), "indexed_repeat": 0, "writers": set()}
    scenarios = []
    for seed in cm.SEEDS:
        datasets, ops = cm.scenario(seed)
        scenarios.append((datasets, ops))
        run = cm.ModelRun(None, datasets)
        for op in ops:
            run.apply(op)
        run.finish()
        for k, v in run.cov.items():
            if isinstance(v, dict):
                for kk, n in v.items():
                    total[k][kk] = total[k].get(kk, 0) + n
            elif isinstance(v, set):
                total[k] |= v
            else:
                total[k] += v
    return total, scenarios


def test_scenarios_are_deterministic_and_sized(coverage):
    _, scenarios = coverage
    assert len(cm.SEEDS) >= 30
    for seed, (datasets, ops) in zip(cm.SEEDS, scenarios):
        again_d, again = cm.scenario(seed)
        assert repr(again) == repr(ops) and [repr(d) for d in again_d] == [repr(d) for d in datasets], seed
        assert all(np.array_equal(a.xyz, b.xyz) and a.t.tobytes() == b.t.tobytes() for a, b in zip(datasets, again_d)), seed
        assert 20 <= len(ops) <= 40 and 3 <= len(datasets) <= 5, (seed, len(ops), len(datasets))
        live = set()
        for op in ops:  # at most four collectors alive, every operation on a live one
            if op["op"] == "new":
                assert op["slot"] not in live
                live.add(op["slot"])
            elif op["op"] == "free":
                live.remove(op["slot"])
            elif "slot" in op:
                assert op["slot"] in live
            assert len(live) <= 4


def test_datasets_cover_the_sizes_phases_and_layouts(coverage):
    _, scenarios = coverage
    ds = [d for datasets, _ in scenarios for d in datasets]
    assert {d.n for d in ds} >= set(cm.SIZES)
    last = [d for d in ds if d.layout == "last"]
    assert {d.xyz_phase for d in last} >= {0, 4, 8, 12, 2, 6} and {d.t_phase for d in last} == {0, 8}
    assert {d.colour for d in last} == {True, False} and {d.colour for d in ds if d.layout == "las"} == {True, False}
    assert {d.xyz_phase % 2 for d in ds if d.layout == "las"} == {0, 1}
    assert {d.times for d in ds} == {"ordinary", "adversarial"}
    assert len({(d.scale, d.offset) for d in ds}) >= 8
    for datasets, _ in scenarios:
        assert len({(d.scale, d.offset) for d in datasets}) >= 3              # grid entries differ within a scenario
        assert any(np.all(np.diff(d.xyz[:, 0]) >= 0) and d.n > 2048 for d in datasets)  # one sorted by x
        assert sum(d.layout == "las" for d in datasets) == 1


def test_every_accepted_combination_runs_at_least_twice(coverage):
    cov, _ = coverage
    missing = {c: cov["combos"].get(c, 0) for c in cm.COMBOS if cov["combos"].get(c, 0) < 2}
    assert not missing, missing
    assert set(cov["combos"]) <= set(cm.COMBOS)


def test_every_collector_kind_is_read_reset_and_recreated_mid_life(coverage):
    cov, _ = coverage
    seq = cm.sequences(cov)
    kinds = set(cm.COLLECTORS)
    assert seq["read_scan_read"] == kinds, seq    # a read, further scans, a second read
    assert seq["reset_scan_read"] == kinds, seq   # a reset, scans, a read
    assert cov["recreate"] == kinds, cov["recreate"]  # freed and created again while another collector holds data


def test_buffers_append_at_every_record_phase_and_grow(coverage):
    cov, _ = coverage
    want = {(h, w) for h in range(16) for w in ("dense", "parked", "sparse")}
    assert cov["phase"] >= want, sorted(want - cov["phase"])
    grown = [g for g in cov["growths"] if g["from"] >= 4096]
    assert len(grown) >= 3 and any(g["overestimated"] for g in grown), cov["growths"]
    assert any(not g["overestimated"] for g in grown)


def test_grids_fold_mixed_runs_onto_winners_of_another_fanout(coverage):
    cov, _ = coverage
    assert cov["tuple_bytes"] == {16, 24}
    assert cov["fold_mixed"] >= 1                 # one fold: both tuple widths, more than one entry
    assert cov["recut"] >= {(1, 7), (7, 1)}, cov["recut"]  # winners of another second-level fan-out than the fold's, both ways
    assert cov["grid_caller_read"] >= 1           # a scan on a caller's stream, then a read with no wait in between
    assert cov["indexed_repeat"] >= 1             # an indexed query repeated on an index that exists


def test_options_take_every_value(coverage):
    _, scenarios = coverage
    seen = {}
    for _, ops in scenarios:
        for op in ops:
            if op["op"] == "set_option":
                seen.setdefault(op["key"], set()).add(op["value"])
    assert seen == {k: set(v) for k, v in cm.OPTION_VALUES.items()}, seen
