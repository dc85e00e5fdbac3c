"""Box AND time on resident datasets: the two libpcq entries (include/pcq.h) and the two host entries (include/pcq_query.h) are
declared and exported beside the old ones, the binding has their methods, the ABI number is what it was, the host entries refuse
null arguments before any device is touched, and the numpy model of the chunk states that the GPU tests compare the statistics
with (tests/_bounds_time_index_model.py) agrees with a brute-force selection.  No GPU call."""
import ctypes as C
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import _bounds_time_index_model as bm  # noqa: E402

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "adhoc-queries-pointclouds_amd")
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
LIB_NEW = ["pcq_scan_dev_count_batch_bounds_time", "pcq_scan_dev_indexed_bounds_time"]
QUERY_NEW = ["pcq_query_resident_count_bounds_time", "pcq_query_resident_search_bounds_time"]
LIB_OLD = ["pcq_scan_dev_count_batch", "pcq_scan_dev_count_batch_combined", "pcq_scan_dev_indexed", "pcq_scan_dev_indexed_combined",
           "pcq_scan_dev_indexed_time"]


def test_the_four_entries_are_declared_and_exported():
    declared = pkg.declared_symbols(["pcq.h"])
    exported = pkg.exported_symbols(pkg.lib_path())
    for name in LIB_NEW + LIB_OLD:
        assert name in declared, name
        assert name in exported, name
    declared = pkg.declared_symbols(["pcq_query.h"])
    exported = pkg.exported_symbols(os.path.join(PKG, "libpcq_query.so"))
    for name in QUERY_NEW + ["pcq_query_resident_count_bounds_class", "pcq_query_resident_search_time"]:
        assert name in declared, name
        assert name in exported, name


def test_abi_number_is_unchanged_and_the_binding_has_the_methods():
    assert pkg.load_library().pcq_abi_version() == 6
    binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
    assert callable(binding.Context.scan_dev_count_batch_bounds_time)
    assert callable(binding.Context.scan_dev_indexed_bounds_time)


def test_host_entries_refuse_null_arguments_without_a_device():
    lib = pkg.load_query_library()
    d3 = C.c_double * 3
    dummy = C.c_void_p(1)  # never dereferenced: another argument is null
    lo, hi = d3(0.0, 0.0, 0.0), d3(1.0, 1.0, 1.0)
    m = C.c_uint64(7)
    assert lib.pcq_query_resident_count_bounds_time(None, lo, hi, 0.0, 1.0, C.byref(m), None) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_count_bounds_time(dummy, None, hi, 0.0, 1.0, C.byref(m), None) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_count_bounds_time(dummy, lo, None, 0.0, 1.0, C.byref(m), None) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_count_bounds_time(dummy, lo, hi, 0.0, 1.0, None, None) == PCQ_ERR_ARG
    assert m.value == 7
    assert b"null argument" in lib.pcq_query_last_error()
    assert lib.pcq_query_resident_search_bounds_time(None, lo, hi, 0.0, 1.0, dummy) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_search_bounds_time(dummy, None, hi, 0.0, 1.0, dummy) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_search_bounds_time(dummy, lo, None, 0.0, 1.0, dummy) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_search_bounds_time(dummy, lo, hi, 0.0, 1.0, None) == PCQ_ERR_ARG
    assert b"null argument" in lib.pcq_query_last_error()


def test_the_model_of_the_combined_states_agrees_with_a_brute_force_selection():
    rng = np.random.default_rng(5)
    lo, hi = [0, -50, -50], [999, 50, 50]
    seen = set()
    for bx in ("in", "out", "mixed"):
        for tk in ("in", "out", "mixed", "nan"):
            n = bm.CHUNK
            x = {"in": rng.integers(0, 1000, n), "out": rng.integers(2000, 3000, n), "mixed": rng.integers(500, 1500, n)}[bx]
            xyz = np.stack([x, rng.integers(-50, 51, n), rng.integers(-50, 51, n)], axis=1).astype(np.int32)
            t = {"in": rng.uniform(10.0, 20.0, n), "out": rng.uniform(30.0, 40.0, n), "mixed": rng.uniform(15.0, 25.0, n),
                 "nan": np.full(n, np.nan)}[tk]
            st = bm.states(xyz, t, lo, hi, 10.0, 20.0)[0]
            sel = bm.select(xyz, t, lo, hi, 10.0, 20.0)
            seen.add(st)
            if st == bm.NONE:
                assert not sel.any(), (bx, tk)
            if st == bm.ALL:
                assert sel.all() and (bx, tk) == ("in", "in")
            if bx == "out" or tk in ("out", "nan"):
                assert st == bm.NONE, (bx, tk)
            if "mixed" in (bx, tk) and st == bm.SCAN:
                assert 0 < int(sel.sum()) < n, (bx, tk)
    assert seen == {bm.NONE, bm.ALL, bm.SCAN}
    # the corners: a box with lo > hi, max time == end, one NaN in a contained chunk
    n = bm.CHUNK
    xyz = np.zeros((n, 3), dtype=np.int32)
    t = np.linspace(10.0, 20.0, n)
    assert bm.states(xyz, t, [0, 0, 0], [0, 0, 0], 10.0, 20.0) == [bm.SCAN]
    assert bm.states(xyz, t, [0, 0, 0], [0, 0, 0], 10.0, 20.5) == [bm.ALL]
    assert bm.states(xyz, t, [1, 0, 0], [0, 0, 0], 10.0, 20.5) == [bm.NONE]
    t[5] = np.nan
    assert bm.states(xyz, t, [0, 0, 0], [0, 0, 0], 10.0, 20.5) == [bm.SCAN]
    assert bm.classify(np.concatenate([xyz, xyz, xyz[:9]]), np.concatenate([t, t + 100.0, t[:9]]), [0, 0, 0], [0, 0, 0], 10.0, 20.5) == (1, 0, 1)
