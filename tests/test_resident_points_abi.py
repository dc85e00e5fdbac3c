"""The point and density entries of the resident dataset (include/pcq_query.h): declared, exported by libpcq_query.so, and
refusing null arguments with PCQ_ERR_ARG before any device is touched (on a machine without a GPU a device would fail with
PCQ_ERR_HIP instead).  No GPU call."""
import ctypes as C
import importlib
import os

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "adhoc-queries-pointclouds_amd")
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
NEW = ["pcq_query_resident_load_points", "pcq_query_resident_search_bounds", "pcq_query_resident_search_class",
       "pcq_query_resident_last_stats"]


def test_resident_point_entries_are_declared_and_exported():
    declared = pkg.declared_symbols(["pcq_query.h"])
    exported = pkg.exported_symbols(os.path.join(PKG, "libpcq_query.so"))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name


def test_resident_point_entries_refuse_null_arguments_without_a_device():
    lib = pkg.load_query_library()
    d3 = (C.c_double * 3)(0.0, 0.0, 0.0)
    dummy = C.c_void_p(1)  # never dereferenced: another argument is null
    h = C.c_void_p()
    one = (C.c_char_p * 1)(b"x.last")
    assert lib.pcq_query_resident_load_points(0, one, 1, None) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_load_points(0, None, 1, C.byref(h)) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_load_points(0, (C.c_char_p * 1)(None), 1, C.byref(h)) == PCQ_ERR_ARG
    assert not h.value
    assert lib.pcq_query_resident_search_bounds(None, d3, d3, dummy) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_search_bounds(dummy, None, d3, dummy) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_search_bounds(dummy, d3, None, dummy) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_search_bounds(dummy, d3, d3, None) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_search_class(None, 6, dummy) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_search_class(dummy, 6, None) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_last_stats(None, C.cast(dummy, C.POINTER(pkg.IndexStats))) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_last_stats(dummy, None) == PCQ_ERR_ARG
    assert b"null argument" in lib.pcq_query_last_error()
