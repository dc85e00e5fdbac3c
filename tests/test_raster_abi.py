"""The density raster of a box: the libpcq entry (include/pcq.h: pcq_scan_dev_raster_batch) and the host entry
(include/pcq_query.h: pcq_query_resident_count_bounds_raster) are declared and exported beside the old batch entries with their two
limits, the binding has the method, the ABI number is what it was, and the host entry makes its argument checks before any device
is touched — from python, and from a stand-alone driver built with ASan and UBSan (tests/native/raster_asan_driver.cpp).  The
division the kernel bins with (csrc/raster_div.h) is checked against `/` as host code (tests/native/raster_div_driver.cpp).  No GPU
call."""
import ctypes as C
import importlib
import os

import _host

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "adhoc-queries-pointclouds_amd")
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
LIB_OLD = ["pcq_scan_dev_count_batch", "pcq_scan_dev_count_batch_combined", "pcq_scan_dev_count_batch_bounds_time",
           "pcq_scan_dev_count_batch_multi", "pcq_scan_dev_class_hist_batch", "pcq_scan_dev_time_hist_batch"]
QUERY_OLD = ["pcq_query_resident_count_bounds", "pcq_query_resident_count_bounds_class", "pcq_query_resident_count_bounds_time",
             "pcq_query_resident_count_bounds_many", "pcq_query_resident_count_bounds_by_class", "pcq_query_resident_count_bounds_by_time"]


def test_both_entries_are_declared_and_exported_beside_the_old_ones():
    declared = pkg.declared_symbols(["pcq.h"])
    exported = pkg.exported_symbols(pkg.lib_path())
    for name in ["pcq_scan_dev_raster_batch"] + LIB_OLD:
        assert name in declared, name
        assert name in exported, name
    declared = pkg.declared_symbols(["pcq_query.h"])
    exported = pkg.exported_symbols(os.path.join(PKG, "libpcq_query.so"))
    for name in ["pcq_query_resident_count_bounds_raster"] + QUERY_OLD:
        assert name in declared, name
        assert name in exported, name
    with open(os.path.join(ROOT, "include", "pcq.h")) as f:
        assert "#define PCQ_RASTER_CELLS_MAX 8192" in f.read()
    with open(os.path.join(ROOT, "include", "pcq_query.h")) as f:
        assert "#define PCQ_QUERY_RASTER_CELLS_MAX (1u << 20)" in f.read()


def test_abi_number_is_unchanged_and_the_binding_has_the_method():
    assert pkg.load_library().pcq_abi_version() == 6
    binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
    assert callable(binding.Context.scan_dev_raster_batch)
    assert callable(binding.Context.scan_dev_class_hist_batch) and callable(binding.Context.scan_dev_time_hist_batch)


def test_host_entry_checks_its_arguments_without_a_device():
    lib = pkg.load_query_library()
    f = lib.pcq_query_resident_count_bounds_raster
    dummy = C.c_void_p(1)  # never dereferenced: a check refuses first
    lo = (C.c_double * 3)(0, 0, 0)
    sentinel = [1000 + 7 * c for c in range(64)]
    words = (C.c_uint64 * 64)(*sentinel)
    s = C.c_uint64(15)
    inf, nan = float("inf"), float("nan")
    for args, text in (((None, lo, 10.0, 1.0, 8, 8, words), b"null argument"), ((dummy, None, 10.0, 1.0, 8, 8, words), b"null argument"),
                       ((dummy, lo, 10.0, 1.0, 8, 8, None), b"null argument"), ((None, None, 10.0, 1.0, 0, 0, None), b"null argument"),
                       ((dummy, lo, 10.0, 1.0, 1025, 1024, words), b"cells"), ((dummy, lo, 10.0, 1.0, 2**20 + 1, 1, words), b"cells"),
                       ((dummy, lo, 10.0, 1.0, 2**32, 2**32, words), b"cells"), ((dummy, lo, 10.0, 1.0, 2**64 - 1, 2**64 - 1, words), b"cells"),
                       ((dummy, lo, 10.0, 0.0, 8, 8, words), b"cell_size"), ((dummy, lo, 10.0, -0.5, 8, 8, words), b"cell_size"),
                       ((dummy, lo, 10.0, inf, 8, 8, words), b"cell_size"), ((dummy, lo, 10.0, nan, 8, 8, words), b"cell_size")):
        for scanned in (C.byref(s), None):
            assert f(*args, scanned) == PCQ_ERR_ARG, args
            assert text in lib.pcq_query_last_error(), (args, lib.pcq_query_last_error())
            assert list(words) == sentinel and s.value == 15
    # nx * ny == 0 comes before the cell size and the number of cells: PCQ_OK, nothing written
    for nx, ny in ((0, 8), (8, 0), (0, 0), (0, 2**64 - 1)):
        assert f(dummy, lo, 10.0, nan, nx, ny, words, C.byref(s)) == 0
        assert list(words) == sentinel and s.value == 15


def test_host_entry_under_address_sanitizer(tmp_path):
    """The argument checks of the new host entry under ASan + UBSan, through a stand-alone program (nothing sanitized is loaded
    into python; no device is touched).  The two translation units the entry lives in — capi.cpp and resident.cpp — are built
    sanitized into the program, where their definitions come first; the rest of the host layer is the libpcq_query.so beside
    them, which keeps the build to a few seconds."""
    host = os.path.join(PKG, "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "native", "raster_asan_driver.cpp"),
           os.path.join(host, "capi.cpp"), os.path.join(host, "resident.cpp"), "-L" + PKG, "-lpcq_query", "-lpcq", "-Wl,-rpath," + PKG]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    assert _host.build_and_run(tmp_path, "raster_asan", cmd, env) == ["ok", "28", "4"]


def test_division_against_the_operator(tmp_path):
    """raster_div.h as host code under UBSan: the listed divisors with every quotient below 8192 at its edges, and 10^6 random pairs"""
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "native", "raster_div_driver.cpp")]
    out = _host.build_and_run(tmp_path, "raster_div", cmd, dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert out[0] == "ok" and int(out[1]) > 1_000_000 + 12 * 8192
