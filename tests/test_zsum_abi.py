"""The mean-height raster of a box: the libpcq entry (include/pcq.h: pcq_scan_dev_zsum_raster_batch) and the host entry
(include/pcq_query_stats.h: pcq_query_resident_bounds_zmean_raster) are declared and exported beside the old entries with the launch
limit, the binding has the method, the ABI number is what it was, query_binding.stats_sig is held to pcq_query_stats.h the way
test_query_binding.py holds sig to pcq_query.h (which keeps its 46), and the host entry makes its argument checks, in the height
raster's order, before any device is touched — from python, and from a stand-alone driver built with ASan and UBSan
(tests/native/zmean_asan_driver.cpp).  host/zsum_plan.h, the cut of a z lattice's files into launches of fewer than 2^32 points, runs
under the same sanitizers with small limits (tests/native/zsum_plan_driver.cpp).  No GPU call."""
import ctypes as C
import importlib
import os
import re

import _host

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
qb = importlib.import_module("adhoc-queries-pointclouds_amd.query_binding")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "adhoc-queries-pointclouds_amd")
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
LIB_OLD = ["pcq_scan_dev_count_batch", "pcq_scan_dev_count_batch_combined", "pcq_scan_dev_count_batch_bounds_time",
           "pcq_scan_dev_count_batch_multi", "pcq_scan_dev_class_hist_batch", "pcq_scan_dev_time_hist_batch", "pcq_scan_dev_raster_batch",
           "pcq_scan_dev_zrange_raster_batch", "pcq_scan_dev_count_batch_polygon"]
QUERY_OLD = ["pcq_query_resident_count_bounds", "pcq_query_resident_count_bounds_class", "pcq_query_resident_count_bounds_time",
             "pcq_query_resident_count_bounds_many", "pcq_query_resident_count_bounds_by_class", "pcq_query_resident_count_bounds_by_time",
             "pcq_query_resident_count_bounds_raster", "pcq_query_resident_bounds_zrange_raster", "pcq_query_resident_count_polygon"]
NEW = "pcq_query_resident_bounds_zmean_raster"


def test_both_entries_are_declared_and_exported_beside_the_old_ones():
    declared = pkg.declared_symbols(["pcq.h"])
    exported = pkg.exported_symbols(pkg.lib_path())
    for name in ["pcq_scan_dev_zsum_raster_batch"] + LIB_OLD:
        assert name in declared, name
        assert name in exported, name
    old = pkg.declared_symbols(["pcq_query.h"])
    assert len(old) == 46 and len(set(old)) == 46 and NEW not in old
    assert pkg.declared_symbols(["pcq_query_stats.h"]) == [NEW]
    exported = pkg.exported_symbols(os.path.join(PKG, "libpcq_query.so"))
    for name in [NEW] + QUERY_OLD:
        assert name in exported, name
    with open(os.path.join(ROOT, "include", "pcq.h")) as f:
        text = f.read()
    assert "#define PCQ_ZSUM_CELLS_MAX 2048" in text and "#define PCQ_ZRANGE_CELLS_MAX 4096" in text and "#define PCQ_RASTER_CELLS_MAX 8192" in text
    with open(os.path.join(ROOT, "include", "pcq_query_stats.h")) as f:
        assert '#include "pcq_query.h"' in f.read()


def test_abi_number_is_unchanged_and_the_binding_has_the_method():
    assert pkg.load_library().pcq_abi_version() == 6
    binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
    assert callable(binding.Context.scan_dev_zsum_raster_batch)
    assert callable(binding.Context.scan_dev_zrange_raster_batch) and callable(binding.Context.scan_dev_raster_batch)


def test_the_stats_table_is_its_header():
    """names, the prototype's number of parameters, and argtypes on the loaded library; sig keeps to pcq_query.h"""
    assert sorted(qb.stats_sig) == sorted(pkg.declared_symbols(["pcq_query_stats.h"])) == [NEW]
    assert sorted(qb.sig) == sorted(pkg.declared_symbols(["pcq_query.h"])) and len(qb.sig) == 46 and not set(qb.sig) & set(qb.stats_sig)
    text = open(os.path.join(ROOT, "include", "pcq_query_stats.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(pcq_query_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", text)
    assert [name for name, _ in protos] == [NEW]
    assert protos[0][1].count(",") + 1 == 9 == len(qb.stats_sig[NEW][1])  # (no nested parentheses or brackets with commas in it)
    lib = pkg.load_query_library()
    for name, (res, args) in list(qb.stats_sig.items()) + list(qb.sig.items()):
        fn = getattr(lib, name)
        assert res is not None and fn.restype is res and list(fn.argtypes) == list(args), name
    u64, dbl = C.c_uint64, C.c_double
    assert qb.stats_sig[NEW] == (C.c_int, [C.c_void_p, C.POINTER(dbl), dbl, dbl, u64, u64, C.POINTER(u64), C.POINTER(dbl), C.POINTER(u64)])


def test_host_entry_checks_its_arguments_without_a_device():
    lib = pkg.load_query_library()
    f = lib.pcq_query_resident_bounds_zmean_raster
    dummy = C.c_void_p(1)  # never dereferenced: a check refuses first
    lo = (C.c_double * 3)(0, 0, 0)
    s_cnt, s_mean = [1000 + 7 * c for c in range(64)], [-3.25 - c for c in range(64)]
    cnt, mean = (C.c_uint64 * 64)(*s_cnt), (C.c_double * 64)(*s_mean)
    s = C.c_uint64(15)
    inf, nan = float("inf"), float("nan")
    for args, text in (((None, lo, 10.0, 1.0, 8, 8, cnt, mean), b"null argument"), ((dummy, None, 10.0, 1.0, 8, 8, cnt, mean), b"null argument"),
                       ((dummy, lo, 10.0, 1.0, 8, 8, None, mean), b"null argument"), ((dummy, lo, 10.0, 1.0, 8, 8, cnt, None), b"null argument"),
                       ((None, None, 10.0, 1.0, 0, 0, None, None), b"null argument"),
                       ((dummy, lo, 10.0, 1.0, 1025, 1024, cnt, mean), b"cells"), ((dummy, lo, 10.0, 1.0, 2**20 + 1, 1, cnt, mean), b"cells"),
                       ((dummy, lo, 10.0, 1.0, 2**32, 2**32, cnt, mean), b"cells"), ((dummy, lo, 10.0, 1.0, 2**64 - 1, 2**64 - 1, cnt, mean), b"cells"),
                       ((dummy, lo, 10.0, 0.0, 8, 8, cnt, mean), b"cell_size"), ((dummy, lo, 10.0, -0.5, 8, 8, cnt, mean), b"cell_size"),
                       ((dummy, lo, 10.0, inf, 8, 8, cnt, mean), b"cell_size"), ((dummy, lo, 10.0, nan, 8, 8, cnt, mean), b"cell_size")):
        for scanned in (C.byref(s), None):
            assert f(*args, scanned) == PCQ_ERR_ARG, args
            assert text in lib.pcq_query_last_error(), (args, lib.pcq_query_last_error())
            assert list(cnt) == s_cnt and list(mean) == s_mean and s.value == 15
    # a null output comes before the number of cells, the number of cells before the cell size
    assert f(dummy, lo, 10.0, nan, 2**32, 2**32, None, mean, None) == PCQ_ERR_ARG and b"null argument" in lib.pcq_query_last_error()
    assert f(dummy, lo, 10.0, nan, 2**32, 2**32, cnt, mean, None) == PCQ_ERR_ARG and b"cells" in lib.pcq_query_last_error()
    # nx * ny == 0 comes before the cell size and the number of cells: PCQ_OK, nothing written
    for nx, ny in ((0, 8), (8, 0), (0, 0), (0, 2**64 - 1)):
        assert f(dummy, lo, 10.0, nan, nx, ny, cnt, mean, C.byref(s)) == 0
        assert list(cnt) == s_cnt and list(mean) == s_mean and s.value == 15


def test_host_entry_under_address_sanitizer(tmp_path):
    """The argument checks of the new host entry under ASan + UBSan, through a stand-alone program (nothing sanitized is loaded
    into python; no device is touched).  The two translation units the entry lives in — capi.cpp and resident.cpp — are built
    sanitized into the program, where their definitions come first; the rest of the host layer is the libpcq_query.so beside
    them, which keeps the build to a few seconds."""
    host = os.path.join(PKG, "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "native", "zmean_asan_driver.cpp"),
           os.path.join(host, "capi.cpp"), os.path.join(host, "resident.cpp"), "-L" + PKG, "-lpcq_query", "-lpcq", "-Wl,-rpath," + PKG]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    assert _host.build_and_run(tmp_path, "zmean_asan", cmd, env) == ["ok", "30", "4"]


def test_zsum_plan_under_address_sanitizer(tmp_path):
    """host/zsum_plan.h with small limits under ASan + UBSan, through a stand-alone program: an empty list, one file, totals at
    limit - 1 and at the limit, a file that alone reaches the limit (refused, with its position), many files; every batch's total
    below the limit, file order kept, no file lost — and the product's limit with totals a u64 could not hold."""
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
           "-I" + os.path.join(PKG, "host"), os.path.join(ROOT, "tests", "native", "zsum_plan_driver.cpp")]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    assert _host.build_and_run(tmp_path, "zsum_plan", cmd, env) == ["ok", "1702"]
