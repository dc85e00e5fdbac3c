"""The canopy-height raster: the libpcq entry (include/pcq.h: pcq_scan_dev_zrange_raster_batch_classes) and the host entry
(include/pcq_query_canopy.h: pcq_query_resident_bounds_canopy_raster) are declared and exported beside the old entries, the binding
has the method, the ABI number is what it was, the four older host headers keep their declarations, query_binding.canopy_sig is held
to pcq_query_canopy.h the way test_zsum_classes_abi.py holds classes_sig to its header, and the host entry makes its argument checks,
in the height raster's order with the two null sets among the null arguments, before any device is touched — from python, and from a
stand-alone driver built with ASan and UBSan (tests/native/canopy_asan_driver.cpp).  No GPU call."""
import ctypes as C
import importlib
import os
import re

import _host

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
qb = importlib.import_module("adhoc-queries-pointclouds_amd.query_binding")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "adhoc-queries-pointclouds_amd")
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
LIB_OLD = ["pcq_scan_dev_count_batch", "pcq_scan_dev_count_batch_combined", "pcq_scan_dev_count_batch_bounds_time",
           "pcq_scan_dev_count_batch_multi", "pcq_scan_dev_class_hist_batch", "pcq_scan_dev_time_hist_batch", "pcq_scan_dev_raster_batch",
           "pcq_scan_dev_zrange_raster_batch", "pcq_scan_dev_zsum_raster_batch", "pcq_scan_dev_zsum_raster_batch_classes",
           "pcq_scan_dev_zmoments_raster_batch", "pcq_scan_dev_count_batch_polygon"]
QUERY_OLD = ["pcq_query_resident_count_bounds", "pcq_query_resident_count_bounds_class", "pcq_query_resident_count_bounds_time",
             "pcq_query_resident_count_bounds_many", "pcq_query_resident_count_bounds_by_class", "pcq_query_resident_count_bounds_by_time",
             "pcq_query_resident_count_bounds_raster", "pcq_query_resident_bounds_zrange_raster", "pcq_query_resident_count_polygon",
             "pcq_query_resident_bounds_zmean_raster", "pcq_query_resident_bounds_zmean_raster_classes", "pcq_query_resident_bounds_zstd_raster"]
OLDER = {"pcq_query_stats.h": ["pcq_query_resident_bounds_zmean_raster"], "pcq_query_classes.h": ["pcq_query_resident_bounds_zmean_raster_classes"],
         "pcq_query_moments.h": ["pcq_query_resident_bounds_zstd_raster"]}
DEV = "pcq_scan_dev_zrange_raster_batch_classes"
NEW = "pcq_query_resident_bounds_canopy_raster"


def test_both_entries_are_declared_and_exported_beside_the_old_ones():
    declared = pkg.declared_symbols(["pcq.h"])
    exported = pkg.exported_symbols(pkg.lib_path())
    for name in [DEV] + LIB_OLD:
        assert name in declared, name
        assert name in exported, name
    old = pkg.declared_symbols(["pcq_query.h"])
    assert len(old) == 46 and len(set(old)) == 46 and NEW not in old
    for header, names in OLDER.items():
        assert pkg.declared_symbols([header]) == names, header
    assert pkg.declared_symbols(["pcq_query_canopy.h"]) == [NEW]
    exported = pkg.exported_symbols(os.path.join(PKG, "libpcq_query.so"))
    for name in [NEW] + QUERY_OLD:
        assert name in exported, name
    with open(os.path.join(ROOT, "include", "pcq.h")) as f:
        text = f.read()
    assert "#define PCQ_ZRANGE_CLASSES_CELLS_MAX 4096" in text and "#define PCQ_ZRANGE_CELLS_MAX 4096" in text


def test_abi_number_is_unchanged_and_the_binding_has_the_method():
    assert pkg.load_library().pcq_abi_version() == 6
    assert callable(binding.Context.scan_dev_zrange_raster_batch_classes)
    assert callable(binding.Context.scan_dev_zsum_raster_batch_classes) and callable(binding.Context.scan_dev_zrange_raster_batch)
    u32, vp = C.c_uint32, C.c_void_p
    fn = getattr(pkg.load_library(), DEV)
    assert fn.restype is C.c_int and list(fn.argtypes) == [vp, C.POINTER(binding.Columns), C.POINTER(binding.Predicate), C.POINTER(u32), C.c_size_t,
                                                          u32, u32, C.POINTER(u32), C.POINTER(u32), vp, vp, vp]


def test_the_canopy_table_is_its_header():
    """names, the prototype's number of parameters, and argtypes on the loaded library; the older tables keep to their headers"""
    assert sorted(qb.canopy_sig) == sorted(pkg.declared_symbols(["pcq_query_canopy.h"])) == [NEW]
    assert sorted(qb.sig) == sorted(pkg.declared_symbols(["pcq_query.h"])) and len(qb.sig) == 46
    for table, header in ((qb.stats_sig, "pcq_query_stats.h"), (qb.classes_sig, "pcq_query_classes.h"), (qb.moments_sig, "pcq_query_moments.h")):
        assert sorted(table) == OLDER[header] and not set(table) & set(qb.canopy_sig)
    assert not set(qb.sig) & set(qb.canopy_sig)
    text = open(os.path.join(ROOT, "include", "pcq_query_canopy.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(pcq_query_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", text)
    assert [name for name, _ in protos] == [NEW]
    assert protos[0][1].count(",") + 1 == 12 == len(qb.canopy_sig[NEW][1])  # (no nested parentheses or brackets with commas in it)
    lib = pkg.load_query_library()
    for name, (res, args) in (list(qb.canopy_sig.items()) + list(qb.moments_sig.items()) + list(qb.classes_sig.items()) +
                              list(qb.stats_sig.items()) + list(qb.sig.items())):
        fn = getattr(lib, name)
        assert res is not None and fn.restype is res and list(fn.argtypes) == list(args), name
    u64, dbl, pd, pu32 = C.c_uint64, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    assert qb.canopy_sig[NEW] == (C.c_int, [C.c_void_p, pd, dbl, dbl, u64, u64, pu32, pu32, pd, pd, pd, C.POINTER(u64)])


def test_host_entry_checks_its_arguments_without_a_device():
    """every case and the order of the height raster's checks, plus the two null sets; height and points_scanned may be null — for
    the canopy pair, each set empty, both empty and both full"""
    lib = pkg.load_query_library()
    f = lib.pcq_query_resident_bounds_canopy_raster
    dummy = C.c_void_p(1)  # never dereferenced: a check refuses first
    lo = (C.c_double * 3)(0, 0, 0)
    s_g, s_s, s_h = [-3.25 - c for c in range(64)], [1000.5 + 7 * c for c in range(64)], [0.125 * c for c in range(64)]
    zg, zs, h = (C.c_double * 64)(*s_g), (C.c_double * 64)(*s_s), (C.c_double * 64)(*s_h)
    s = C.c_uint64(15)
    inf, nan = float("inf"), float("nan")
    but = [c for c in range(256) if c not in (7, 18)]

    def same():
        return list(zg) == s_g and list(zs) == s_s and list(h) == s_h and s.value == 15

    for low, high in (((2,), but), ((), but), ((2,), ()), ((), ()), (range(256), range(256))):
        g, u = (C.c_uint32 * 8)(*binding.class_set_words(low)), (C.c_uint32 * 8)(*binding.class_set_words(high))
        for args, text in (((None, lo, 10.0, 1.0, 8, 8, g, u, zg, zs), b"null argument"), ((dummy, None, 10.0, 1.0, 8, 8, g, u, zg, zs), b"null argument"),
                           ((dummy, lo, 10.0, 1.0, 8, 8, None, u, zg, zs), b"null argument"), ((dummy, lo, 10.0, 1.0, 8, 8, g, None, zg, zs), b"null argument"),
                           ((dummy, lo, 10.0, 1.0, 8, 8, g, u, None, zs), b"null argument"), ((dummy, lo, 10.0, 1.0, 8, 8, g, u, zg, None), b"null argument"),
                           ((None, None, 10.0, 1.0, 0, 0, None, None, None, None), b"null argument"),
                           ((dummy, lo, 10.0, 1.0, 1025, 1024, g, u, zg, zs), b"cells"), ((dummy, lo, 10.0, 1.0, 2**20 + 1, 1, g, u, zg, zs), b"cells"),
                           ((dummy, lo, 10.0, 1.0, 2**32, 2**32, g, u, zg, zs), b"cells"),
                           ((dummy, lo, 10.0, 1.0, 2**64 - 1, 2**64 - 1, g, u, zg, zs), b"cells"),
                           ((dummy, lo, 10.0, 0.0, 8, 8, g, u, zg, zs), b"cell_size"), ((dummy, lo, 10.0, -0.5, 8, 8, g, u, zg, zs), b"cell_size"),
                           ((dummy, lo, 10.0, inf, 8, 8, g, u, zg, zs), b"cell_size"), ((dummy, lo, 10.0, nan, 8, 8, g, u, zg, zs), b"cell_size")):
            for height in (h, None):
                for scanned in (C.byref(s), None):
                    assert f(*args, height, scanned) == PCQ_ERR_ARG, args
                    assert text in lib.pcq_query_last_error(), (args, lib.pcq_query_last_error())
                    assert same()
        # a null output or a null set comes before the number of cells, the number of cells before the cell size
        for args in ((g, u, None, zs), (g, u, zg, None), (None, u, zg, zs), (g, None, zg, zs)):
            assert f(dummy, lo, 10.0, nan, 2**32, 2**32, *args, h, None) == PCQ_ERR_ARG and b"null argument" in lib.pcq_query_last_error()
        assert f(dummy, lo, 10.0, nan, 0, 0, None, u, zg, zs, h, None) == PCQ_ERR_ARG and b"null argument" in lib.pcq_query_last_error()
        assert f(dummy, lo, 10.0, nan, 2**32, 2**32, g, u, zg, zs, h, None) == PCQ_ERR_ARG and b"cells" in lib.pcq_query_last_error()
        # nx * ny == 0 comes before the cell size and the number of cells: PCQ_OK, nothing written
        for nx, ny in ((0, 8), (8, 0), (0, 0), (0, 2**64 - 1)):
            assert f(dummy, lo, 10.0, nan, nx, ny, g, u, zg, zs, h, C.byref(s)) == 0
            assert same()


def test_host_entry_under_address_sanitizer(tmp_path):
    """The argument checks of the new host entry under ASan + UBSan, through a stand-alone program with its own main (nothing
    sanitized is loaded into python; no device is touched), built the way test_zsum_classes_abi.py builds its driver: capi.cpp and
    resident.cpp sanitized into the program, the rest of the host layer from the libpcq_query.so beside them."""
    host = os.path.join(PKG, "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "native", "canopy_asan_driver.cpp"),
           os.path.join(host, "capi.cpp"), os.path.join(host, "resident.cpp"), "-L" + PKG, "-lpcq_query", "-lpcq", "-Wl,-rpath," + PKG]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    assert _host.build_and_run(tmp_path, "canopy_asan", cmd, env) == ["ok", "380", "20"]
