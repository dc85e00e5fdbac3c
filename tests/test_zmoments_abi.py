"""The height-spread raster: the libpcq entry (include/pcq.h: pcq_scan_dev_zmoments_raster_batch) and the host entry
(include/pcq_query_moments.h: pcq_query_resident_bounds_zstd_raster) are declared and exported beside the old entries, the limit is
1024 cells and the other limits are what they were, the binding has the method, the ABI number is 6, query_binding.moments_sig is
held to pcq_query_moments.h the way the other three tables are held to their headers, and the host entry makes its argument checks
from python with a dummy handle — in the mean-height raster's order with zstd among the pointers that may not be null — before any
device is touched, leaving the three arrays and points_scanned as they were.  No GPU call.

What turns it red: a missing declaration, export, binding method or table entry; another limit; an ABI bump; a parameter added to
or taken from the prototype; a check moved before another; an output written by a refusal."""
import ctypes as C
import importlib
import os
import re

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
qb = importlib.import_module("adhoc-queries-pointclouds_amd.query_binding")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "adhoc-queries-pointclouds_amd")
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
LIB_OLD = ["pcq_scan_dev_count_batch", "pcq_scan_dev_count_batch_combined", "pcq_scan_dev_count_batch_bounds_time",
           "pcq_scan_dev_count_batch_multi", "pcq_scan_dev_class_hist_batch", "pcq_scan_dev_time_hist_batch", "pcq_scan_dev_raster_batch",
           "pcq_scan_dev_zrange_raster_batch", "pcq_scan_dev_zsum_raster_batch", "pcq_scan_dev_zsum_raster_batch_classes",
           "pcq_scan_dev_count_batch_polygon"]
QUERY_OLD = ["pcq_query_resident_count_bounds", "pcq_query_resident_count_bounds_class", "pcq_query_resident_count_bounds_time",
             "pcq_query_resident_count_bounds_many", "pcq_query_resident_count_bounds_by_class", "pcq_query_resident_count_bounds_by_time",
             "pcq_query_resident_count_bounds_raster", "pcq_query_resident_bounds_zrange_raster", "pcq_query_resident_count_polygon",
             "pcq_query_resident_bounds_zmean_raster", "pcq_query_resident_bounds_zmean_raster_classes"]
STATS = "pcq_query_resident_bounds_zmean_raster"
CLASSES = "pcq_query_resident_bounds_zmean_raster_classes"
NEW = "pcq_query_resident_bounds_zstd_raster"
DEV = "pcq_scan_dev_zmoments_raster_batch"


def test_both_entries_are_declared_and_exported_beside_the_old_ones():
    declared = pkg.declared_symbols(["pcq.h"])
    exported = pkg.exported_symbols(pkg.lib_path())
    for name in [DEV] + LIB_OLD:
        assert name in declared, name
        assert name in exported, name
    old = pkg.declared_symbols(["pcq_query.h"])
    assert len(old) == 46 and len(set(old)) == 46 and NEW not in old
    assert pkg.declared_symbols(["pcq_query_stats.h"]) == [STATS]
    assert pkg.declared_symbols(["pcq_query_classes.h"]) == [CLASSES]
    assert pkg.declared_symbols(["pcq_query_moments.h"]) == [NEW]
    exported = pkg.exported_symbols(os.path.join(PKG, "libpcq_query.so"))
    for name in [NEW] + QUERY_OLD:
        assert name in exported, name
    with open(os.path.join(ROOT, "include", "pcq_query_moments.h")) as f:
        assert '#include "pcq_query_stats.h"' in f.read()


def test_the_limits():
    with open(os.path.join(ROOT, "include", "pcq.h")) as f:
        text = f.read()
    for line in ("#define PCQ_ZMOMENTS_CELLS_MAX 1024", "#define PCQ_ZSUM_CELLS_MAX 2048", "#define PCQ_ZRANGE_CELLS_MAX 4096"):
        assert text.count(line + "\n") == 1, line
    limits = dict(re.findall(r"^#define (PCQ_[A-Z_]*CELLS_MAX) (\d+)$", text, flags=re.M))
    assert limits["PCQ_ZMOMENTS_CELLS_MAX"] == "1024" and limits["PCQ_ZSUM_CELLS_MAX"] == "2048" and limits["PCQ_ZRANGE_CELLS_MAX"] == "4096"
    assert limits["PCQ_RASTER_CELLS_MAX"] == "8192" and len(limits) == 4
    # 32 KiB of LDS per wave at each raster's own limit
    assert 1024 * 4 * 8 == 2048 * 2 * 8 == 4096 * 8 == 8192 * 4 == 32768


def test_abi_number_is_unchanged_and_the_binding_has_the_method():
    assert pkg.load_library().pcq_abi_version() == 6
    assert callable(binding.Context.scan_dev_zmoments_raster_batch)
    assert callable(binding.Context.scan_dev_zsum_raster_batch) and callable(binding.Context.scan_dev_raster_batch)
    u32, vp = C.c_uint32, C.c_void_p
    fn = getattr(pkg.load_library(), DEV)
    assert fn.restype is C.c_int and list(fn.argtypes) == [vp, C.POINTER(binding.Columns), C.POINTER(binding.Predicate), C.POINTER(u32), C.c_size_t,
                                                          u32, u32, vp, vp, vp, vp, vp]
    text = open(os.path.join(ROOT, "include", "pcq.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    (params,) = re.findall(r"\b" + DEV + r"\s*\(([^;{]*)\)\s*;", text)
    assert params.count(",") + 1 == 12 == len(fn.argtypes)


def test_the_moments_table_is_its_header():
    """names, the prototype's number of parameters, and argtypes on the loaded library; the other three tables keep to their headers"""
    assert sorted(qb.moments_sig) == sorted(pkg.declared_symbols(["pcq_query_moments.h"])) == [NEW]
    assert sorted(qb.classes_sig) == sorted(pkg.declared_symbols(["pcq_query_classes.h"])) == [CLASSES]
    assert sorted(qb.stats_sig) == sorted(pkg.declared_symbols(["pcq_query_stats.h"])) == [STATS]
    assert sorted(qb.sig) == sorted(pkg.declared_symbols(["pcq_query.h"])) and len(qb.sig) == 46
    assert not (set(qb.sig) | set(qb.stats_sig) | set(qb.classes_sig)) & set(qb.moments_sig)
    text = open(os.path.join(ROOT, "include", "pcq_query_moments.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(pcq_query_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", text)
    assert [name for name, _ in protos] == [NEW]
    assert protos[0][1].count(",") + 1 == 10 == len(qb.moments_sig[NEW][1])  # (no nested parentheses or brackets with commas in it)
    lib = pkg.load_query_library()
    for name, (res, args) in list(qb.moments_sig.items()) + list(qb.classes_sig.items()) + list(qb.stats_sig.items()) + list(qb.sig.items()):
        fn = getattr(lib, name)
        assert res is not None and fn.restype is res and list(fn.argtypes) == list(args), name
    u64, dbl = C.c_uint64, C.c_double
    assert qb.moments_sig[NEW] == (C.c_int, [C.c_void_p, C.POINTER(dbl), dbl, dbl, u64, u64, C.POINTER(u64), C.POINTER(dbl), C.POINTER(dbl),
                                             C.POINTER(u64)])


def test_host_entry_checks_its_arguments_without_a_device():
    """every case and the order test_zsum_abi.py pins for the mean-height raster, plus a null zstd"""
    lib = pkg.load_query_library()
    f = lib.pcq_query_resident_bounds_zstd_raster
    dummy = C.c_void_p(1)  # never dereferenced: a check refuses first
    lo = (C.c_double * 3)(0, 0, 0)
    s_cnt, s_mean, s_std = [1000 + 7 * c for c in range(64)], [-3.25 - c for c in range(64)], [0.5 + 2 * c for c in range(64)]
    cnt, mean, std = (C.c_uint64 * 64)(*s_cnt), (C.c_double * 64)(*s_mean), (C.c_double * 64)(*s_std)
    s = C.c_uint64(15)
    inf, nan = float("inf"), float("nan")

    def untouched():
        return list(cnt) == s_cnt and list(mean) == s_mean and list(std) == s_std and s.value == 15

    for args, text in (((None, lo, 10.0, 1.0, 8, 8, cnt, mean, std), b"null argument"), ((dummy, None, 10.0, 1.0, 8, 8, cnt, mean, std), b"null argument"),
                       ((dummy, lo, 10.0, 1.0, 8, 8, None, mean, std), b"null argument"), ((dummy, lo, 10.0, 1.0, 8, 8, cnt, None, std), b"null argument"),
                       ((dummy, lo, 10.0, 1.0, 8, 8, cnt, mean, None), b"null argument"),
                       ((None, None, 10.0, 1.0, 0, 0, None, None, None), b"null argument"),
                       ((dummy, lo, 10.0, 1.0, 1025, 1024, cnt, mean, std), b"cells"), ((dummy, lo, 10.0, 1.0, 2**20 + 1, 1, cnt, mean, std), b"cells"),
                       ((dummy, lo, 10.0, 1.0, 2**32, 2**32, cnt, mean, std), b"cells"),
                       ((dummy, lo, 10.0, 1.0, 2**64 - 1, 2**64 - 1, cnt, mean, std), b"cells"),
                       ((dummy, lo, 10.0, 0.0, 8, 8, cnt, mean, std), b"cell_size"), ((dummy, lo, 10.0, -0.5, 8, 8, cnt, mean, std), b"cell_size"),
                       ((dummy, lo, 10.0, inf, 8, 8, cnt, mean, std), b"cell_size"), ((dummy, lo, 10.0, nan, 8, 8, cnt, mean, std), b"cell_size")):
        for scanned in (C.byref(s), None):
            assert f(*args, scanned) == PCQ_ERR_ARG, args
            assert text in lib.pcq_query_last_error(), (args, lib.pcq_query_last_error())
            assert untouched()
    # a null output comes before the number of cells, the number of cells before the cell size
    assert f(dummy, lo, 10.0, nan, 2**32, 2**32, cnt, mean, None, None) == PCQ_ERR_ARG and b"null argument" in lib.pcq_query_last_error()
    assert f(dummy, lo, 10.0, nan, 0, 0, cnt, mean, None, None) == PCQ_ERR_ARG and b"null argument" in lib.pcq_query_last_error()
    assert f(dummy, lo, 10.0, nan, 2**32, 2**32, None, mean, std, None) == PCQ_ERR_ARG and b"null argument" in lib.pcq_query_last_error()
    assert f(dummy, lo, 10.0, nan, 2**32, 2**32, cnt, mean, std, None) == PCQ_ERR_ARG and b"cells" in lib.pcq_query_last_error()
    # nx * ny == 0 comes before the cell size and the number of cells: PCQ_OK, nothing written
    for nx, ny in ((0, 8), (8, 0), (0, 0), (0, 2**64 - 1)):
        assert f(dummy, lo, 10.0, nan, nx, ny, cnt, mean, std, C.byref(s)) == 0
        assert untouched()
