"""ctypes view of include/pcq_query.h, include/pcq_query_stats.h, include/pcq_query_classes.h, include/pcq_query_moments.h and include/pcq_query_canopy.h (libpcq_query.so): the C++ host layer and the resident-dataset API.

Plumbing only, in the style of binding.load_library(): ONE signature table per header for every function it declares, so that no
caller writes an argtypes line of its own.  The conventions, chosen once:

  * three-vectors, edge tables and vertex arrays are POINTER(c_double) (d3(v) builds a three-vector; a float64 numpy array goes
    in as ``a.ctypes.data_as(POINTER(c_double))``);
  * counts, histograms and rasters are POINTER(c_uint64);
  * the two bulk record buffers (collector_points, collector_grid_cells) and raw byte buffers are c_void_p, as binding.py has
    them for their pcq_ twins;
  * handles (collectors, resident datasets) are c_void_p, handle outputs POINTER(c_void_p);
  * pcq_index_stats, pcq_columns and pcq_predicate are binding.py's structures.

None is accepted wherever the header allows a null pointer.  Importing this module opens nothing; load_query_library() makes no
device call.
"""
from __future__ import annotations

import ctypes as C
import os

from . import binding
from .binding import Columns, IndexStats, Predicate, PCQ_RESIDENT_COLOUR, PCQ_RESIDENT_TIME  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))


class LasHeaderInfo(C.Structure):
    """include/pcq_query.h: pcq_las_header_info."""
    _fields_ = [("version_major", C.c_uint8), ("version_minor", C.c_uint8), ("point_data_record_format", C.c_uint8),
                ("_pad", C.c_uint8), ("header_size", C.c_uint16), ("point_data_record_length", C.c_uint16),
                ("offset_to_point_data", C.c_uint32), ("_pad2", C.c_uint32), ("number_of_points", C.c_uint64),
                ("scale", C.c_double * 3), ("offset", C.c_double * 3), ("min", C.c_double * 3), ("max", C.c_double * 3)]


def query_lib_path() -> str:
    return os.path.join(_HERE, "libpcq_query.so")


def _signatures() -> dict:
    vp, u64, dbl, u8, sz = C.c_void_p, C.c_uint64, C.c_double, C.c_uint8, C.c_size_t
    P = C.POINTER
    dd, pu64, strs, pint = P(dbl), P(u64), P(C.c_char_p), P(C.c_int)
    return {
        "pcq_query_last_error": (C.c_char_p, []),
        "pcq_query_last_was_panic": (C.c_int, []),
        "pcq_query_parse_las_header": (C.c_int, [vp, sz, C.c_int, P(LasHeaderInfo)]),
        "pcq_query_parse_aabb": (C.c_int, [C.c_char_p, dd, dd]),
        "pcq_query_is_valid_file": (C.c_int, [C.c_char_p]),
        "pcq_query_get_total_bounds": (C.c_int, [strs, sz, dd, dd]),
        "pcq_query_lz4_frame_decode": (C.c_int, [vp, sz, u64, u64, vp, u64]),
        "pcq_query_collector_new_count": (C.c_int, [C.c_int, P(vp)]),
        "pcq_query_collector_new_buffer": (C.c_int, [C.c_int, P(vp)]),
        "pcq_query_collector_new_grid": (C.c_int, [C.c_int, dd, dd, dbl, P(vp)]),
        "pcq_query_collector_free": (C.c_int, [vp]),
        "pcq_query_collector_point_count": (C.c_int, [vp, pu64]),
        "pcq_query_collector_has_points": (C.c_int, [vp]),
        "pcq_query_collector_points": (C.c_int, [vp, vp, u64, pu64]),
        "pcq_query_collector_grid_cells": (C.c_int, [vp, vp, u64, pu64]),
        "pcq_query_search_file_bounds": (C.c_int, [C.c_char_p, dd, dd, C.c_int, vp, pint]),
        "pcq_query_search_file_class": (C.c_int, [C.c_char_p, u8, C.c_int, vp]),
        "pcq_query_search_file_time": (C.c_int, [C.c_char_p, dbl, dbl, C.c_int, vp]),
        "pcq_query_search_file_bounds_class": (C.c_int, [C.c_char_p, dd, dd, u8, C.c_int, vp]),
        "pcq_query_search_file_bounds_time": (C.c_int, [C.c_char_p, dd, dd, dbl, dbl, C.c_int, vp]),
        "pcq_query_resident_load": (C.c_int, [C.c_int, strs, sz, P(vp)]),
        "pcq_query_resident_free": (C.c_int, [vp]),
        "pcq_query_resident_count_bounds": (C.c_int, [vp, dd, dd, pu64, pu64]),
        "pcq_query_resident_count_class": (C.c_int, [vp, u8, pu64, pu64]),
        "pcq_query_resident_count_bounds_class": (C.c_int, [vp, dd, dd, u8, pu64, pu64]),
        "pcq_query_resident_count_bounds_many": (C.c_int, [vp, sz, dd, dd, pu64, pu64, pu64]),
        "pcq_query_resident_count_bounds_by_class": (C.c_int, [vp, dd, dd, pu64, pu64]),
        "pcq_query_resident_load_points": (C.c_int, [C.c_int, strs, sz, P(vp)]),
        "pcq_query_resident_search_bounds": (C.c_int, [vp, dd, dd, vp]),
        "pcq_query_resident_search_class": (C.c_int, [vp, u8, vp]),
        "pcq_query_resident_search_bounds_class": (C.c_int, [vp, dd, dd, u8, vp]),
        "pcq_query_resident_load_with": (C.c_int, [C.c_int, strs, sz, C.c_uint, P(vp)]),
        "pcq_query_resident_search_time": (C.c_int, [vp, dbl, dbl, vp]),
        "pcq_query_resident_count_bounds_time": (C.c_int, [vp, dd, dd, dbl, dbl, pu64, pu64]),
        "pcq_query_resident_count_bounds_by_time": (C.c_int, [vp, dd, dd, dd, sz, pu64, pu64]),
        "pcq_query_resident_count_bounds_raster": (C.c_int, [vp, dd, dbl, dbl, u64, u64, pu64, pu64]),
        "pcq_query_resident_bounds_zrange_raster": (C.c_int, [vp, dd, dbl, dbl, u64, u64, dd, dd, pu64]),
        "pcq_query_resident_count_polygon": (C.c_int, [vp, sz, dd, dbl, dbl, pu64, pu64]),
        "pcq_query_resident_search_bounds_time": (C.c_int, [vp, dd, dd, dbl, dbl, vp]),
        "pcq_query_resident_last_stats": (C.c_int, [vp, P(IndexStats)]),
        "pcq_query_main": (C.c_int, [C.c_int, strs]),
        "pcq_query_main_with_hooks": (C.c_int, [C.c_int, strs, C.c_char_p, C.c_int]),
        "pcq_query_simulate_schedule": (C.c_int, [pu64, sz, dd, C.c_int, dbl, pint, pint, dd]),
        "pcq_query_test_plan_time": (C.c_int, [C.c_char_p, dbl, dbl, P(Columns), P(Predicate), pint]),
        "pcq_query_test_plan_combined": (C.c_int, [C.c_char_p, dd, dd, C.c_int, dbl, dbl, P(Columns), P(Predicate), pint]),
        "pcq_query_test_plan_replace_execute": (C.c_int, [C.c_char_p, C.c_char_p, dd, dd, vp]),
    }


def _stats_signatures() -> dict:
    vp, u64, dbl = C.c_void_p, C.c_uint64, C.c_double
    dd, pu64 = C.POINTER(dbl), C.POINTER(u64)
    return {
        "pcq_query_resident_bounds_zmean_raster": (C.c_int, [vp, dd, dbl, dbl, u64, u64, pu64, dd, pu64]),
    }


def _classes_signatures() -> dict:
    vp, u64, dbl = C.c_void_p, C.c_uint64, C.c_double
    dd, pu64 = C.POINTER(dbl), C.POINTER(u64)
    return {
        "pcq_query_resident_bounds_zmean_raster_classes": (C.c_int, [vp, dd, dbl, dbl, u64, u64, C.POINTER(C.c_uint32), pu64, dd, pu64]),
    }


def _moments_signatures() -> dict:
    vp, u64, dbl = C.c_void_p, C.c_uint64, C.c_double
    dd, pu64 = C.POINTER(dbl), C.POINTER(u64)
    return {
        "pcq_query_resident_bounds_zstd_raster": (C.c_int, [vp, dd, dbl, dbl, u64, u64, pu64, dd, dd, pu64]),
    }


def _canopy_signatures() -> dict:
    vp, u64, dbl = C.c_void_p, C.c_uint64, C.c_double
    dd, pu64, pu32 = C.POINTER(dbl), C.POINTER(u64), C.POINTER(C.c_uint32)
    return {
        "pcq_query_resident_bounds_canopy_raster": (C.c_int, [vp, dd, dbl, dbl, u64, u64, pu32, pu32, dd, dd, dd, pu64]),
    }


sig = _signatures()   # {name: (restype, argtypes)} for every function of include/pcq_query.h
stats_sig = _stats_signatures()   # the same for include/pcq_query_stats.h (which says why it is a header of its own)
classes_sig = _classes_signatures()   # the same for include/pcq_query_classes.h (a header of its own for the same reason)
moments_sig = _moments_signatures()   # the same for include/pcq_query_moments.h (likewise)
canopy_sig = _canopy_signatures()   # the same for include/pcq_query_canopy.h (likewise)
_qlib = None


def load_query_library() -> C.CDLL:
    """Loads libpcq_query.so (once per process); raises if it has not been built.  libpcq.so is loaded first, through
    binding.load_library(), so that binding._one_hip_runtime's rule holds whichever of the two a process asks for first."""
    global _qlib
    if _qlib is not None:
        return _qlib
    path = query_lib_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build the host layer first (make -C {_HERE}/host, or __graft_entry__.build()).")
    binding.load_library()
    lib = C.CDLL(path)
    for name, (res, args) in list(sig.items()) + list(stats_sig.items()) + list(classes_sig.items()) + list(moments_sig.items()) + \
            list(canopy_sig.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _qlib = lib
    return lib


def d3(v) -> C.Array:
    """A three-vector (or any flat sequence of floats) as a C array of doubles."""
    v = [float(x) for x in v]
    return (C.c_double * len(v))(*v)


def query_last_error() -> bytes:
    """The message of the last failure of a pcq_query_ call on this thread."""
    return load_query_library().pcq_query_last_error()
