"""The time part of the chunk index and time queries on resident datasets: the libpcq entry (include/pcq.h) and the two host
entries (include/pcq_query.h) are declared and exported, beside the old ones — the ABI number is what it was; the host entries
refuse null arguments before any device is touched; and the numpy model of the chunk states that the GPU tests compare the
statistics with (tests/_time_index_model.py) agrees with a brute-force selection.  No GPU call."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _time_images as ti  # noqa: E402
import _time_index_model as tm  # noqa: E402

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "adhoc-queries-pointclouds_amd")
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
LIB_NEW = ["pcq_scan_dev_indexed_time"]
QUERY_NEW = ["pcq_query_resident_load_with", "pcq_query_resident_search_time"]


def test_the_three_entries_are_declared_and_exported():
    declared = pkg.declared_symbols(["pcq.h"])
    exported = pkg.exported_symbols(pkg.lib_path())
    for name in LIB_NEW:
        assert name in declared, name
        assert name in exported, name
    declared = pkg.declared_symbols(["pcq_query.h"])
    exported = pkg.exported_symbols(os.path.join(PKG, "libpcq_query.so"))
    for name in QUERY_NEW:
        assert name in declared, name
        assert name in exported, name
    text = open(os.path.join(ROOT, "include", "pcq_query.h")).read()
    assert "#define PCQ_RESIDENT_COLOUR 1u" in text and "#define PCQ_RESIDENT_TIME 2u" in text


def test_abi_number_is_unchanged_and_the_binding_has_the_method():
    assert pkg.load_library().pcq_abi_version() == 6
    binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
    assert callable(binding.Context.scan_dev_indexed_time)


def test_host_entries_refuse_null_arguments_without_a_device():
    lib = pkg.load_query_library()
    dummy = C.c_void_p(1)  # never dereferenced: another argument is null
    out = C.c_void_p(7)
    one = (C.c_char_p * 1)(None)
    assert lib.pcq_query_resident_load_with(0, one, 1, 3, None) == PCQ_ERR_ARG       # no place for the result
    assert lib.pcq_query_resident_load_with(0, None, 1, 3, C.byref(out)) == PCQ_ERR_ARG  # no list
    assert lib.pcq_query_resident_load_with(0, one, 1, 2, C.byref(out)) == PCQ_ERR_ARG   # a null path
    assert out.value is None
    assert b"null argument" in lib.pcq_query_last_error()
    assert lib.pcq_query_resident_load_with(0, one, 1, 4, C.byref(out)) == PCQ_ERR_ARG   # a bit that names no block
    assert lib.pcq_query_resident_search_time(None, 0.0, 1.0, dummy) == PCQ_ERR_ARG
    assert lib.pcq_query_resident_search_time(dummy, 0.0, 1.0, None) == PCQ_ERR_ARG
    assert b"null argument" in lib.pcq_query_last_error()


def adversarial_chunks():
    """Chunks of 4096 times: ordinary, adversarial, and the corners the state table names."""
    out = []
    for seed in range(4):
        out.append(np.sort(np.random.default_rng(seed).uniform(-1.5, 1.5, tm.CHUNK)))
    for k, (start, end) in enumerate(ti.RANGES):
        out.append(ti.adversarial_times(tm.CHUNK, start, end, 50 + k))
    inside = np.random.default_rng(9).uniform(0.25, 0.75, tm.CHUNK)
    one_nan = inside.copy()
    one_nan[1234] = np.nan
    out += [inside, one_nan, np.full(tm.CHUNK, np.nan), np.full(tm.CHUNK, 0.0), np.full(tm.CHUNK, -0.0),
            np.where(np.arange(tm.CHUNK) % 2 == 0, 0.0, -0.0), np.full(tm.CHUNK, np.inf), np.full(tm.CHUNK, -np.inf),
            np.full(tm.CHUNK, 1.0), np.full(tm.CHUNK, 5e-324), np.where(np.arange(tm.CHUNK) % 2 == 0, np.nan, 0.5)]
    return out


@pytest.mark.parametrize("rng", ti.RANGES + [(0.25, 0.75), (0.0, 0.75), (0.25, 1.0), (0.5, 2.0), (-np.inf, 1.0), (0.0, 5e-324)])
def test_the_model_of_the_chunk_states_agrees_with_a_brute_force_selection(rng):
    start, end = rng
    seen = set()
    for t in adversarial_chunks():
        st, sel = tm.chunk_state(t, start, end), ti.select(t, start, end)
        seen.add(st)
        if st == tm.NONE:
            assert not sel.any(), (rng, t[:4])
        if st == tm.ALL:
            assert sel.all(), (rng, t[:4])
        # and the other way round wherever the three numbers can tell: no match at all in a chunk without NaN whose times
        # are all on one side, every time a match
        if not sel.any() and (not (start < end) or np.isnan(t).all()):
            assert st == tm.NONE
        if sel.all():
            assert st == tm.ALL, (rng, t[:4])
    assert tm.NONE in seen or tm.ALL in seen


def test_the_model_on_the_corners_of_the_table():
    inside = np.linspace(0.25, 0.75, tm.CHUNK)
    one_nan = inside.copy()
    one_nan[77] = np.nan
    assert tm.chunk_state(inside, 0.25, 0.76) == tm.ALL
    assert tm.chunk_state(one_nan, 0.25, 0.76) == tm.SCAN and int(ti.select(one_nan, 0.25, 0.76).sum()) == tm.CHUNK - 1
    assert tm.chunk_state(np.full(tm.CHUNK, np.nan), -np.inf, np.inf) == tm.NONE
    assert tm.chunk_state(inside, 0.0, 0.75) == tm.SCAN      # max == end: the last time is no match
    assert tm.chunk_state(inside, 0.0, 0.25) == tm.NONE      # min == end
    assert tm.chunk_state(inside, 0.75, 2.0) == tm.SCAN      # max == start: read
    zeros = np.where(np.arange(tm.CHUNK) % 2 == 0, 0.0, -0.0)
    assert tm.chunk_state(zeros, -0.0, 5e-324) == tm.ALL and tm.chunk_state(zeros, 0.0, 1.0) == tm.ALL
    assert tm.chunk_state(np.full(tm.CHUNK, np.inf), -np.inf, np.inf) == tm.NONE      # inf < inf is false
    assert tm.chunk_state(np.full(tm.CHUNK, -np.inf), -np.inf, np.inf) == tm.ALL
    assert tm.chunk_state(np.full(tm.CHUNK, np.inf), 1.0, np.inf) == tm.NONE
    for start, end in [(1.0, 1.0), (1.0, -1.0), (np.nan, 1.0), (-1.0, np.nan)]:
        assert tm.chunk_state(inside, start, end) == tm.NONE
    assert tm.classify(np.concatenate([inside, one_nan, inside + 1.0, inside[:100]]), 0.25, 0.76) == (1, 1, 1)
