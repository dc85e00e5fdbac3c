"""query_binding.py is the one ctypes view of include/pcq_query.h: its signature table names exactly the functions the header
declares, each with as many parameters as its prototype has, every one exported by libpcq_query.so; the status codes and the
resident-block bits named in the package are the headers' numbers.  No GPU call."""
import importlib
import os
import re

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
qb = importlib.import_module("adhoc-queries-pointclouds_amd.query_binding")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    """The header's text without comments"""
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def parameter_counts(text):
    """{function: number of parameters} of the prototypes in a comment-stripped header: top-level commas + 1, (void) is 0"""
    out = {}
    for m in re.finditer(r"\b(pcq_query_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", text):
        params, depth, commas = m.group(2).strip(), 0, 0
        for ch in params:
            depth += ch in "(["
            depth -= ch in ")]"
            commas += ch == "," and depth == 0
        out[m.group(1)] = 0 if params in ("", "void") else commas + 1
    return out


def test_the_table_is_the_header():
    declared = pkg.declared_symbols(["pcq_query.h"])
    assert len(declared) == 46 and len(set(declared)) == 46
    assert sorted(qb.sig) == sorted(declared)
    exported = pkg.exported_symbols(pkg.query_lib_path())
    assert [name for name in qb.sig if name not in exported] == []


def test_every_function_has_the_headers_number_of_parameters():
    counts = parameter_counts(header("pcq_query.h"))
    assert sorted(counts) == sorted(qb.sig)
    assert counts["pcq_query_last_error"] == 0 and counts["pcq_query_resident_bounds_zrange_raster"] == 9
    wrong = {name: (len(args), counts[name]) for name, (_, args) in qb.sig.items() if len(args) != counts[name]}
    assert not wrong, wrong


def test_every_result_type_is_stated_and_the_library_carries_the_table():
    import ctypes as C
    assert all(res is not None for res, _ in qb.sig.values())
    assert qb.sig["pcq_query_last_error"][0] is C.c_char_p
    lib = pkg.load_query_library()
    assert pkg.load_query_library() is lib
    for name, (res, args) in qb.sig.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert isinstance(pkg.query_last_error(), bytes)
    assert list(pkg.d3((1, 2.5, -3))) == [1.0, 2.5, -3.0]


def test_the_named_numbers_are_the_headers():
    status = dict((k, int(v)) for k, v in re.findall(r"\b(PCQ_OK|PCQ_ERR_[A-Z]+)\s*=\s*(-?\d+)", header("pcq.h")))
    assert len(status) == 13 and status["PCQ_OK"] == 0
    for name, value in status.items():
        assert getattr(pkg, name) == value, name
    bits = dict((k, int(v)) for k, v in re.findall(r"#define\s+(PCQ_RESIDENT_[A-Z]+)\s+(\d+)u\b", header("pcq_query.h")))
    assert sorted(bits) == ["PCQ_RESIDENT_COLOUR", "PCQ_RESIDENT_TIME"]
    for name, value in bits.items():
        assert getattr(pkg, name) == value, name


def test_the_header_structure_has_the_headers_size():
    import ctypes as C
    assert C.sizeof(pkg.LasHeaderInfo) == 24 + 12 * 8  # pcq_las_header_info: 4 x u8, 2 x u16, 2 x u32, u64, 12 doubles
