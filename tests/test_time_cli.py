"""The GPS time-range search on the host side, without a GPU: the `--time` argument of the CLI, its place among --bounds and
--class, the format errors that a file's plan resolves before any GPU work, where the plans of LAS and LAST files find the
times and positions, and the new entry point of the C view.

Files of format 0 or 2 carry no GPS time (las.rs:306-318), formats above 10 are "Invalid LAS format" (:324-329); both
are found by the parallel driver's host-only planning pass (run_search.cpp), so those queries end before a device is
opened.  The records, counts and grids of the search are in test_gpu_time.py.
"""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _time_images as ti  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "adhoc-queries-pointclouds_amd")
QUERY = os.path.join(PKG, "host", "query")
pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

NEITHER = "Error: Found neither BOUNDS nor CLASS argument but exactly one of these arguments is required!"
BOTH = "Error: Specifying BOUNDS and CLASS at the same time is invalid! Specify either BOUNDS or CLASS argument!"
WITH_TIME = "Error: Specifying TIME together with BOUNDS or CLASS is invalid! Specify exactly one of BOUNDS, CLASS or TIME!"
BAD_TIME = "Could not prase argument TIME"


def _query(args):
    r = subprocess.run([QUERY] + args, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture
def datadir(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    return str(d)


@pytest.mark.parametrize("value", ["abc", "1", "1;2;3", "1;", ";2", "0x1;2", " 1;2", "1;2 ", "1,2", ""])
def test_time_values_that_do_not_parse_panic_like_their_siblings(datadir, value):
    rc, out, err = _query(["-i", datadir, "--time", value])
    assert (rc, out, err.strip()) == (101, "", BAD_TIME)


@pytest.mark.parametrize("value", ["1;2", "-inf;inf", "NaN;1", "2;1", "1e3;1E4", "+1.5;-0.0"])
def test_time_values_parse_like_bounds_components(datadir, value):
    """Rust's f64 parse: inf / NaN / exponents / signs accepted.  The directory is empty: nothing is searched."""
    rc, out, err = _query(["-i", datadir, "--time", value, "--optimized", "--parallel"])
    assert rc == 0, err
    assert out.startswith("Searching 0 files...\n"), out


@pytest.mark.parametrize("args,rc,msg", [
    (["--bounds", "0;0;0;1;1;1", "--class", "2"], 1, BOTH),
    (["--bounds", "0;0;0;1;1;1", "--class", "2", "--time", "0;1"], 1, BOTH),   # the existing check comes first
    (["--bounds", "0;0;0;1;1;1", "--time", "0;1"], 1, WITH_TIME),
    (["--class", "2", "--time", "0;1"], 1, WITH_TIME),
    ([], 1, NEITHER),
    (["--density", "1"], 1, NEITHER),
    (["--class", "2", "--time", "zz"], 101, BAD_TIME),                          # values are parsed before they are compared
])
def test_exactly_one_of_bounds_class_time(datadir, args, rc, msg):
    got = _query(["-i", datadir] + args)
    assert (got[0], got[1], got[2].strip()) == (rc, "", msg)


def test_help_lists_the_time_flag():
    rc, out, _ = _query(["-h"])
    assert rc == 0
    assert re.search(r"^\s+--time <TIME>\s+\"start;end\": GPS time range, start <= t < end$", out, re.M), out


def _write(path, img):
    img.tofile(path)
    return str(path)


@pytest.mark.parametrize("fmt,ext", [(0, "las"), (2, "las"), (0, "last"), (2, "last")])
def test_files_without_gps_times_fail_on_the_host(datadir, fmt, ext):
    xyz, cls, rgb, t = ti.points(64, fmt)
    img = ti.las_image(fmt, xyz, cls, rgb, t)
    p = _write(os.path.join(datadir, f"f.{ext}"), img)
    rc, out, err = _query(["-i", datadir, "--time", "0;1", "--optimized", "--parallel"])
    assert (rc, out, err.strip()) == (1, "Searching 1 files...\n", f"Error: File {p} does not contain GPS times!")


@pytest.mark.parametrize("fmt_byte,ext", [(11, "las"), (12, "last"), (255, "las")])
def test_formats_above_10_fail_on_the_host(datadir, fmt_byte, ext):
    xyz, cls, rgb, t = ti.points(64, 3)
    img = ti.las_image(1, xyz, cls, rgb, t, fmt_byte=fmt_byte)
    p = _write(os.path.join(datadir, f"f.{ext}"), img)
    rc, out, err = _query(["-i", datadir, "--time", "0;1", "--optimized", "--parallel"])
    assert (rc, out, err.strip()) == (1, "Searching 1 files...\n", f"Error: Invalid LAS format {fmt_byte} in file {p}")


@pytest.fixture(scope="module")
def qlib():
    return pkg.load_query_library()


def _plan(qlib, path, start, end):
    cols, pred, needs = binding.Columns(), binding.Predicate(), C.c_int(-1)
    rc = qlib.pcq_query_test_plan_time(path.encode(), start, end, C.byref(cols), C.byref(pred), C.byref(needs))
    return rc, cols, pred, needs.value


@pytest.mark.parametrize("fmt", [1, 3, 6, 7])
@pytest.mark.parametrize("layout", ["las", "last"])
def test_plans_find_the_times_and_positions(qlib, tmp_path, fmt, layout):
    n = 1_001
    xyz, cls, rgb, t = ti.points(n, fmt)
    img = ti.las_image(fmt, xyz, cls, rgb, t) if layout == "las" else ti.last_image(fmt, xyz, cls, rgb, t)
    p = _write(tmp_path / f"f.{layout}", img)
    rc, cols, pred, needs = _plan(qlib, p, 1200.0, 1300.0)
    assert (rc, needs) == (0, 1), qlib.pcq_query_last_error()
    otp = 375 if fmt >= 6 else 227
    toff = ti.time_offset(fmt)
    assert pred.kind == binding.PRED_TIME and (pred.wmin[0], pred.wmax[0]) == (1200.0, 1300.0)
    assert cols.n == n and cols.xyz == otp and cols.rgb is None
    assert list(cols.scale) == list(ti.SCALE) and list(cols.offset) == list(ti.OFFSET)
    if layout == "las":
        rl = ti.FORMATS[fmt][0]
        assert (cols.cls, cols.xyz_stride, cols.cls_stride) == (otp + toff, rl, rl)
        got_t = np.frombuffer(img[cols.cls:].tobytes()[:(n - 1) * rl + 8], dtype=np.uint8)
        got_t = np.stack([got_t[i * rl:i * rl + 8] for i in range(n)]).copy().view("<f8").ravel()
    else:
        assert (cols.cls, cols.xyz_stride, cols.cls_stride) == (otp + n * toff, 12, 8)
        got_t = img[cols.cls:cols.cls + 8 * n].copy().view("<f8")
        got_xyz = img[cols.xyz:cols.xyz + 12 * n].copy().view("<i4").reshape(n, 3)
        assert np.array_equal(got_xyz, xyz)
    assert np.array_equal(got_t, t)  # the plan's time column holds the file's times


def test_plans_of_empty_and_truncated_files(qlib, tmp_path):
    xyz, cls, rgb, t = ti.points(10, 1)
    empty = ti.las_image(1, xyz[:0], cls[:0], rgb[:0], t[:0])
    rc, _, _, needs = _plan(qlib, _write(tmp_path / "e.las", empty), 0.0, 1.0)
    assert (rc, needs) == (0, 0)  # nothing to scan: resolved on the host
    full = ti.last_image(1, xyz, cls, rgb, t)
    rc, _, _, needs = _plan(qlib, _write(tmp_path / "t.last", full[:-1]), 0.0, 1.0)  # the time block reaches past the end
    assert (rc, needs) == (-5, 0)
    full = ti.las_image(3, xyz, cls, rgb, t)
    rc, _, _, needs = _plan(qlib, _write(tmp_path / "t.las", full[:-6]), 0.0, 1.0)  # last record's colour gone: its time is still there
    assert (rc, needs) == (0, 1)
    rc, _, _, needs = _plan(qlib, _write(tmp_path / "u.las", full[:-7]), 0.0, 1.0)
    assert (rc, needs) == (-5, 0)


def test_format_errors_carry_the_format_status(qlib, tmp_path):
    xyz, cls, rgb, t = ti.points(10, 2)
    for fmt, fb, msg in [(0, None, "does not contain GPS times!"), (2, None, "does not contain GPS times!"),
                         (1, 14, "Invalid LAS format 14 in file ")]:
        p = _write(tmp_path / "f.last", ti.las_image(fmt, xyz, cls, rgb, t, fmt_byte=fb))
        rc, _, _, needs = _plan(qlib, p, 0.0, 1.0)
        assert (rc, needs) == (-3, 0)
        assert msg in qlib.pcq_query_last_error().decode()


def test_query_library_exports_the_time_search():
    """pcq_query_search_file_time is declared in pcq_query.h and exported by libpcq_query.so; PCQ_PRED_TIME is 3 and the ABI
    version stays 6 (the structs did not change)."""
    hdr = open(os.path.join(ROOT, "include", "pcq_query.h")).read()
    assert re.search(r"int pcq_query_search_file_time\(const char \*path, double start, double end, int optimized,\s+"
                     r"pcq_host_collector \*c\);", hdr)
    lib = pkg.load_query_library()
    assert hasattr(lib, "pcq_query_search_file_time") and hasattr(lib, "pcq_query_test_plan_time")
    assert re.search(r"PCQ_PRED_TIME = 3\b", open(os.path.join(ROOT, "include", "pcq.h")).read())
    assert binding.PRED_TIME == 3
    p = binding.Predicate.time_range(-1.5, float("inf"))
    assert (p.kind, p.wmin[0], p.wmax[0]) == (3, -1.5, float("inf"))
    core = C.CDLL(os.path.join(PKG, "libpcq.so"))
    assert core.pcq_abi_version() == 6


def test_time_pass0_keeps_its_loads_in_flight():
    """The grid collector's pass 0 for TIME (packed and strided) reads the next tile's times while this tile is sorted: no
    wait right behind a time load (global_load_dwordx2 for 8-byte aligned times, dwords or bytes otherwise) — the property
    test_hot_loops_keep_their_loads_in_flight guards for the class byte."""
    from test_abi_and_host import _kernel_asm, _kernel_bodies
    found = {}
    for name, body in _kernel_bodies(_kernel_asm("grid_pass0.hip"), "k_p0_part"):
        if not name.startswith("_ZN7pcqgrid9k_p0_partILi3E"):  # PCQ_PRED_TIME
            continue
        loads = 0
        for n, l in enumerate(body):
            if any(k in l for k in ("global_load_dwordx2", "global_load_dword ", "global_load_ubyte")):
                loads += 1
                assert not any("vmcnt(0)" in x for x in body[n + 1:n + 3]), (name, n, l.strip())
        found[name] = loads
    assert sorted(found) == ["_ZN7pcqgrid9k_p0_partILi3ELb0ELb0ELb0EEEvNS_6P0ArgsE", "_ZN7pcqgrid9k_p0_partILi3ELb0ELb1ELb0EEEvNS_6P0ArgsE"]
    packed = found["_ZN7pcqgrid9k_p0_partILi3ELb0ELb1ELb0EEEvNS_6P0ArgsE"]
    assert packed > 0
