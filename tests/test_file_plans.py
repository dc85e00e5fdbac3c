"""What the host layer decides about a file before any GPU work, for every query kind and both file layouts, without a GPU.

tests/native/file_plan_driver.cpp prints one line per (file, query): status, needs_gpu, the record size the LAS bounds search
prints, where the plan finds its columns, and its predicate.  tests/golden/file_plans.txt holds those lines as they were
recorded ONCE from commit 0dbfbeb, the tree before the six per-kind, per-layout prologues became one plan builder (the driver uses only
Searcher::plan_file and Searcher::search_file, which that tree has too); the output of this tree must equal them byte for byte.

The corpus: LAS and LAST images of 40 points in every format 0-10, empty files, files cut one byte short of each block or record
field a plan checks, a header cut at byte 100, format bytes 11, 0x1B and 0x83, and a file whose z scale is ten times its x scale
(the reference divides every box minimum by the x scale, so a box inside the header converts to lmin > lmax).  The oracle's
synthesiser writes formats 0-3 only, so the images come from _time_images, with the two extreme points fixed: the header's
bounds, which the early-out reads, do not depend on the random generator.
"""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _time_images as ti  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "adhoc-queries-pointclouds_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "file_plans.txt")

N = 40
BOUNDS, CLASS, TIME, BOUNDS_CLASS, BOUNDS_TIME = 0, 1, 3, 4, 5
SKEW_SCALE, SKEW_OFFSET = (0.01, 0.01, 0.1), (0.0, 0.0, 0.0)


def _points(seed):
    xyz, cls, rgb, t = ti.points(N, seed)
    xyz[0], xyz[1] = (-5000, -5000, -1000), (4999, 4999, 999)  # header: x [50, 149.99], y [-300, -100.02], z [-42.5, 57.45]
    return xyz, cls, rgb, t


def _image(layout, fmt, seed, n=N, fmt_byte=None, scale=ti.SCALE, offset=ti.OFFSET):
    xyz, cls, rgb, t = _points(seed)
    rec = ti.records(fmt, xyz, cls, rgb, t)
    if layout == "last":
        body = ti.last_image(fmt, xyz, cls, rgb, t)[375 if fmt >= 6 else 227:]
    else:
        body = rec.reshape(-1)
    h = bytearray(ti.header(fmt, N, xyz, scale=scale, offset=offset, fmt_byte=fmt_byte))
    if n == 0:  # the bounds of a file with points, and none of them
        struct.pack_into("<I", h, 107, 0)
        if fmt >= 6:
            struct.pack_into("<Q", h, 247, 0)
        body = body[:0]
    return np.concatenate([np.frombuffer(bytes(h), dtype=np.uint8), body])


def _corpus(d):
    """{file name: image}, in the order of the golden file; the files are written into d."""
    files = {}
    for fmt in range(11):
        for layout in ("las", "last"):
            files[f"f{fmt}.{layout}"] = _image(layout, fmt, 100 + fmt)
    for layout in ("las", "last"):
        files[f"empty.{layout}"] = _image(layout, 1, 101, n=0)
    for fmt in (1, 3, 6):
        rl, toff, coff, kof = ti.FORMATS[fmt]
        otp = 375 if fmt >= 6 else 227
        las, last = files[f"f{fmt}.las"], files[f"f{fmt}.last"]
        # LAS: the last record cut on either side of each check (positions and class at +15: 16 bytes; class at +16; time; colour)
        for keep in sorted({14, 15, 16, toff + 7} | ({coff + 5} if coff else set())):
            files[f"f{fmt}_rec{keep}.las"] = las[:otp + (N - 1) * rl + keep]
        # LAST: one byte short of the end of each block
        for name, off, size in (("xyz", 0, 12), ("class", kof, 1), ("colour", coff, 6), ("time", toff, 8)):
            if off is not None:
                files[f"f{fmt}_{name}.last"] = last[:otp + N * (off + size) - 1]
    for layout in ("las", "last"):
        files[f"cut100.{layout}"] = files[f"f1.{layout}"][:100]
        for byte in (11, 0x1B, 0x83):
            files[f"byte{byte}.{layout}"] = _image(layout, 3, 103, fmt_byte=byte)
        files[f"skew.{layout}"] = _image(layout, 1, 101, scale=SKEW_SCALE, offset=SKEW_OFFSET)
        files[f"skew_empty.{layout}"] = _image(layout, 1, 101, n=0, scale=SKEW_SCALE, offset=SKEW_OFFSET)
    files["skew_rec15.las"] = files["skew.las"][:227 + (N - 1) * 28 + 15]
    files["skew_xyz.last"] = files["skew.last"][:227 + N * 12 - 1]
    for name, img in files.items():
        np.asarray(img).tofile(os.path.join(d, name))
    return files


def _jobs(files):
    xmax = float(ti.world(np.array([[4999, 4999, 999]]))[0, 0])  # the header's max x, to the bit
    inside, disjoint = (60.0, -290.0, -30.0, 140.0, -110.0, 50.0), (1000.0, 1000.0, 1000.0, 1001.0, 1001.0, 1001.0)
    touch = (xmax, -290.0, -30.0, xmax + 10.0, -110.0, 50.0)  # shares one face with the header's box: the early-out is inclusive
    skew = (-10.0, -10.0, 10.0, 10.0, 10.0, 20.0)             # z: lmin = 10 / 0.01 = 1000 > lmax = 20 / 0.1 = 200
    basic = [("in", BOUNDS, inside), ("class", CLASS, inside), ("time", TIME, inside), ("in+class", BOUNDS_CLASS, inside),
             ("in+time", BOUNDS_TIME, inside)]
    boxes = [("touch", BOUNDS, touch), ("touch+class", BOUNDS_CLASS, touch), ("out", BOUNDS, disjoint), ("out+class", BOUNDS_CLASS, disjoint),
             ("out+time", BOUNDS_TIME, disjoint)]
    skewed = [("skew", BOUNDS, skew), ("skew+class", BOUNDS_CLASS, skew), ("skew+time", BOUNDS_TIME, skew)]
    lines = []
    for name in files:
        stem = name.split(".")[0]
        if stem.startswith("skew"):
            queries = skewed
        elif stem in ("f1", "f6", "empty"):
            queries = basic + boxes
        elif "_" in stem:  # cut short: a box that misses the header is resolved before the blocks are checked, or after
            queries = basic + boxes[2:4]
        elif stem in ("f4", "f5", "f8", "f9", "f10"):
            queries = basic[:3]
        else:
            queries = basic
        for tag, kind, box in queries:
            lines.append(" ".join([name, tag, str(kind)] + [repr(v) for v in box] + ["2", "1200.0", "1300.0"]))
    return lines


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    host = os.path.join(PKG, "host")
    exe = str(tmp_path_factory.mktemp("file_plans") / "file_plan_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "native", "file_plan_driver.cpp"),
           os.path.join(host, "core.cpp"), os.path.join(host, "search.cpp"), os.path.join(host, "lazer.cpp"),
           os.path.join(host, "lz4_frame.cpp"), "-L" + PKG, "-lpcq", "-Wl,-rpath," + PKG, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("corpus"))
    return d, _corpus(d)


def _run(exe, args, cwd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, cwd=cwd, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-4000:])
    return r.stdout


def test_plans_and_dispatch_equal_the_recorded_ones(driver, corpus):
    """Every plan of the corpus and every line of the dispatch ladder, against the lines recorded before the refactoring."""
    d, files = corpus
    with open(os.path.join(d, "jobs.txt"), "w") as f:
        f.write("\n".join(_jobs(files)) + "\n")
    got = _run(driver, ["plans", "jobs.txt"], d) + _run(driver, ["dispatch"], d)
    with open(GOLDEN) as f:
        want = f.read()
    assert len(want) < 64 * 1024
    got_lines, want_lines = got.splitlines(), want.splitlines()
    for g, w in zip(got_lines, want_lines):
        assert g == w
    assert len(got_lines) == len(want_lines)
    assert got == want


def test_the_recorded_plans_reach_every_branch():
    """The golden file itself: each outcome the plan builder can have occurs in it, for both layouts."""
    with open(GOLDEN) as f:
        lines = f.read().splitlines()
    plans = [ln for ln in lines if " gpu=" in ln]
    for layout in (".las ", ".last "):
        mine = [ln for ln in plans if layout in ln]
        for needle in ("rc=0 gpu=1", "rc=0 gpu=0", "msg=failed to fill whole buffer", "does not contain GPS times!", "msg=Invalid LAS format 11 in file",
                       "msg=Invalid LAS format 27 in file", "msg=Invalid LAS format 131 in file", "msg=invalid point format number: 11",
                       "msg=AABB::from_min_max: Minimum position must be <= maximum position!"):
            assert any(needle in ln for ln in mine), (layout, needle)
        for kind in (BOUNDS, CLASS, TIME, BOUNDS_CLASS, BOUNDS_TIME):
            assert any(f"gpu=1" in ln and f" k={kind} " in ln for ln in mine), (layout, kind)
    # only the LAST class attribute masks the format byte: 0x83 is format 3 there and nowhere else
    ok_0x83 = sorted(ln.split()[0] + " " + ln.split()[1] for ln in plans if ln.startswith("byte131.") and " rc=0 " in ln)
    assert ok_0x83 == ["byte131.last class", "byte131.last in+class"]
    # the record size: LAS plain bounds only, on every return after the header
    assert all((" rec=-1 " not in ln) == (ln.split()[0].endswith(".las") and ln.split()[1] in ("in", "touch", "out", "skew") and "rc=-2" not in ln)
               for ln in plans)
    for text in ("Invalid extension on file", "Unsupported file extension in file", "compressed format .laz", "the Regular (non --optimized)",
                 "time search in .lazer files", "combined search in .lazer files"):
        assert any(text in ln for ln in lines if " gpu=" not in ln), text


def _expected_resident(oracle, name, img, with_points, with_times):
    """(code, message, blocks) of resident_file_blocks, from the oracle's header and the layout of a LAST file: the blocks start
    at offset_to_point_data + n * offset_in_point."""
    eof = (-5, "failed to fill whole buffer")
    if not name.endswith(".last"):
        return (-4, "resident datasets hold LAST files: " + name), None
    data = img.tobytes()
    try:
        h = oracle.parse_header(data)
    except Exception as e:  # OracleError
        msg = e.message
        if with_times and msg.startswith("invalid point format number: "):
            return (-3, f"Invalid LAS format {data[104]} in file {name}"), None
        return (-2, msg), None
    fmt, n, otp = h.point_data_record_format, h.number_of_points, h.offset_to_point_data
    rl, toff, coff, kof = ti.FORMATS[fmt]
    coff = coff if fmt in (2, 3, 5) else None  # (the reference knows the colours of formats 2, 3 and 5 only)
    inside = lambda off, size: otp + n * (off + size) <= len(data)  # noqa: E731
    if with_times:
        if toff is None:
            return (-3, f"File {name} does not contain GPS times!"), None
        if n and not (inside(0, 12) and inside(toff, 8)):
            return eof, None
    if not (inside(0, 12) and inside(kof, 1)):
        return eof, None
    colours = with_points and coff is not None
    if colours and not inside(coff, 6):
        return eof, None
    return (0, ""), {"format": fmt, "n": n, "xyz": otp, "cls": otp + n * kof, "rgb": otp + n * coff if colours else 0,
                     "time": otp + n * toff if with_times else 0}


def test_resident_blocks_follow_the_same_layout(driver, corpus, oracle):
    """ResidentDataset::load's host-only part: its failures in their order, and the four block offsets by the layout's formulas."""
    d, files = corpus
    names = [n for n in files if n.endswith(".last")] + ["f1.las", "absent.last"]
    out = _run(driver, ["resident"] + names, d).splitlines()
    assert len(out) == 4 * len(names)
    it = iter(out)
    seen = set()
    for name in names:
        for combo in range(4):
            with_points, with_times = bool(combo & 1), bool(combo & 2)
            line = next(it)
            head, msg = line.split(" msg=", 1)
            f = dict(kv.split("=") for kv in head.split()[1:])
            assert head.split()[0] == name and (int(f["points"]), int(f["times"])) == (with_points, with_times)
            if name == "absent.last":
                assert int(f["rc"]) == -1 and msg.startswith("absent.last: "), line
                continue
            (code, text), blocks = _expected_resident(oracle, name, files[name], with_points, with_times)
            assert (int(f["rc"]), msg) == (code, text), line
            seen.add(text.replace(name, "F"))
            if blocks:
                assert {k: int(f[k]) for k in blocks} == blocks, line
    assert {"", "failed to fill whole buffer", "File F does not contain GPS times!", "Invalid LAS format 131 in file F", "invalid point format number: 11",
            "resident datasets hold LAST files: F"} <= seen
