"""ctypes view of include/pcq.h and include/pcq_synth.h (libpcq.so).

Plumbing only: every scan runs in the HIP library.  Loading fails loudly when the library has not
been built (``python -c "import __graft_entry__ as g; g.build()"``).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)

PCQ_OK = 0
PCQ_ERR_IO, PCQ_ERR_HEADER, PCQ_ERR_FORMAT, PCQ_ERR_EXTENSION, PCQ_ERR_EOF = -1, -2, -3, -4, -5
PCQ_ERR_GRID, PCQ_ERR_PANIC, PCQ_ERR_ARG, PCQ_ERR_HIP, PCQ_ERR_CAPACITY = -6, -7, -8, -9, -10
PCQ_ERR_UNSUPPORTED, PCQ_ERR_NOMEM = -11, -12
PCQ_RESIDENT_COLOUR, PCQ_RESIDENT_TIME = 1, 2   # include/pcq_query.h: the `blocks` bits of pcq_query_resident_load_with
PRED_BOUNDS, PRED_CLASS, PRED_BOUNDS_F64, PRED_TIME, PRED_BOUNDS_CLASS, PRED_BOUNDS_TIME = 0, 1, 2, 3, 4, 5

# readers/src/lib.rs:10-19 — packed 31-byte result record
POINT_DTYPE = np.dtype(
    [("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("r", "<u2"), ("g", "<u2"), ("b", "<u2"), ("classification", "u1")]
)
assert POINT_DTYPE.itemsize == 31


class PcqError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"pcq error {code}: {message}")
        self.code = code
        self.message = message


class Point(C.Structure):
    _pack_ = 1
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double), ("r", C.c_uint16), ("g", C.c_uint16),
                ("b", C.c_uint16), ("classification", C.c_uint8)]


class Columns(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("cls", C.c_void_p), ("rgb", C.c_void_p), ("xyz_stride", C.c_uint64),
                ("cls_stride", C.c_uint64), ("rgb_stride", C.c_uint64), ("n", C.c_uint64), ("first_index", C.c_uint64),
                ("scale", C.c_double * 3), ("offset", C.c_double * 3)]


class Predicate(C.Structure):
    _fields_ = [("kind", C.c_int32), ("cls", C.c_uint8), ("_pad", C.c_uint8 * 3), ("lmin", C.c_int64 * 3),
                ("lmax", C.c_int64 * 3), ("wmin", C.c_double * 3), ("wmax", C.c_double * 3)]

    @staticmethod
    def bounds_f64(wmin: Sequence[float], wmax: Sequence[float]) -> "Predicate":
        p = Predicate()
        p.kind = PRED_BOUNDS_F64
        for a in range(3):
            p.wmin[a] = float(wmin[a])
            p.wmax[a] = float(wmax[a])
        return p

    @staticmethod
    def bounds(lmin: Sequence[int], lmax: Sequence[int]) -> "Predicate":
        p = Predicate()
        p.kind = PRED_BOUNDS
        for a in range(3):
            p.lmin[a] = int(lmin[a])
            p.lmax[a] = int(lmax[a])
        return p

    @staticmethod
    def classification(cls: int) -> "Predicate":
        p = Predicate()
        p.kind = PRED_CLASS
        p.cls = int(cls)
        return p

    @staticmethod
    def time_range(start: float, end: float) -> "Predicate":
        """GPS time in [start, end) (Range<f64>::contains); the time column goes in Columns.cls (cls_stride >= 8)."""
        p = Predicate()
        p.kind = PRED_TIME
        p.wmin[0] = float(start)
        p.wmax[0] = float(end)
        return p

    @staticmethod
    def bounds_class(lmin, lmax, cls: int) -> "Predicate":
        """The local box AND the class byte (PCQ_PRED_BOUNDS_CLASS): positions and class bytes are both read, even for a count."""
        p = Predicate.bounds(lmin, lmax)
        p.kind = PRED_BOUNDS_CLASS
        p.cls = int(cls)
        return p

    @staticmethod
    def bounds_time(lmin, lmax, start: float, end: float) -> "Predicate":
        """The local box AND GPS time in [start, end) (PCQ_PRED_BOUNDS_TIME); the time column goes in Columns.cls (cls_stride >= 8)."""
        p = Predicate.bounds(lmin, lmax)
        p.kind = PRED_BOUNDS_TIME
        p.wmin[0] = float(start)
        p.wmax[0] = float(end)
        return p


class DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("gcn_arch", C.c_char * 64), ("compute_units", C.c_int),
                ("wavefront_size", C.c_int), ("hbm_bytes", C.c_uint64), ("lds_bytes_per_block", C.c_uint64),
                ("clock_khz", C.c_int)]


class IndexStats(C.Structure):
    _fields_ = [("chunks", C.c_uint64), ("skipped", C.c_uint64), ("whole", C.c_uint64), ("scanned", C.c_uint64),
                ("built", C.c_uint64)]


class SynthSpec(C.Structure):
    """include/pcq_synth.h: pcq_synth_spec (the test-side host generator uses the same layout)."""
    _fields_ = [("seed", C.c_uint64), ("n", C.c_uint64), ("format", C.c_uint32), ("n_classes", C.c_uint32),
                ("scale", C.c_double * 3), ("offset", C.c_double * 3), ("lo", C.c_int32 * 3), ("span", C.c_uint32 * 3),
                ("zo_prob16", C.c_uint32), ("zo_lo", C.c_int32), ("zo_span", C.c_uint32), ("cls_cum16", C.c_uint32 * 8),
                ("cls_val", C.c_uint8 * 8)]


def lib_path() -> str:
    """libpcq.so — or, for the measurement tools in tools/ (PCQ_LAB=1), libpcq_lab.so: the same sources plus the
    superseded kernel shapes and read microbenchmarks of csrc/lab/ (make -C csrc lab); PCQ_LAB=stamps: libpcq_stamps.so,
    the timing build of the grid folds (make -C csrc stamps)."""
    which = os.environ.get("PCQ_LAB")
    return os.path.join(_HERE, "libpcq_lab.so" if which == "1" else "libpcq_stamps.so" if which == "stamps" else "libpcq.so")


_lib = None


def _one_hip_runtime() -> Optional[str]:
    """One HIP runtime per process.  libpcq.so needs `libamdhip64.so.7`; a PyTorch wheel ships its own copy of that
    library (same SONAME, found through torch/lib's RUNPATH).  Two copies in one process means two HSA runtimes, and
    the one that initialises second reports "no ROCm-capable device".  The dynamic loader reuses an already mapped
    library with the SONAME a new one asks for, so: when PyTorch is installed, its copy is mapped first (without
    importing torch) and libpcq.so binds to it — whichever of the two is imported first afterwards, there is one
    runtime.  Without PyTorch (the `query` CLI, a Rust host) libpcq.so finds ROCm's through its RUNPATH.
    PCQ_HIP_RUNTIME=rocm keeps ROCm's runtime even when PyTorch is installed."""
    if os.environ.get("PCQ_HIP_RUNTIME", "") == "rocm":
        return None
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if not os.path.exists(cand):
        return None
    C.CDLL(cand, mode=C.RTLD_GLOBAL)
    return cand


_hip_runtime_path = None


def hip_runtime_path() -> Optional[str]:
    """The libamdhip64 mapped on behalf of libpcq.so by load_library() (None: ROCm's, through the RUNPATH)."""
    return _hip_runtime_path


def load_library() -> C.CDLL:
    """Loads libpcq.so; raises if it has not been built.  There is no fallback."""
    global _lib, _hip_runtime_path
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build the HIP library first (make -C {_HERE}/csrc, or "
                           "__graft_entry__.build()). This package has no CPU path.")
    _hip_runtime_path = _one_hip_runtime()
    lib = C.CDLL(path)
    vp, u64, i64 = C.c_void_p, C.c_uint64, C.c_int64
    P = C.POINTER
    sig = {
        "pcq_init": (C.c_int, [C.c_int, P(vp)]),
        "pcq_shutdown": (C.c_int, [vp]),
        "pcq_last_error": (C.c_char_p, []),
        "pcq_abi_version": (C.c_int, []),
        "pcq_get_device_info": (C.c_int, [vp, P(DeviceInfo)]),
        "pcq_ctx_stream": (vp, [vp]),
        "pcq_ctx_synchronize": (C.c_int, [vp]),
        "pcq_box_to_local": (C.c_int, [P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_double), P(i64), P(i64)]),
        "pcq_collector_new_count": (C.c_int, [vp, P(vp)]),
        "pcq_collector_new_count_at": (C.c_int, [vp, vp, P(vp)]),
        "pcq_collector_new_buffer": (C.c_int, [vp, P(vp)]),
        "pcq_collector_new_grid": (C.c_int, [vp, P(C.c_double), P(C.c_double), C.c_double, P(vp)]),
        "pcq_collector_free": (C.c_int, [vp]),
        "pcq_collector_point_count": (C.c_int, [vp, P(u64)]),
        "pcq_collector_has_points": (C.c_int, [vp]),
        "pcq_collector_points": (C.c_int, [vp, vp, u64, P(u64)]),
        "pcq_collector_grid_cells": (C.c_int, [vp, vp, u64, P(u64)]),
        "pcq_collector_grid_params": (C.c_int, [vp, P(u64), P(u64)]),
        "pcq_collector_reset": (C.c_int, [vp]),
        "pcq_collector_flush": (C.c_int, [vp]),
        "pcq_scan_dev": (C.c_int, [vp, P(Columns), P(Predicate), vp, vp]),
        "pcq_scan_host": (C.c_int, [vp, P(Columns), P(Predicate), vp]),
        "pcq_scan_fd": (C.c_int, [vp, C.c_int, P(Columns), P(Predicate), vp]),
        "pcq_scan_host_nowait": (C.c_int, [vp, P(Columns), P(Predicate), vp]),
        "pcq_scan_fd_nowait": (C.c_int, [vp, C.c_int, P(Columns), P(Predicate), vp]),
        "pcq_prepare_host_scans": (C.c_int, [vp]),
        "pcq_scan_dev_count_batch": (C.c_int, [vp, P(Columns), P(Predicate), C.c_size_t, vp, vp]),
        "pcq_scan_dev_count_batch_combined": (C.c_int, [vp, P(Columns), P(Predicate), C.c_size_t, vp, vp]),
        "pcq_scan_dev_count_batch_bounds_time": (C.c_int, [vp, P(Columns), P(Predicate), C.c_size_t, vp, vp]),
        "pcq_scan_dev_count_batch_multi": (C.c_int, [vp, P(Columns), P(Predicate), C.c_size_t, C.c_size_t, vp, vp]),
        "pcq_scan_dev_class_hist_batch": (C.c_int, [vp, P(Columns), P(Predicate), C.c_size_t, vp, vp]),
        "pcq_scan_dev_time_hist_batch": (C.c_int, [vp, P(Columns), P(Predicate), C.c_size_t, P(C.c_double), C.c_size_t, vp, vp]),
        "pcq_scan_dev_raster_batch": (C.c_int, [vp, P(Columns), P(Predicate), P(C.c_uint32), C.c_size_t, C.c_uint32, C.c_uint32, vp, vp]),
        "pcq_scan_dev_zrange_raster_batch": (C.c_int, [vp, P(Columns), P(Predicate), P(C.c_uint32), C.c_size_t, C.c_uint32, C.c_uint32, vp, vp, vp]),
        "pcq_scan_dev_zsum_raster_batch": (C.c_int, [vp, P(Columns), P(Predicate), P(C.c_uint32), C.c_size_t, C.c_uint32, C.c_uint32, vp, vp, vp]),
        "pcq_scan_dev_zsum_raster_batch_classes": (C.c_int, [vp, P(Columns), P(Predicate), P(C.c_uint32), C.c_size_t, C.c_uint32, C.c_uint32,
                                                             P(C.c_uint32), vp, vp, vp]),
        "pcq_scan_dev_zmoments_raster_batch": (C.c_int, [vp, P(Columns), P(Predicate), P(C.c_uint32), C.c_size_t, C.c_uint32, C.c_uint32,
                                                         vp, vp, vp, vp, vp]),
        "pcq_scan_dev_zrange_raster_batch_classes": (C.c_int, [vp, P(Columns), P(Predicate), P(C.c_uint32), C.c_size_t, C.c_uint32, C.c_uint32,
                                                               P(C.c_uint32), P(C.c_uint32), vp, vp, vp]),
        "pcq_scan_dev_count_batch_polygon": (C.c_int, [vp, P(Columns), P(Predicate), P(C.c_int32), C.c_size_t, C.c_size_t, vp, vp]),
        "pcq_allreduce_sum_u64": (C.c_int, [P(vp), P(vp), P(vp), C.c_int]),
        "pcq_allreduce_prepare": (C.c_int, [P(C.c_int), C.c_int]),
        "pcq_read_fd_to_device": (C.c_int, [vp, C.c_int, u64, u64, vp]),
        "pcq_index_new": (C.c_int, [vp, P(vp)]),
        "pcq_index_free": (C.c_int, [vp]),
        "pcq_index_get_stats": (C.c_int, [vp, P(IndexStats)]),
        "pcq_scan_dev_indexed": (C.c_int, [vp, P(Columns), P(Predicate), vp, vp, vp]),
        "pcq_scan_dev_indexed_combined": (C.c_int, [vp, P(Columns), P(Predicate), vp, vp, vp]),
        "pcq_scan_dev_indexed_time": (C.c_int, [vp, P(Columns), P(Predicate), vp, vp, vp]),
        "pcq_scan_dev_indexed_bounds_time": (C.c_int, [vp, P(Columns), P(Predicate), vp, vp, vp]),
        "pcq_device_alloc": (C.c_int, [vp, u64, P(vp)]),
        "pcq_device_free": (C.c_int, [vp, vp]),
        "pcq_copy_to_device": (C.c_int, [vp, vp, vp, u64]),
        "pcq_copy_to_host": (C.c_int, [vp, vp, vp, u64]),
        "pcq_device_memset": (C.c_int, [vp, vp, C.c_int, u64, vp]),
        "pcq_set_option": (C.c_int, [vp, C.c_char_p, i64]),
        "pcq_get_option": (C.c_int, [vp, C.c_char_p, P(i64)]),
        "pcq_bind_thread_near_device": (C.c_int, [vp]),
        "pcq_synth_fill_dev": (C.c_int, [vp, P(SynthSpec), u64, u64, vp, vp, vp]),
    }
    lab_sig = {  # include/pcq_lab.h: present in libpcq_lab.so only
        "pcq_membench_read": (C.c_int, [vp, vp, u64, C.c_int, C.c_int, C.c_int, vp]),
        "pcq_membench_read_tiles": (C.c_int, [vp, vp, u64, C.c_int, C.c_int, C.c_int, vp]),
        "pcq_membench_read_xcd": (C.c_int, [vp, vp, u64, C.c_int, C.c_int, C.c_int, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in lab_sig.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def declared_symbols(headers: Optional[Sequence[str]] = None) -> list:
    """Function names declared in include/*.h (the ABI contract)."""
    inc = os.path.join(_ROOT, "include")
    names = []
    for h in headers or sorted(os.listdir(inc)):
        if not h.endswith(".h"):
            continue
        text = open(os.path.join(inc, h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names += re.findall(r"\b(pcq[a-z0-9_]*)\s*\(", text)
    seen, out = set(), []
    for n in names:
        if n not in seen:
            seen.add(n)
            out.append(n)
    return out


def exported_symbols(path: str) -> set:
    """Dynamic symbols a shared library exports (read with ctypes only: no GPU call)."""
    import subprocess
    txt = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in txt.splitlines() if line.strip()}


def class_set_words(classes) -> list:
    """A set of class bytes as the eight words of pcq.h / pcq_query_classes.h: class c is bit (c & 31) of word c >> 5."""
    words = [0] * 8
    for c in classes:
        c = int(c)
        assert 0 <= c <= 255, "a class is a byte"
        words[c >> 5] |= 1 << (c & 31)
    return words


def _check(rc: int) -> None:
    if rc != PCQ_OK:
        raise PcqError(rc, load_library().pcq_last_error().decode("utf-8", "replace"))


def _d3(v) -> C.Array:
    return (C.c_double * 3)(*[float(x) for x in v])


def box_to_local(bmin, bmax, scale, offset):
    """last.rs:98-109 via the library (pure host arithmetic; needs no device)."""
    lib = load_library()
    lmin, lmax = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    _check(lib.pcq_box_to_local(_d3(bmin), _d3(bmax), _d3(scale), _d3(offset), lmin, lmax))
    return list(lmin), list(lmax)


class Collector:
    def __init__(self, ctx: "Context", handle: int, kind: str):
        self.ctx, self.handle, self.kind = ctx, C.c_void_p(handle), kind

    def point_count(self) -> int:
        n = C.c_uint64(0)
        _check(self.ctx.lib.pcq_collector_point_count(self.handle, C.byref(n)))
        return n.value

    def has_points(self) -> bool:
        return bool(self.ctx.lib.pcq_collector_has_points(self.handle))

    def points(self) -> np.ndarray:
        n = C.c_uint64(0)
        _check(self.ctx.lib.pcq_collector_points(self.handle, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=POINT_DTYPE)
        if n.value:
            _check(self.ctx.lib.pcq_collector_points(self.handle, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def grid_cells(self) -> np.ndarray:
        n = C.c_uint64(0)
        _check(self.ctx.lib.pcq_collector_grid_cells(self.handle, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            _check(self.ctx.lib.pcq_collector_grid_cells(self.handle, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def grid_params(self):
        dims, bits = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        _check(self.ctx.lib.pcq_collector_grid_params(self.handle, dims, bits))
        return list(dims), list(bits)

    def reset(self) -> None:
        _check(self.ctx.lib.pcq_collector_reset(self.handle))

    def flush(self) -> None:
        _check(self.ctx.lib.pcq_collector_flush(self.handle))

    def free(self) -> None:
        if self.handle:
            self.ctx.lib.pcq_collector_free(self.handle)
            self.handle = C.c_void_p(None)


class Context:
    """One pcq_ctx (a GPU + its stream, staging and scratch)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        _check(self.lib.pcq_init(device, C.byref(h)))
        self.handle = h

    def close(self) -> None:
        if self.handle:
            self.lib.pcq_shutdown(self.handle)
            self.handle = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def device_info(self) -> dict:
        d = DeviceInfo()
        _check(self.lib.pcq_get_device_info(self.handle, C.byref(d)))
        return {"name": d.name.decode(), "gcn_arch": d.gcn_arch.decode(), "compute_units": d.compute_units,
                "wavefront_size": d.wavefront_size, "hbm_bytes": d.hbm_bytes,
                "lds_bytes_per_block": d.lds_bytes_per_block, "clock_khz": d.clock_khz}

    def set_option(self, key: str, value: int) -> None:
        _check(self.lib.pcq_set_option(self.handle, key.encode(), int(value)))

    def get_option(self, key: str) -> int:
        v = C.c_int64()
        _check(self.lib.pcq_get_option(self.handle, key.encode(), C.byref(v)))
        return v.value

    def synchronize(self) -> None:
        _check(self.lib.pcq_ctx_synchronize(self.handle))

    def stream_handle(self) -> int:
        """The context's own HIP stream (hipStream_t as an integer): what scans without a caller's stream and every fold run on."""
        return int(self.lib.pcq_ctx_stream(self.handle) or 0)

    # collectors -------------------------------------------------------------------------------
    def count_collector(self, device_counter: Optional[int] = None) -> Collector:
        h = C.c_void_p()
        if device_counter is None:
            _check(self.lib.pcq_collector_new_count(self.handle, C.byref(h)))
        else:
            _check(self.lib.pcq_collector_new_count_at(self.handle, C.c_void_p(device_counter), C.byref(h)))
        return Collector(self, h.value, "count")

    def buffer_collector(self) -> Collector:
        h = C.c_void_p()
        _check(self.lib.pcq_collector_new_buffer(self.handle, C.byref(h)))
        return Collector(self, h.value, "buffer")

    def grid_collector(self, bmin, bmax, cell: float) -> Collector:
        h = C.c_void_p()
        _check(self.lib.pcq_collector_new_grid(self.handle, _d3(bmin), _d3(bmax), float(cell), C.byref(h)))
        return Collector(self, h.value, "grid")

    # memory -----------------------------------------------------------------------------------
    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _check(self.lib.pcq_device_alloc(self.handle, int(nbytes), C.byref(p)))
        return p.value

    def free(self, ptr: int) -> None:
        _check(self.lib.pcq_device_free(self.handle, C.c_void_p(ptr)))

    def to_device(self, dst: int, src: np.ndarray) -> None:
        src = np.ascontiguousarray(src)
        _check(self.lib.pcq_copy_to_device(self.handle, C.c_void_p(dst), src.ctypes.data_as(C.c_void_p), src.nbytes))

    def to_host(self, dst: np.ndarray, src: int) -> None:
        _check(self.lib.pcq_copy_to_host(self.handle, dst.ctypes.data_as(C.c_void_p), C.c_void_p(src), dst.nbytes))

    def memset(self, dst: int, value: int, nbytes: int, stream: Optional[int] = None) -> None:
        _check(self.lib.pcq_device_memset(self.handle, C.c_void_p(dst), value, nbytes, C.c_void_p(stream)))

    # scans ------------------------------------------------------------------------------------
    def scan_dev(self, cols: Columns, pred: Predicate, coll: Collector, stream: Optional[int] = None) -> None:
        _check(self.lib.pcq_scan_dev(self.handle, C.byref(cols), C.byref(pred), coll.handle, C.c_void_p(stream)))

    def scan_host(self, cols: Columns, pred: Predicate, coll: Collector) -> None:
        _check(self.lib.pcq_scan_host(self.handle, C.byref(cols), C.byref(pred), coll.handle))

    def scan_host_nowait(self, cols: Columns, pred: Predicate, coll: Collector) -> None:
        """scan_host that returns once the caller's columns have been read; results after synchronize() / accessors."""
        _check(self.lib.pcq_scan_host_nowait(self.handle, C.byref(cols), C.byref(pred), coll.handle))

    def scan_fd(self, fd: int, cols: Columns, pred: Predicate, coll: Collector) -> None:
        """Like scan_host, with the column pointers given as byte offsets into the open file `fd`."""
        _check(self.lib.pcq_scan_fd(self.handle, fd, C.byref(cols), C.byref(pred), coll.handle))

    def scan_fd_nowait(self, fd: int, cols: Columns, pred: Predicate, coll: Collector) -> None:
        """scan_fd that returns once the file has been read and its last kernels are enqueued; results after synchronize() / accessors."""
        _check(self.lib.pcq_scan_fd_nowait(self.handle, fd, C.byref(cols), C.byref(pred), coll.handle))

    def prepare_host_scans(self) -> None:
        """Starts pinning the staging ring and the copy helpers on a thread of the library (returns at once)."""
        _check(self.lib.pcq_prepare_host_scans(self.handle))

    def scan_dev_count_batch(self, cols: Sequence[Columns], preds: Sequence[Predicate], device_total: int,
                             stream: Optional[int] = None) -> None:
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        _check(self.lib.pcq_scan_dev_count_batch(self.handle, ca, pa, n, C.c_void_p(device_total), C.c_void_p(stream)))

    def scan_dev_count_batch_combined(self, cols: Sequence[Columns], preds: Sequence[Predicate], device_total: int,
                                      stream: Optional[int] = None) -> None:
        """Box AND class (Predicate kind PCQ_PRED_BOUNDS_CLASS) over many resident LAST files in one launch; += into device_total."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        _check(self.lib.pcq_scan_dev_count_batch_combined(self.handle, ca, pa, n, C.c_void_p(device_total), C.c_void_p(stream)))

    def scan_dev_class_hist_batch(self, cols: Sequence[Columns], preds: Sequence[Predicate], device_hist: int,
                                  stream: Optional[int] = None) -> None:
        """The class histogram of a box (Predicate kind PCQ_PRED_BOUNDS; segments laid out as for scan_dev_count_batch_combined)
        over many resident LAST files in ONE pass: for every point inside its segment's box, += 1 into the word of its class
        byte among the PCQ_CLASS_BINS (256) words of device_hist."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        _check(self.lib.pcq_scan_dev_class_hist_batch(self.handle, ca, pa, n, C.c_void_p(device_hist), C.c_void_p(stream)))

    def scan_dev_time_hist_batch(self, cols: Sequence[Columns], preds: Sequence[Predicate], edges, device_hist: int,
                                 stream: Optional[int] = None) -> None:
        """The time histogram of a box (Predicate kind PCQ_PRED_BOUNDS; segments laid out as for
        scan_dev_count_batch_bounds_time) over many resident LAST files in ONE pass.  edges: nbins + 1 non-decreasing f64 values
        in host memory (a C-contiguous float64 numpy array is read in place, anything else is copied); for every point inside its
        segment's box whose time lies in [edges[b], edges[b + 1]), += 1 into word b of the nbins words of device_hist."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        if isinstance(edges, np.ndarray) and edges.dtype == np.float64 and edges.flags["C_CONTIGUOUS"]:
            ea = edges.ctypes.data_as(C.POINTER(C.c_double))
        else:
            ea = (C.c_double * len(edges))(*edges)
        _check(self.lib.pcq_scan_dev_time_hist_batch(self.handle, ca, pa, n, ea, max(len(edges), 1) - 1, C.c_void_p(device_hist),
                                                     C.c_void_p(stream)))

    def scan_dev_raster_batch(self, cols: Sequence[Columns], preds: Sequence[Predicate], cells, nx: int, ny: int, d_raster: int,
                              stream: Optional[int] = None) -> None:
        """The density raster of a box (Predicate kind PCQ_PRED_BOUNDS; segments laid out as for scan_dev_count_batch) over many
        resident LAST files in ONE pass.  cells: per segment its (x, y) cell widths in lattice units; for every point (X, Y, Z)
        inside its segment's box, += 1 into word ((Y - lmin[1]) // cell_y) * nx + (X - lmin[0]) // cell_x of the nx * ny words of
        d_raster."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        flat = [int(w) for c in cells for w in c]
        assert len(flat) == 2 * n, "one (x, y) pair of cell widths per segment"
        wa = (C.c_uint32 * max(len(flat), 1))(*flat)
        _check(self.lib.pcq_scan_dev_raster_batch(self.handle, ca, pa, wa, n, nx, ny, C.c_void_p(d_raster), C.c_void_p(stream)))

    def scan_dev_zrange_raster_batch(self, cols: Sequence[Columns], preds: Sequence[Predicate], cells, nx: int, ny: int, d_zmin: int,
                                     d_zmax: int, stream: Optional[int] = None) -> None:
        """The height raster of a box (segments, predicates and cells as for scan_dev_raster_batch; at most PCQ_ZRANGE_CELLS_MAX
        cells) in ONE pass: for every point (X, Y, Z) inside its segment's box, Z is folded with a signed min into word
        ((Y - lmin[1]) // cell_y) * nx + (X - lmin[0]) // cell_x of the nx * ny i32 words of d_zmin and with a signed max into that
        word of d_zmax.  The caller presets the words (INT32_MAX / INT32_MIN: nothing yet)."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        flat = [int(w) for c in cells for w in c]
        assert len(flat) == 2 * n, "one (x, y) pair of cell widths per segment"
        wa = (C.c_uint32 * max(len(flat), 1))(*flat)
        _check(self.lib.pcq_scan_dev_zrange_raster_batch(self.handle, ca, pa, wa, n, nx, ny, C.c_void_p(d_zmin), C.c_void_p(d_zmax),
                                                         C.c_void_p(stream)))

    def scan_dev_zsum_raster_batch(self, cols: Sequence[Columns], preds: Sequence[Predicate], cells, nx: int, ny: int, d_count: int,
                                   d_zsum: int, stream: Optional[int] = None) -> None:
        """The mean-height raster of a box (segments, predicates and cells as for scan_dev_raster_batch; at most PCQ_ZSUM_CELLS_MAX
        cells) in ONE pass: for every point (X, Y, Z) inside its segment's box, += 1 into word ((Y - lmin[1]) // cell_y) * nx +
        (X - lmin[0]) // cell_x of the nx * ny u64 words of d_count and += Z into that i64 word of d_zsum, both modulo 2^64."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        flat = [int(w) for c in cells for w in c]
        assert len(flat) == 2 * n, "one (x, y) pair of cell widths per segment"
        wa = (C.c_uint32 * max(len(flat), 1))(*flat)
        _check(self.lib.pcq_scan_dev_zsum_raster_batch(self.handle, ca, pa, wa, n, nx, ny, C.c_void_p(d_count), C.c_void_p(d_zsum),
                                                       C.c_void_p(stream)))

    def scan_dev_zsum_raster_batch_classes(self, cols: Sequence[Columns], preds: Sequence[Predicate], cells, nx: int, ny: int, classes,
                                           d_count: int, d_zsum: int, stream: Optional[int] = None) -> None:
        """The mean-height raster of the points of a set of classes (scan_dev_zsum_raster_batch restricted to them; segments laid
        out as for scan_dev_count_batch_combined: cls beside xyz) in ONE pass.  classes: the class bytes of the set, an iterable of
        0 .. 255 (class_set_words makes the eight words), or None for a null class_set."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        flat = [int(w) for c in cells for w in c]
        assert len(flat) == 2 * n, "one (x, y) pair of cell widths per segment"
        wa = (C.c_uint32 * max(len(flat), 1))(*flat)
        sa = None if classes is None else (C.c_uint32 * 8)(*class_set_words(classes))
        _check(self.lib.pcq_scan_dev_zsum_raster_batch_classes(self.handle, ca, pa, wa, n, nx, ny, sa, C.c_void_p(d_count),
                                                               C.c_void_p(d_zsum), C.c_void_p(stream)))

    def scan_dev_zmoments_raster_batch(self, cols: Sequence[Columns], preds: Sequence[Predicate], cells, nx: int, ny: int, d_count: int,
                                       d_zsum: int, d_zsq_lo: int, d_zsq_hi: int, stream: Optional[int] = None) -> None:
        """The height-spread raster of a box (segments, predicates and cells as for scan_dev_raster_batch; at most
        PCQ_ZMOMENTS_CELLS_MAX cells) in ONE pass: for every point (X, Y, Z) inside its segment's box, into the word of its cell of
        each of four arrays of nx * ny words, += 1 (d_count), += Z (d_zsum, i64), += (Z * Z) & 0xffffffff (d_zsq_lo) and
        += (Z * Z) >> 32 (d_zsq_hi), all modulo 2^64."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        flat = [int(w) for c in cells for w in c]
        assert len(flat) == 2 * n, "one (x, y) pair of cell widths per segment"
        wa = (C.c_uint32 * max(len(flat), 1))(*flat)
        _check(self.lib.pcq_scan_dev_zmoments_raster_batch(self.handle, ca, pa, wa, n, nx, ny, C.c_void_p(d_count), C.c_void_p(d_zsum),
                                                           C.c_void_p(d_zsq_lo), C.c_void_p(d_zsq_hi), C.c_void_p(stream)))

    def scan_dev_zrange_raster_batch_classes(self, cols: Sequence[Columns], preds: Sequence[Predicate], cells, nx: int, ny: int, low, high,
                                             d_zmin: int, d_zmax: int, stream: Optional[int] = None) -> None:
        """The canopy-height raster of a box (segments laid out as for scan_dev_zsum_raster_batch_classes: cls beside xyz; at most
        PCQ_ZRANGE_CLASSES_CELLS_MAX cells) in ONE pass: for every point inside its segment's box, d_zmin[cell] = min(itself, Z) when
        the point's class byte is in `low` and d_zmax[cell] = max(itself, Z) when it is in `high`, signed i32.  low, high: the class
        bytes of each set, iterables of 0 .. 255 (class_set_words makes the eight words), or None for a null pointer."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        flat = [int(w) for c in cells for w in c]
        assert len(flat) == 2 * n, "one (x, y) pair of cell widths per segment"
        wa = (C.c_uint32 * max(len(flat), 1))(*flat)
        la = None if low is None else (C.c_uint32 * 8)(*class_set_words(low))
        ha = None if high is None else (C.c_uint32 * 8)(*class_set_words(high))
        _check(self.lib.pcq_scan_dev_zrange_raster_batch_classes(self.handle, ca, pa, wa, n, nx, ny, la, ha, C.c_void_p(d_zmin),
                                                                 C.c_void_p(d_zmax), C.c_void_p(stream)))

    def scan_dev_count_batch_polygon(self, cols: Sequence[Columns], preds: Sequence[Predicate], verts, d_total: int,
                                     stream: Optional[int] = None) -> None:
        """Box AND polygon (Predicate kind PCQ_PRED_BOUNDS; segments laid out as for scan_dev_count_batch_multi) over many resident
        LAST files in ONE pass.  verts: per segment its outline as a sequence of (x, y) pairs of i32 in the segment's lattice, all of
        one length (3 .. PCQ_POLYGON_VERTS_MAX); for every point inside its segment's box and inside the outline under the even-odd
        rule of pcq.h, += 1 into the word d_total."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        assert len(verts) == n, "one outline per segment"
        nverts = len(verts[0]) if n else 3
        assert all(len(v) == nverts for v in verts), "outlines of one length"
        flat = [int(w) for v in verts for xy in v for w in xy]
        assert len(flat) == 2 * n * nverts, "(x, y) pairs"
        va = (C.c_int32 * max(len(flat), 1))(*flat)
        _check(self.lib.pcq_scan_dev_count_batch_polygon(self.handle, ca, pa, va, n, nverts, C.c_void_p(d_total), C.c_void_p(stream)))

    def scan_dev_count_batch_bounds_time(self, cols: Sequence[Columns], preds: Sequence[Predicate], device_total: int,
                                         stream: Optional[int] = None) -> None:
        """Box AND GPS time range (Predicate kind PCQ_PRED_BOUNDS_TIME; the times in Columns.cls, stride 8) over many resident
        LAST files in one launch; += into device_total."""
        n = len(cols)
        ca = (Columns * n)(*cols)
        pa = (Predicate * n)(*preds)
        _check(self.lib.pcq_scan_dev_count_batch_bounds_time(self.handle, ca, pa, n, C.c_void_p(device_total), C.c_void_p(stream)))

    def scan_dev_count_batch_multi(self, cols: Sequence[Columns], pred_rows: Sequence[Sequence[Predicate]], device_totals: int,
                                   stream: Optional[int] = None, nqueries: Optional[int] = None) -> None:
        """Up to PCQ_MULTI_BOX_MAX boxes (Predicate kind PCQ_PRED_BOUNDS) asked of many resident LAST files in ONE pass:
        pred_rows[i][q] is box q of segment i (an empty box: not asked of that segment); the count of box q is += into word q of
        device_totals.  nqueries: the row length, for a call without segments."""
        n = len(cols)
        if len(pred_rows) != n:
            raise ValueError("one row of predicates per segment")
        nq = (len(pred_rows[0]) if n else 0) if nqueries is None else nqueries
        if any(len(row) != nq for row in pred_rows):
            raise ValueError("every row holds nqueries predicates")
        ca = (Columns * n)(*cols)
        pa = (Predicate * (n * nq))(*[p for row in pred_rows for p in row])
        _check(self.lib.pcq_scan_dev_count_batch_multi(self.handle, ca, pa, n, nq, C.c_void_p(device_totals), C.c_void_p(stream)))

    # chunk index --------------------------------------------------------------------------------
    def index_new(self) -> int:
        h = C.c_void_p()
        _check(self.lib.pcq_index_new(self.handle, C.byref(h)))
        return h.value

    def index_free(self, ix: int) -> None:
        self.lib.pcq_index_free(C.c_void_p(ix))

    def index_stats(self, ix: int) -> dict:
        st = IndexStats()
        _check(self.lib.pcq_index_get_stats(C.c_void_p(ix), C.byref(st)))
        return {k: getattr(st, k) for k, _ in IndexStats._fields_}

    def scan_dev_indexed(self, cols: Columns, pred: Predicate, ix: int, coll: Collector, stream: Optional[int] = None) -> None:
        _check(self.lib.pcq_scan_dev_indexed(self.handle, C.byref(cols), C.byref(pred), C.c_void_p(ix), coll.handle,
                                             C.c_void_p(stream)))

    def scan_dev_indexed_combined(self, cols: Columns, pred: Predicate, ix: int, coll: Collector, stream: Optional[int] = None) -> None:
        """Box AND class through both parts of the chunk index (boxes and class histograms)."""
        _check(self.lib.pcq_scan_dev_indexed_combined(self.handle, C.byref(cols), C.byref(pred), C.c_void_p(ix), coll.handle,
                                                      C.c_void_p(stream)))

    def scan_dev_indexed_time(self, cols: Columns, pred: Predicate, ix: int, coll: Collector, stream: Optional[int] = None) -> None:
        """GPS time in [start, end) through the time part of the chunk index (min, max and NaN count per 4096 times)."""
        _check(self.lib.pcq_scan_dev_indexed_time(self.handle, C.byref(cols), C.byref(pred), C.c_void_p(ix), coll.handle,
                                                  C.c_void_p(stream)))

    def scan_dev_indexed_bounds_time(self, cols: Columns, pred: Predicate, ix: int, coll: Collector, stream: Optional[int] = None) -> None:
        """Box AND GPS time range through the bounds part and the time part of the chunk index (the same 4096-point chunks)."""
        _check(self.lib.pcq_scan_dev_indexed_bounds_time(self.handle, C.byref(cols), C.byref(pred), C.c_void_p(ix), coll.handle,
                                                         C.c_void_p(stream)))

    def synth_fill(self, spec: SynthSpec, first: int, count: int, d_xyz: Optional[int], d_cls: Optional[int],
                   stream: Optional[int] = None) -> None:
        _check(self.lib.pcq_synth_fill_dev(self.handle, C.byref(spec), first, count, C.c_void_p(d_xyz),
                                           C.c_void_p(d_cls), C.c_void_p(stream)))


def make_columns(xyz=None, cls=None, rgb=None, n=0, xyz_stride=12, cls_stride=1, rgb_stride=6, first_index=0,
                 scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0)) -> Columns:
    c = Columns()
    c.xyz, c.cls, c.rgb = xyz, cls, rgb
    c.xyz_stride, c.cls_stride, c.rgb_stride = xyz_stride, cls_stride, rgb_stride
    c.n, c.first_index = n, first_index
    for a in range(3):
        c.scale[a] = float(scale[a])
        c.offset[a] = float(offset[a])
    return c
