"""adhoc-queries-pointclouds_amd — MI355X-native predicate path for ad-hoc point-cloud queries.

The product is native code:
  * ``libpcq.so``        HIP kernels + the thin C ABI of ``include/pcq.h`` (``csrc/``)
  * ``libpcq_query.so``  C++ host layer mirroring the reference's Searcher / ResultCollector
                         interface (``host/``), plus the ``query`` CLI binary

This Python package is only a ctypes view of those C ABIs, one module per library: ``binding.py`` views
``include/pcq.h`` and ``include/pcq_synth.h`` (``load_library()``), ``query_binding.py`` views
``include/pcq_query.h`` (``load_query_library()``).  Each holds the one signature table of its header; the
tests, the tools, ``bench.py`` and ``__graft_entry__.py`` declare no function themselves.  It never computes a scan itself and has no CPU fallback: if the HIP
library is missing or no device is usable, it raises.

The directory name contains hyphens (it mirrors the upstream repository name), so import it with
``importlib.import_module("adhoc-queries-pointclouds_amd")``.
"""
from .binding import (  # noqa: F401
    PcqError,
    Columns,
    Predicate,
    Point,
    SynthSpec,
    POINT_DTYPE,
    Context,
    Collector,
    lib_path,
    load_library,
    hip_runtime_path,
    box_to_local,
    exported_symbols,
    declared_symbols,
    IndexStats,
    PCQ_OK, PCQ_ERR_IO, PCQ_ERR_HEADER, PCQ_ERR_FORMAT, PCQ_ERR_EXTENSION, PCQ_ERR_EOF, PCQ_ERR_GRID, PCQ_ERR_PANIC,
    PCQ_ERR_ARG, PCQ_ERR_HIP, PCQ_ERR_CAPACITY, PCQ_ERR_UNSUPPORTED, PCQ_ERR_NOMEM,
    PCQ_RESIDENT_COLOUR, PCQ_RESIDENT_TIME,
)
from .query_binding import (  # noqa: F401
    LasHeaderInfo,
    query_lib_path,
    load_query_library,
    query_last_error,
    d3,
)
