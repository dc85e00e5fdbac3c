"""pcq_set_option / pcq_get_option and the PCQ_* environment of pcq_init: every option documented in include/pcq.h has the
default written in csrc/pcq_internal.h, accepts exactly its range, and leaves its value alone when a set is refused; the
diagnostics read and cannot be set.  No scan runs here."""
import importlib
import os
import re

import pytest

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -8

# name, field of pcq_ctx, min, max (None: the lower edge only)
RANGED = [
    ("blocks_per_cu", "grid_blocks_per_cu", 1, 32),
    ("chunk_points", "chunk_points", 4, None),
    ("copy_threads", "copy_threads", 1, 64),
    ("allreduce_fail", "allreduce_fail", 0, 3),
    ("grid_pending_budget", "grid_pending_budget", 0, 1 << 40),
    ("grid_agg", "grid_agg", 0, 2),
    ("grid_f2", "grid_f2", 0, 4096),
    ("host_in_place", "host_in_place", 0, 2),
    ("emit_park_max", "emit_park_max", 0, 256),
    ("emit_sparse_max", "emit_sparse_max", 0, 2048),
    ("grid_tuple16", "grid_tuple16", 0, 2),
    ("grid_stream", "grid_stream", 0, 1),
    ("grid_block_pad", "grid_block_pad", 0, 65536),
    ("grid_p0_blocks", "grid_p0_blocks", 0, 65536),
    ("scratch_cap_words", "scratch_cap_words", 0, None),
]
BOOLEAN = [("numa_local", "numa_local"), ("allreduce_single_rank", "allreduce_single_rank")]
DIAGNOSTICS = ["numa_node", "grid_folds", "grid_level2", "grid_refolds", "grid_level2_exact", "grid_compactions", "grid_last_f2",
               "grid_last_tuples", "grid_last_tuple_bytes", "emit_park_fallbacks", "grid_deferred", "grid_dense_deferred"]


def header_default(field):
    """The initialiser of a pcq_ctx member in pcq_internal.h (`int x = 2;`, `uint64_t x = 1ull << 20;`, several per line)."""
    text = open(os.path.join(ROOT, "adhoc-queries-pointclouds_amd", "csrc", "pcq_internal.h")).read()
    body = text[text.index("struct pcq_ctx {"):text.index("struct pcq_collector {")]
    m = re.search(r"\b%s\s*=\s*([^;,]+)[;,]" % re.escape(field), body)
    assert m, field
    return int(eval(re.sub(r"(\d)(?:ull|ll|u)\b", r"\1", m.group(1))))


def refused(ctx, key, value):
    with pytest.raises(pkg.PcqError) as e:
        ctx.set_option(key, value)
    return e.value.code == ERR_ARG


def test_every_documented_option_has_its_default_and_its_range(monkeypatch):
    doc = open(os.path.join(ROOT, "include", "pcq.h")).read()
    for name in [r[0] for r in RANGED] + [b[0] for b in BOOLEAN] + DIAGNOSTICS:
        assert '"%s"' % name in doc, name
        monkeypatch.delenv("PCQ_" + name.upper(), raising=False)
    with pkg.Context(0) as ctx:
        for name, field, lo, hi in RANGED:
            default = ctx.get_option(name)
            if name == "copy_threads":  # pcq_init caps it at the host's hardware threads per GPU, never below 2
                assert default == header_default(field) or 2 <= default < header_default(field), default
            else:
                assert default == header_default(field), name
            for v in [lo] + ([hi] if hi is not None else []):
                ctx.set_option(name, v)
                assert ctx.get_option(name) == v, (name, v)
            ctx.set_option(name, default)
            for v in [lo - 1] + ([hi + 1] if hi is not None else []):
                assert refused(ctx, name, v), (name, v)
                assert ctx.get_option(name) == default, (name, v)
        for name, field in BOOLEAN:
            default = ctx.get_option(name)
            assert default == header_default(field), name
            for v, want in ((0, 0), (1, 1), (7, 1), (-3, 1), (1 << 40, 1), (0, 0)):
                ctx.set_option(name, v)
                assert ctx.get_option(name) == want, (name, v)
            ctx.set_option(name, default)
        for name in DIAGNOSTICS:
            before = ctx.get_option(name)
            assert refused(ctx, name, 0) and refused(ctx, name, 1), name
            assert ctx.get_option(name) == before, name
        assert ctx.get_option("numa_node") >= -1
        assert refused(ctx, "no_such_option", 1)
        with pytest.raises(pkg.PcqError) as e:
            ctx.get_option("no_such_option")
        assert e.value.code == ERR_ARG
    monkeypatch.setenv("PCQ_CHUNK_POINTS", "4096")
    with pkg.Context(0) as ctx:
        assert ctx.get_option("chunk_points") == 4096
    monkeypatch.setenv("PCQ_CHUNK_POINTS", "3")  # out of range: ignored silently
    monkeypatch.setenv("PCQ_HOST_IN_PLACE", "7")
    with pkg.Context(0) as ctx:
        assert ctx.get_option("chunk_points") == header_default("chunk_points")
        assert ctx.get_option("host_in_place") == header_default("host_in_place")
