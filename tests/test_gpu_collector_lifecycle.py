"""What a collector carries from one call to the next: the scenarios of _collector_model.py replayed against the product
and the model, operation by operation.

A buffer collector keeps a two-slot device counter that flips with every emit, a host-side upper bound of what it holds,
and records that a later scan appends at byte 31 * have; a grid collector keeps pending runs of tuples, and winners that
the next fold merges; a count collector an internal or a caller-owned counter; and all collectors of a context share its
scratch, its pool and its one stream in flight.  A scenario is one context, up to four live collectors and 20 to 40
operations: scans through every entry point and predicate kind, reads, flushes, resets, frees, option changes.  At every
read the product must hold exactly what the model holds (test_collector_model.py pins the model to the oracle and states
which sequences the committed seeds contain).  Two directed tests cover sequences too specific to leave to chance, two
more keep the sequences that failed when this file was written, and one test drives the host layer's file searches
into long-lived collectors against the oracle's.
"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import _collector_model as cm
import _time_images as ti
from test_gpu_host import Q  # (ctypes view of include/pcq_query.h)

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
OTP = 227  # formats 1 and 3: the LAS 1.2 header


def make_pred(p):
    kind = p["kind"]
    if kind == "BOUNDS":
        return pkg.Predicate.bounds(p["lmin"], p["lmax"])
    if kind == "CLASS":
        return pkg.Predicate.classification(p["cls"])
    if kind == "TIME":
        return pkg.Predicate.time_range(p["start"], p["end"])
    if kind == "BOUNDS_CLASS":
        return pkg.Predicate.bounds_class(p["lmin"], p["lmax"], p["cls"])
    if kind == "BOUNDS_TIME":
        return pkg.Predicate.bounds_time(p["lmin"], p["lmax"], p["start"], p["end"])
    return pkg.Predicate.bounds_f64(p["wmin"], p["wmax"])


class Device:
    """The datasets of a scenario where the product reads them: on the device at their byte phases, in host memory and
    in a file (the LAST / LAS image)."""

    def __init__(self, ctx, datasets, tmp_path):
        self.ctx, self.datasets, self.blocks, self.views = ctx, datasets, [], []
        try:
            for k, d in enumerate(datasets):
                self.views.append(self._load(d, os.path.join(str(tmp_path), f"d{k}.{d.layout}")))
        except Exception:
            self.free()
            raise

    def put(self, arr, pad):
        arr = np.ascontiguousarray(arr)
        base = self.ctx.alloc(arr.nbytes + 64 + pad)
        self.blocks.append(base)
        assert base % 16 == 0
        if arr.nbytes:
            self.ctx.to_device(base + pad, arr)
        return base + pad

    def _load(self, d, path):
        v = {"fd": -1, "path": path}
        _, toff, coff, kof = ti.FORMATS[d.fmt]
        if d.layout == "last":
            v["xyz"], v["cls"], v["t"] = self.put(d.xyz, d.xyz_phase), self.put(d.cls, d.cls_phase), self.put(d.t, d.t_phase)
            v["rgb"] = self.put(d.rgb, d.rgb_phase) if d.rgb is not None else None
        else:
            base = self.put(ti.records(d.fmt, d.xyz, d.cls, d.rgb_all, d.t).reshape(-1), d.xyz_phase)
            v["xyz"], v["cls"], v["t"], v["rgb"] = base, base + kof, base + toff, (base + coff if d.rgb is not None else None)
        v["image"] = d.image()
        v["image"].tofile(path)
        v["fd"] = os.open(path, os.O_RDONLY)
        return v

    def columns(self, j, where, kind, n, colour):
        """The columns of dataset j's first n points for a scan of this predicate kind (a time kind: the time column in cls)."""
        d, v = self.datasets[j], self.views[j]
        rl, toff, coff, kof = ti.FORMATS[d.fmt]
        tk = cm.time_kind(kind)
        if where == "dev":
            xyz, attr, rgb = v["xyz"], (v["t"] if tk else v["cls"]), v["rgb"]
        else:
            base = (v["image"].ctypes.data if where == "host" else 0) + OTP
            if d.layout == "las":
                xyz, attr, rgb = base, base + (toff if tk else kof), (base + coff if d.rgb is not None else None)
            else:
                xyz, attr, rgb = base, base + d.n * (toff if tk else kof), (base + d.n * coff if d.rgb is not None else None)
        if not colour:
            rgb = None
        if d.layout == "las":
            return binding.make_columns(xyz=xyz, cls=attr, rgb=rgb, n=n, xyz_stride=rl, cls_stride=rl, rgb_stride=rl, scale=list(d.scale),
                                        offset=list(d.offset))
        return binding.make_columns(xyz=xyz, cls=attr, rgb=rgb, n=n, cls_stride=8 if tk else 1, scale=list(d.scale), offset=list(d.offset))

    def free(self):
        for v in self.views:
            if v["fd"] >= 0:
                os.close(v["fd"])
                os.remove(v["path"])
        for b in self.blocks:
            self.ctx.free(b)
        self.views, self.blocks = [], []


def same_grid(gg, og, what):
    assert gg.grid_params() == og.grid_params(), what
    assert gg.point_count() == og.point_count(), what
    gp, gk = gg.points(), gg.grid_cells()
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], og.grid_cells()), what
    assert gp[order].tobytes() == og.points().tobytes(), what


def same_records(got, want, what):
    if got.tobytes() != want.tobytes():
        n = min(len(got), len(want))
        a, b = got[:n].view(np.uint8).reshape(-1, 31), want[:n].view(np.uint8).reshape(-1, 31)
        bad = np.flatnonzero((a != b).any(axis=1))
        first = int(bad[0]) if len(bad) else n
        raise AssertionError(f"{what}: {len(got)} records against {len(want)}, first difference at record {first} "
                             f"({len(bad)} of the first {n} differ)")


class Replay:
    """One scenario on one context: every operation on the product and on the model; compare() at the reads."""

    def __init__(self, ctx, oracle, datasets, tmp_path):
        import torch
        self.ctx, self.datasets = ctx, datasets
        self.ts = torch.cuda.Stream()
        self.run = cm.ModelRun(oracle, datasets)
        self.colls, self.counters, self.indexes, self.first_index = {}, {}, {}, {}
        self.index_built = set()
        self.seen = {"tuple_bytes": set(), "indexed_repeats": 0}
        self.saved = {k: ctx.get_option(k) for k in cm.OPTION_VALUES}
        self.dev = Device(ctx, datasets, tmp_path)

    def close(self):
        for k, v in self.saved.items():
            self.ctx.set_option(k, v)
        for c in self.colls.values():
            c.free()
        for p in self.counters.values():
            self.ctx.free(p)
        for ix in self.indexes.values():
            self.ctx.index_free(ix)
        self.dev.free()
        self.run.finish()

    def stream(self, op):
        return self.ts.cuda_stream if op["stream"] == "caller" else None

    def step(self, op, what):
        want = self.run.apply(op)
        name = op["op"]
        if name == "set_option":
            self.ctx.set_option(op["key"], op["value"])
            return
        slot = op["slot"]
        if name == "new":
            kind = op["kind"]
            if kind == "ext":  # a caller-owned counter, zeroed by the caller
                self.counters[slot] = self.ctx.alloc(16)
                self.ctx.memset(self.counters[slot], 0, 8)
                self.ctx.synchronize()
                self.colls[slot] = self.ctx.count_collector(self.counters[slot])
            elif kind == "grid":
                self.colls[slot] = self.ctx.grid_collector(cm.GRID_BOX[0], cm.GRID_BOX[1], op["cell"])
            else:
                self.colls[slot] = self.ctx.count_collector() if kind == "count" else self.ctx.buffer_collector()
            self.first_index[slot] = 0
            return
        coll = self.colls[slot]
        if name == "free":
            coll.free()
            del self.colls[slot]
            if slot in self.counters:
                self.ctx.free(self.counters.pop(slot))
        elif name == "scan":
            self.scan(op, coll)
        elif name == "batch":
            cols = [self.dev.columns(j, "dev", p["kind"], self.datasets[j].n, False) for j, p in op["segs"]]
            self.ctx.scan_dev_count_batch(cols, [make_pred(p) for _, p in op["segs"]], self.counters[slot], self.stream(op))
            if op["stream"] == "caller":
                self.ts.synchronize()  # the collector does not know of this stream: the caller waits for it
        elif name == "flush":
            coll.flush()
        elif name == "reset":
            coll.reset()
            self.first_index[slot] = 0
        else:
            self.compare(name, coll, want, what)

    def scan(self, op, coll):
        j, p, n, entry = op["ds"], op["pred"], op["n"], op["entry"]
        d = self.datasets[j]
        where = {"scan_host": "host", "scan_host_nowait": "host", "scan_fd": "fd"}.get(entry, "dev")
        cols = self.dev.columns(j, where, p["kind"], n, op["colour"])
        cols.first_index = self.first_index[op["slot"]]
        self.first_index[op["slot"]] += n
        pred = make_pred(p)
        if entry == "scan_dev":
            self.ctx.scan_dev(cols, pred, coll, self.stream(op))
        elif entry == "scan_dev_indexed":
            ix = self.indexes.get(j)
            if ix is None:
                ix = self.indexes[j] = self.ctx.index_new()
            self.ctx.scan_dev_indexed(cols, pred, ix, coll, self.stream(op))
            covered = d.layout == "last" and n == d.n and (p["kind"] == "CLASS" or p["kind"] == "BOUNDS" and d.xyz_phase == 0 and n >= 4096)
            if covered:
                key = (j, p["kind"])
                st = self.ctx.index_stats(ix)
                assert st["built"] == (0 if key in self.index_built else 1), (op, st)  # one index, shared by the repeated queries
                self.seen["indexed_repeats"] += key in self.index_built
                self.index_built.add(key)
        elif entry == "scan_host":
            self.ctx.scan_host(cols, pred, coll)
        elif entry == "scan_host_nowait":
            self.ctx.scan_host_nowait(cols, pred, coll)
        else:
            self.ctx.scan_fd(self.dev.views[j]["fd"], cols, pred, coll)
        if coll.kind == "grid" and not cm.box_empty(p):
            self.seen["tuple_bytes"].add(self.ctx.get_option("grid_last_tuple_bytes"))

    def compare(self, name, coll, want, what):
        if coll.kind == "grid":
            if name == "point_count":
                assert coll.point_count() == want.point_count(), what
            else:
                same_grid(coll, want, what)
        elif name == "point_count":
            assert coll.point_count() == want, what
        else:
            same_records(coll.points(), want, what)

    def compare_all(self, what):
        for slot in sorted(self.colls):
            coll = self.colls[slot]
            name = "point_count" if coll.kind == "count" else "points"
            self.compare(name, coll, self.run.apply({"op": name, "slot": slot}), (what, "at the end", slot))


WITNESS = {"seeds": set(), "grid_refolds": 0, "grid_level2": 0, "tuple_bytes": set(), "indexed_repeats": 0}


def replay(ctx, oracle, datasets, ops, tmp_path, tag):
    counters = ("grid_refolds", "grid_level2", "emit_park_fallbacks")
    before = {k: ctx.get_option(k) for k in counters}
    r = Replay(ctx, oracle, datasets, tmp_path)
    try:
        for i, op in enumerate(ops):
            r.step(op, (tag, i, op))
        r.compare_all(tag)
    finally:
        r.close()
    delta = {k: ctx.get_option(k) - before[k] for k in counters}
    assert delta["emit_park_fallbacks"] == 0, tag  # (no scenario caps the scratch: every thin tile found its room)
    return delta, r.seen


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_collector_lifecycle(oracle, gpu_ctx, tmp_path, seed):
    datasets, ops = cm.scenario(seed)
    delta, seen = replay(gpu_ctx, oracle, datasets, ops, tmp_path, f"seed {seed}")
    print(f"seed {seed}: {len(ops)} operations, {delta}, {seen}")
    WITNESS["seeds"].add(seed)
    WITNESS["grid_refolds"] += delta["grid_refolds"]
    WITNESS["grid_level2"] += delta["grid_level2"]
    WITNESS["tuple_bytes"] |= seen["tuple_bytes"]
    WITNESS["indexed_repeats"] += seen["indexed_repeats"]


def test_the_intended_paths_ran():
    """Over the whole parametrised set above (it runs in front of this test): a fold was repeated with more partitions, a
    fold had a second level, grid scans wrote 16- and 24-byte tuples, and an indexed query was repeated on an index that
    existed (built == 0, asserted where it happened)."""
    if WITNESS["seeds"] != set(cm.SEEDS):
        pytest.skip("needs every seed of test_collector_lifecycle in the same run")
    print(WITNESS)
    assert WITNESS["grid_refolds"] > 0
    assert WITNESS["grid_level2"] > 0
    assert WITNESS["tuple_bytes"] == {16, 24}
    assert WITNESS["indexed_repeats"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# directed sequences
# ---------------------------------------------------------------------------------------------------------------------
def _tiles(sel):
    return np.add.reduceat(sel.astype(np.int64), np.arange(0, len(sel), cm.EMIT_TILE))


@pytest.mark.parametrize("colour", [True, False])
def test_buffer_append_at_every_record_phase(gpu_ctx, tmp_path, colour):
    """Behind k = 0 .. 31 records (a scan of the first k points that matches them all) one append each whose tiles go to
    k_emit_points (dense), k_emit_parked and k_emit_sparse, for BOUNDS, CLASS and TIME (only a box parks): the 16-byte phase
    of the append's first byte is 31 k mod 16, every value.  One collector, reset between the cases.  Only points() is
    compared: what lies behind the last record is the collector's own."""
    ctx = gpu_ctx
    rng = np.random.default_rng(77)
    d = cm.make_dataset(rng, "d", 3 * 2048 + 77, cm.SCALES[2], cm.OFFSETS[2], colour=colour, xyz_phase=4, cls_phase=3, rgb_phase=2, t_phase=8)
    everything = {"lmin": [-2**30] * 3, "lmax": [2**30] * 3}
    a, b = np.quantile(d.xyz[:, 0], [0.30, 0.31]).astype(np.int64)
    thin = {"lmin": [int(a), -2**30, -2**30], "lmax": [int(b), 2**30, 2**30]}
    # (predicate, emit_park_max, the writer every tile with matches must go to; emit_sparse_max is 256 throughout)
    cases = [({"kind": "BOUNDS", **everything}, 256, "dense"), ({"kind": "BOUNDS", **thin}, 256, "parked"), ({"kind": "BOUNDS", **thin}, 0, "sparse"),
             ({"kind": "CLASS", "cls": 2}, 256, "dense"), ({"kind": "CLASS", "cls": 1}, 256, "sparse"),
             ({"kind": "TIME", "start": -np.inf, "end": np.inf}, 256, "dense"), ({"kind": "TIME", "start": float(d.t[3000]), "end": float(d.t[3060])}, 256, "sparse")]
    for p, park, writer in cases:  # the inputs are what the case says: which writer takes the tiles (the last, ragged tile aside)
        m = _tiles(cm.select(d, p))[:-1]
        m = m[m > 0]
        park_eff = park if p["kind"] == "BOUNDS" else 0
        assert len(m) and all({"dense": v > 256, "parked": 0 < v <= park_eff, "sparse": park_eff < v <= 256}[writer] for v in m), (p, m)
    saved = {k: ctx.get_option(k) for k in ("emit_park_max", "emit_sparse_max")}
    dev = Device(ctx, [d], tmp_path)
    gb = ctx.buffer_collector()
    try:
        ctx.set_option("emit_sparse_max", 256)
        for k in range(32):
            head = {"kind": ("BOUNDS", "TIME", "BOUNDS_F64")[k % 3], **everything, "start": -np.inf, "end": np.inf, "wmin": [-1e6] * 3, "wmax": [1e6] * 3}
            for p, park, writer in cases:
                ctx.set_option("emit_park_max", park)
                gb.reset()
                want = []
                if k:
                    ctx.scan_dev(dev.columns(0, "dev", head["kind"], k, colour), make_pred(head), gb)
                    want.append(cm.records(d, head, cm.select(d, head, k), colour))
                    assert len(want[0]) == k
                ctx.scan_dev(dev.columns(0, "dev", p["kind"], d.n, colour), make_pred(p), gb)
                want.append(cm.records(d, p, cm.select(d, p), colour))
                same_records(gb.points(), np.concatenate(want), (k, p, park, writer))
    finally:
        for key, v in saved.items():
            ctx.set_option(key, v)
        gb.free()
        dev.free()


@pytest.mark.parametrize("kind", ["count", "ext", "buffer"])
def test_reset_then_scan_on_a_caller_stream(gpu_ctx, tmp_path, kind):
    """A scan on a caller's stream, reset(), another scan on the same stream, a read: the collector holds the second scan
    alone.  pcq_collector_reset zeroes the counters on the context's stream while the scan that follows stays on the
    caller's, and pcq_scratch_stream — which sees no change of stream — waits for nothing: the reset itself has to order the
    zeroing in front of that scan (it drains the context's stream).  The sequence is documented here; a race of a few
    microseconds is not something one run can be relied on to catch."""
    import torch
    ctx = gpu_ctx
    ts = torch.cuda.Stream()
    rng = np.random.default_rng(78)
    d = cm.make_dataset(rng, "d", 300_007, cm.SCALES[1], cm.OFFSETS[1], colour=True)
    first = {"kind": "CLASS", "cls": 2}
    second = {"kind": "BOUNDS", "lmin": [int(v) for v in np.quantile(d.xyz, 0.2, axis=0)], "lmax": [int(v) for v in np.quantile(d.xyz, 0.9, axis=0)]}
    dev = Device(ctx, [d], tmp_path)
    counter = None
    try:
        if kind == "ext":
            counter = ctx.alloc(16)
            ctx.memset(counter, 0, 8)
            ctx.synchronize()
        coll = {"count": ctx.count_collector, "ext": lambda: ctx.count_collector(counter), "buffer": ctx.buffer_collector}[kind]()
        try:
            ctx.scan_dev(dev.columns(0, "dev", "CLASS", d.n, True), make_pred(first), coll, ts.cuda_stream)
            coll.reset()
            ctx.scan_dev(dev.columns(0, "dev", "BOUNDS", d.n, True), make_pred(second), coll, ts.cuda_stream)
            sel = cm.select(d, second)
            assert 10_000 < int(sel.sum()) != int(cm.select(d, first).sum())
            assert coll.point_count() == int(sel.sum())
            if kind == "buffer":
                same_records(coll.points(), cm.records(d, second, sel, True), kind)
                coll.reset()  # and a reset behind a read, then a scan on the context's own stream
                ctx.scan_dev(dev.columns(0, "dev", "CLASS", d.n, True), make_pred(first), coll)
                same_records(coll.points(), cm.records(d, first, cm.select(d, first), True), kind)
        finally:
            coll.free()
    finally:
        if counter:
            ctx.free(counter)
        dev.free()


@pytest.mark.parametrize("kind", ["count", "ext", "buffer"])
def test_indexed_scan_of_a_world_space_box(gpu_ctx, tmp_path, kind):
    """Reduced from the scenarios: pcq_scan_dev_indexed with a PCQ_PRED_BOUNDS_F64 predicate.  There is no index of that
    kind: the plain scan serves it — for a count collector too, whatever columns come with it — and the index's statistics
    claim nothing.  Before and after, the index serves an integer box."""
    ctx = gpu_ctx
    rng = np.random.default_rng(79)
    d = cm.make_dataset(rng, "d", 70_001, cm.SCALES[2], cm.OFFSETS[2], colour=False)
    w = d.world()
    p = {"kind": "BOUNDS_F64", "wmin": [float(np.quantile(w[:, 0], 0.3)), -1e6, -1e6], "wmax": [float(np.quantile(w[:, 0], 0.6)), 1e6, 1e6]}
    box = {"kind": "BOUNDS", "lmin": [int(np.quantile(d.xyz[:, 0], 0.1)), -2**30, -2**30], "lmax": [int(np.quantile(d.xyz[:, 0], 0.2)), 2**30, 2**30]}
    dev = Device(ctx, [d], tmp_path)
    ix = ctx.index_new()
    counter = None
    try:
        if kind == "ext":
            counter = ctx.alloc(16)
            ctx.memset(counter, 0, 8)
            ctx.synchronize()
        coll = {"count": ctx.count_collector, "ext": lambda: ctx.count_collector(counter), "buffer": ctx.buffer_collector}[kind]()
        try:
            want = 0
            for q in (box, p, box, p):
                ctx.scan_dev_indexed(dev.columns(0, "dev", q["kind"], d.n, False), make_pred(q), ix, coll)
                want += int(cm.select(d, q).sum())
                assert coll.point_count() == want, (kind, q)
                if q is p:
                    st = ctx.index_stats(ix)
                    assert not any(st.values()), st
            assert int(cm.select(d, p).sum()) > 10_000 and int((d.cls == 0).sum()) == 0
        finally:
            coll.free()
    finally:
        ctx.index_free(ix)
        if counter:
            ctx.free(counter)
        dev.free()


def test_sparse_fold_of_several_entries_with_a_second_level(oracle, gpu_ctx, tmp_path):
    """Reduced from scenario 6, which ended in an illegal memory access: a fold of a few thousand tuples from scans that
    differ in scale, offset and tuple width (several entries), cut by a forced second level into 3584 partitions — most of
    them empty.  The folds load one tuple per lane whatever the partition holds; for an empty partition that is memory nobody
    wrote, and its idx chose the tile whose entry was looked up — anywhere.  The lookup clamps the tile now.  Whether the old
    code faulted depended on what the recycled pool block held; the sequence is kept, the cells must be the oracle's."""
    ctx = gpu_ctx
    rng = np.random.default_rng(80)
    ds = [cm.make_dataset(rng, "a", 2049, cm.SCALES[2], cm.OFFSETS[1], colour=False, cls_phase=5),
          cm.make_dataset(rng, "b", 2048, cm.SCALES[1], cm.OFFSETS[0], colour=False, xyz_phase=12),
          cm.make_dataset(rng, "c", 5121, cm.SCALES[3], cm.OFFSETS[2], colour=True, layout="las")]
    scans = [(0, {"kind": "CLASS", "cls": 2}, False), (1, {"kind": "BOUNDS_F64", "wmin": [-1e6] * 3, "wmax": [1e6] * 3}, False),
             (0, {"kind": "TIME", "start": 1200.0, "end": 1500.0}, False), (2, {"kind": "BOUNDS", "lmin": [-2**30] * 3, "lmax": [2**30] * 3}, True)]
    saved = ctx.get_option("grid_f2")
    dev = Device(ctx, ds, tmp_path)
    gg = ctx.grid_collector(cm.GRID_BOX[0], cm.GRID_BOX[1], cm.CELLS[0])
    model = cm.Model(oracle, "grid", cm.CELLS[0])
    try:
        for f2 in (7, 0, 7):  # the first fold, one onto its winners without a second level, one that cuts them again
            ctx.set_option("grid_f2", f2)
            before = ctx.get_option("grid_level2")
            for j, p, colour in scans:
                ctx.scan_dev(dev.columns(j, "dev", p["kind"], ds[j].n, colour), make_pred(p), gg)
                model.scan(cm.records(ds[j], p, cm.select(ds[j], p), colour))
            same_grid(gg, model.og, f2)
            assert ctx.get_option("grid_level2") - before == (1 if f2 else 0)
    finally:
        ctx.set_option("grid_f2", saved)
        gg.free()
        model.free()
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# the host layer: file searches of every kind into three long-lived collectors
# ---------------------------------------------------------------------------------------------------------------------
def test_host_collectors_across_files_searches_and_reads(oracle, tmp_path):
    """libpcq_query.so: bounds, class, time, box + class and box + time searches over seven small files (LAS and LAST of
    several formats, one LAZER) and the resident searches over the LAST files, in a fixed random order, each into ONE count,
    ONE buffer and ONE grid host collector, with reads in between — against the oracle's search_file / search_file_range into
    one oracle collector of each kind in the same order.  A search that a file refuses (a format without GPS time, a time
    search in a LAZER file) fails the same way on both sides and leaves the collectors as they were."""
    q = Q()
    lib = q.lib
    rng = np.random.default_rng(4100 + cm.SEED_BASE)
    files = []
    for k, (fmt, layout) in enumerate([(1, "las"), (3, "las"), (7, "las"), (3, "last"), (6, "last"), (2, "last"), (3, "lazer")]):
        xyz, cls, rgb, t = ti.points(3_000 + 1_000 * k, 4200 + k)
        img = ti.las_image(fmt, xyz, cls, rgb, t) if layout == "las" else ti.last_image(fmt, xyz, cls, rgb, t)
        if layout == "lazer":
            img = oracle.lazer_from_last(img, 1000)
        path = str(tmp_path / f"f{k}.{layout}")
        img.tofile(path)
        files.append(path)
    lasts = [f for f in files if f.endswith(".last")]
    grid_box, cell = ((-60.0, -400.0, -50.0), (160.0, 0.0, 60.0)), 2.5
    boxes = [((60.0, -250.0, -20.0), (140.0, -150.0, 40.0)), ((99.0, -300.0, -50.0), (101.0, -100.0, 60.0)), ((0.0, -400.0, -100.0), (200.0, 0.0, 100.0)),
             ((500.0, 500.0, 500.0), (600.0, 600.0, 600.0))]
    calls = [(s, f) for s in ("bounds", "class", "time", "bounds_class", "bounds_time") for f in files] + [("resident_bounds", None), ("resident_class", None)] * 2
    calls = [calls[i] for i in rng.permutation(len(calls))]
    res = C.c_void_p()
    arr = (C.c_char_p * len(lasts))(*[p.encode() for p in lasts])
    assert lib.pcq_query_resident_load_points(0, arr, len(lasts), C.byref(res)) == 0, lib.pcq_query_last_error()
    hs = {"count": q.collector("count"), "buffer": q.collector("buffer"), "grid": q.collector("grid", grid_box[0], grid_box[1], cell)}
    os_ = {"count": oracle.count_collector(), "buffer": oracle.buffer_collector(), "grid": oracle.grid_collector(grid_box[0], grid_box[1], cell)}

    def read(what):
        assert q.count(hs["count"]) == os_["count"].point_count(), what
        same_records(q.points(hs["buffer"]), os_["buffer"].points(), what)
        keys, pts = q.cells(hs["grid"]), q.points(hs["grid"])
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(keys[order], os_["grid"].grid_cells()), what
        assert pts[order].tobytes() == os_["grid"].points().tobytes(), what

    try:
        refused = 0
        for i, (search, path) in enumerate(calls):
            bmin, bmax = boxes[int(rng.integers(len(boxes)))]
            cls = int(rng.choice([1, 2, 6, 7]))
            start = float(rng.uniform(1000.0, 1900.0))
            end = start + float(rng.choice([20.0, 300.0]))
            for kind in ("count", "buffer", "grid"):
                h, o = hs[kind], os_[kind]
                if search == "bounds":
                    got, want = q.search_bounds(path, bmin, bmax, h)[0], oracle.search_file(path, 0, bmin, bmax, 0, o)[0]
                elif search == "class":
                    got, want = q.search_class(path, cls, h), oracle.search_file(path, 1, None, None, cls, o)[0]
                elif search == "time":
                    got = lib.pcq_query_search_file_time(path.encode(), start, end, 1, h)
                    want = oracle.search_file_range(path, 2, None, None, 0, start, end, o)
                elif search == "bounds_class":
                    got = lib.pcq_query_search_file_bounds_class(path.encode(), q.d3(bmin), q.d3(bmax), cls, 1, h)
                    want = oracle.search_file_range(path, 3, bmin, bmax, cls, 0.0, 0.0, o)
                elif search == "bounds_time":
                    got = lib.pcq_query_search_file_bounds_time(path.encode(), q.d3(bmin), q.d3(bmax), start, end, 1, h)
                    want = oracle.search_file_range(path, 4, bmin, bmax, 0, start, end, o)
                elif search == "resident_bounds":
                    got = lib.pcq_query_resident_search_bounds(res, q.d3(bmin), q.d3(bmax), h)
                    want = max(abs(oracle.search_file(f, 0, bmin, bmax, 0, o)[0]) for f in lasts)
                else:
                    got = lib.pcq_query_resident_search_class(res, cls, h)
                    want = max(abs(oracle.search_file(f, 1, None, None, cls, o)[0]) for f in lasts)
                assert got == want, (i, search, path, kind, lib.pcq_query_last_error(), oracle.err())
                refused += got != 0
            if i % 4 == 3 or got != 0:
                read((i, search, path))
        read("at the end")
        assert refused >= 3 * 4 and os_["count"].point_count() > 10_000  # (format 2 has no time: 2 searches; the LAZER file: 3)
    finally:
        lib.pcq_query_resident_free(res)
        for h in hs.values():
            q.free(h)
        for o in os_.values():
            o.free()
