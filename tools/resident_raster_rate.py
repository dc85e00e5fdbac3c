"""Developer tool: the density raster of a box on resident data — one pass that bins every point inside the box into an nx x ny
raster over x and y, against the plain box count of the same bytes (the floor) and, for 8 x 8, against the only other way to the
same answer: one box per cell through the multi-box count, eight boxes per pass.

FILES resident synthetic files of N points each (the 4 x 4 tiles of synth_ca13), twice: (g) in the generator's order (random inside
a tile) and (s) in scan-strip order (strips 10 m wide in y and z, points sorted along x — the order of flight-line tiles: the
lanes of a wave mostly share a cell).  Two boxes: the ca13_XL box and the same with z unbounded, which keeps every point.  Rasters
of 8 x 8, 64 x 64 and 128 x 64 cells over the box's x and y.  Per order, box and raster the routes are timed with device events
around the whole of each, alternated in one process, REPS rounds after 3 warm-up rounds; median, minimum and maximum, TB/s on
12 B/point:
  raster      ONE pcq_scan_dev_raster_batch;
  count       ONE pcq_scan_dev_count_batch: the floor — the same bytes, a popcount instead of two divisions and an LDS add;
  cells       (8 x 8 only) the 64 cells as boxes through pcq_scan_dev_count_batch_multi, eight launches of eight boxes, as
              pcq_query_resident_count_bounds_many issues them: a tile that misses a cell carries an empty predicate for it, a
              tile that misses all eight cells of a group is no segment of that group's launch.
Every raster must sum to the plain count; the 8 x 8 raster must equal the 64 cell counts.  Rule: for 8 x 8, raster's slowest round
is below cells' fastest round, in both orders.
With PCQ_LAB=1 (libpcq_lab.so accepts the options "raster_waves_per_cu" and "raster_add") also the one pass with the per-lane add
(1) and the wave-level shortcut (2) at 2 .. 16 workgroups per CU before the LDS limit (160 KiB / (4 nx ny): 5 at 128 x 64).
The last line restates the checks.
usage: resident_raster_rate.py [N [FILES [REPS]]]"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 163_000_000
files = int(sys.argv[2]) if len(sys.argv) > 2 else 16
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
dev = torch.device("cuda:0")
ts = torch.cuda.Stream(); torch.cuda.set_stream(ts); stream = ts.cuda_stream
lab = os.environ.get("PCQ_LAB") == "1"
RASTERS = ((8, 8), (64, 64), (128, 64))
EMPTY = ([1, 1, 1], [0, 0, 0])


def spread(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "reps": len(v)}


def alternate(fns, reps, warm=3):
    """fns: name -> callable; one of each per round, device events around each, the first `warm` rounds dropped"""
    times = {k: [] for k in fns}
    for it in range(reps + warm):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record(); e1.synchronize()
            if it >= warm:
                times[k].append(e0.elapsed_time(e1))
    return {k: spread(v) for k, v in times.items()}


def tbps(points, ms):
    return points * 12 / (ms * 1e-3) / 1e12


checks = {}
with pkg.Context(0) as ctx:
    tiles = specs.synth_ca13(points_per_file=n, files=files)
    bmin, bmax = specs.box("ca13_XL")
    keep, cols = [], {"g": [], "s": []}
    for spec in tiles:
        raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
        cls = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        ctx.synth_fill(spec, 0, n, raw.data_ptr(), cls.data_ptr(), stream)
        torch.cuda.synchronize()
        t = raw.view(n, 3)
        width, zwidth = int(10.0 / spec.scale[1]), int(10.0 / spec.scale[2])
        key = ((t[:, 1].long() // width) * 4096 + (t[:, 2].long() // zwidth + 2048)) * (1 << 32) + (t[:, 0].long() + (1 << 31))
        order = torch.argsort(key)
        del key
        strips = t[order].contiguous().view(-1)
        del order, cls
        keep += [raw, strips]
        for name, buf in (("g", raw), ("s", strips)):
            assert buf.data_ptr() % 16 == 0
            cols[name].append(binding.make_columns(xyz=buf.data_ptr(), n=n, scale=list(spec.scale), offset=list(spec.offset)))
    torch.cuda.synchronize()
    # every tile has the scale and offset of the first: one local box, one lattice
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(tiles[0].scale), list(tiles[0].offset))
    assert all(pkg.box_to_local(bmin, bmax, list(s.scale), list(s.offset)) == (lmin, lmax) for s in tiles)
    out = torch.zeros(128 * 64, dtype=torch.int64, device=dev)
    total = torch.zeros(64, dtype=torch.int64, device=dev)
    points = files * n

    def geometry(nx, ny, zlo, zhi):
        cw = [-(-(lmax[a] - lmin[a] + 1) // d) for a, d in ((0, nx), (1, ny))]
        lo, hi = [lmin[0], lmin[1], zlo], [lmin[0] + nx * cw[0] - 1, lmin[1] + ny * cw[1] - 1, zhi]
        return cw, lo, hi

    for box_name, (zlo, zhi) in (("ca13_XL", (lmin[2], lmax[2])), ("every_point", (-2**40, 2**40))):
        for nx, ny in RASTERS:
            cw, lo, hi = geometry(nx, ny, zlo, zhi)
            preds = [pkg.Predicate.bounds(lo, hi)] * files
            cells = [cw] * files
            groups = []  # (8 x 8) per group of eight cells: the tiles that meet one of them, and their rows of eight predicates
            if (nx, ny) == (8, 8):
                for q0 in range(0, 64, 8):
                    segs, rows = [], []
                    for i, s in enumerate(tiles):
                        row = []
                        for q in range(q0, q0 + 8):
                            clo = [lo[0] + (q % 8) * cw[0], lo[1] + (q // 8) * cw[1], lo[2]]
                            chi = [clo[0] + cw[0] - 1, clo[1] + cw[1] - 1, hi[2]]
                            met = all(s.lo[a] <= chi[a] and s.lo[a] + s.span[a] - 1 >= clo[a] for a in range(2))  # (the header early-out)
                            row.append(pkg.Predicate.bounds(clo, chi) if met else pkg.Predicate.bounds(*EMPTY))
                            if met:
                                segs.append(i)
                        rows.append(row)
                    live = sorted(set(segs))
                    groups.append((live, [rows[i] for i in live]))
            for order in ("g", "s"):
                c = cols[order]

                def raster():
                    out.zero_()
                    ctx.scan_dev_raster_batch(c, preds, cells, nx, ny, out.data_ptr(), stream)

                def count():
                    total.zero_()
                    ctx.scan_dev_count_batch(c, preds, total.data_ptr(), stream)

                def by_cells():
                    total.zero_()
                    for g, (live, rows) in enumerate(groups):
                        ctx.scan_dev_count_batch_multi([c[i] for i in live], rows, total.data_ptr() + 64 * g, stream)

                raster(); count()
                torch.cuda.synchronize()
                ras, in_box = out[:nx * ny].clone(), int(total[0])
                tag = f"{box_name}_{nx}x{ny}_{order}"
                checks[f"{tag}_sums_to_the_count"] = int(ras.sum()) == in_box
                routes = {"raster": raster, "count": count}
                if groups:
                    by_cells()
                    torch.cuda.synchronize()
                    checks[f"{tag}_equals_the_cell_counts"] = ras.tolist() == total.tolist()
                    routes["cells"] = by_cells
                res = alternate(routes, reps)
                res["raster"]["TBps_12B_per_point"] = tbps(points, res["raster"]["median_ms"])
                res["count"]["TBps_12B_per_point"] = tbps(points, res["count"]["median_ms"])
                line = {"box": box_name, "nx_ny": [nx, ny], "order": order, "files": files, "points_per_file": n, "in_box": in_box,
                        "cells_hit": int((ras > 0).sum()), "largest_cell": int(ras.max()), "raster_over_count": res["raster"]["median_ms"] / res["count"]["median_ms"]}
                if groups:
                    read = sum(len(live) for live, _ in groups) * n
                    res["cells"]["points_read"] = read
                    line["speedup_over_cells"] = res["cells"]["median_ms"] / res["raster"]["median_ms"]
                    checks[f"{tag}_raster_faster_than_cells_beyond_spread"] = res["raster"]["max_ms"] < res["cells"]["min_ms"]
                print("(rate)", json.dumps({**line, **res}), flush=True)
                if lab:  # ---- the one pass with either add at other grids -----------------------------------------------------
                    sweep = {}
                    for add in (1, 2):
                        ctx.set_option("raster_add", add)
                        for w in (2, 3, 4, 5, 6, 8, 12, 16):
                            ctx.set_option("raster_waves_per_cu", w)
                            r = alternate({"raster": raster}, max(3, reps // 2), warm=1)["raster"]
                            torch.cuda.synchronize()
                            assert out[:nx * ny].tolist() == ras.tolist(), (add, w)
                            sweep[f"add{add}_w{w}"] = [round(r["median_ms"], 3), round(r["min_ms"], 3), round(r["max_ms"], 3)]
                    ctx.set_option("raster_add", 0)
                    ctx.set_option("raster_waves_per_cu", 0)
                    print("(sweep)", json.dumps({"box": box_name, "nx_ny": [nx, ny], "order": order, "lds_limit_waves_per_cu": 160 * 1024 // (4 * nx * ny),
                                                 "median_min_max_ms": sweep}), flush=True)
    del keep, cols
print("checks", json.dumps(checks), flush=True)
