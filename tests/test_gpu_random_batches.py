"""Seeded random parity of eleven batched entries with numpy (_random_batches.py; its seeds are proven on the CPU by
test_random_batches_plan.py).  PCQ_TEST_SEED_BASE moves the whole seed range for a soak run.

Per seed: the case is uploaded once, all the entries run through binding.Context on the session's context — consecutive seeds
bring unrelated shapes, so the segment table and the partials are reused, outgrown and regrown across them — and every output
word is compared with numpy's, exactly.  The outputs lie in one device buffer, each between two runs of guard words, all of it
preset to distinct non-zero words: the counts have to be ADDED to what was there, the height raster FOLDED onto it (its words
are preset to values among the data's own, to INT32_MAX / INT32_MIN "nothing yet", and to the limits that no z can beat), and
no guard word may change.  The mean-height raster, which joined the ten later (the test keeps its name), adds its counts and its
z sums into two arrays behind the others' outputs; test_the_mean_height_raster_against_numpy asks for it alone, from a table and
partials that the previous seed's call left.  A mismatch names the seed, the entry, the first words with got - want, and the segments whose
shares (numpy's, per segment) make up those words: rerun draw(seed) and cut the case down to them.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _random_batches as rb  # noqa: E402
from _random_batches import I32_MAX, I32_MIN  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

GUARD = 16  # u64 words in front of and behind every output
STREAM_SEEDS = (3, 11, 19, 27, 35, 43)


def image(size, offs, parts, unit):
    img = np.zeros(size + 64, dtype=np.uint8)
    for o, a in zip(offs, parts):
        img[o:o + len(a) * unit] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return img


def layout(c):
    """Per output its first u64 word and its length in u64 words (the height raster: two arrays of i32 words, two to a u64 word,
    an odd cell count rounded up: the half word behind it is a guard as well); the buffer's length"""
    at, q = {}, GUARD
    for name in rb.FIRST_TEN[:-2] + ("polygon", "zmin", "zmax", "zcount", "zsum"):
        words = (rb.words_of(c, "zrange") + 1) // 2 if name in ("zmin", "zmax") else rb.words_of(c, "zsum" if name == "zcount" else name)
        at[name] = (q, words)
        q += words + GUARD
    return at, q


def preset_words(c, total, at):
    """Distinct non-zero u64 words; the height raster's i32 words from the case's own z values and the two limits"""
    rng = np.random.default_rng(rb.BASE + rb.SEED_BASE + c.seed + 10**6)
    pre = (1000 + 7 * np.arange(total) + (np.arange(total) << 40)).astype(np.uint64)
    zs = np.concatenate([x[:, 2] for x in c.xyz] + [np.asarray([I32_MIN, I32_MAX], dtype=np.int32)])
    w32 = pre.view(np.int32)
    for name, nothing in (("zmin", I32_MAX), ("zmax", I32_MIN)):
        first, words = at[name]
        v = rng.choice(zs, 2 * words)
        v[rng.random(2 * words) < 0.4] = nothing
        w32[2 * first:2 * (first + words)] = v
    return pre


def expected(c, pre, at, entries=rb.ENTRIES):
    exp = pre.copy()
    for e in entries:
        if e == "zsum":  # (modulo 2^64: the presets are large)
            for name, words in zip(("zcount", "zsum"), rb.answer(c, e)):
                first, n = at[name]
                exp[first:first + n] += words.view(np.uint64)
        elif e == "zrange":
            zmin, zmax = rb.answer(c, e)
            cells = len(zmin)
            w32 = exp.view(np.int32)
            a, b = 2 * at["zmin"][0], 2 * at["zmax"][0]
            w32[a:a + cells] = np.minimum(w32[a:a + cells], zmin)
            w32[b:b + cells] = np.maximum(w32[b:b + cells], zmax)
        else:
            first, words = at[e]
            exp[first:first + words] += rb.answer(c, e).astype(np.uint64)
    return exp


def launch_all(ctx, c, base, d_out, at, stream=None, entries=rb.ENTRIES):
    d_pos, d_cls, d_t = base
    S = c.S
    pos = [d_pos + c.poff[k] for k in range(S)]
    cls = [d_cls + c.coff[k] for k in range(S)]
    tim = [d_t + c.toff[k] for k in range(S)]
    plain = [binding.make_columns(xyz=pos[k], n=c.n[k]) for k in range(S)]
    with_class = [binding.make_columns(xyz=pos[k], cls=cls[k], n=c.n[k]) for k in range(S)]
    with_time = [binding.make_columns(xyz=pos[k], cls=tim[k], n=c.n[k], cls_stride=8) for k in range(S)]
    only_class = [binding.make_columns(cls=cls[k], n=c.n[k]) for k in range(S)]
    out = {name: d_out + 8 * first for name, (first, words) in at.items()}
    P = pkg.Predicate

    def bounds(rows):
        return [P.bounds(r[0], r[1]) for r in rows]

    if "zsum" in entries and len(entries) == 1:
        ctx.scan_dev_zsum_raster_batch(plain, bounds(c.zsum), [r[2] for r in c.zsum], *c.zsum_dims, out["zcount"], out["zsum"], stream=stream)
        return
    assert tuple(entries) == rb.ENTRIES
    ctx.scan_dev_count_batch(plain, bounds(c.box["box"]), out["box"], stream=stream)
    ctx.scan_dev_count_batch(only_class, [P.classification(v) for v in c.cclass], out["class"], stream=stream)
    ctx.scan_dev_count_batch_combined(with_class, [P.bounds_class(lo, hi, v) for (lo, hi), v in zip(c.box["box_class"], c.qclass)],
                                      out["box_class"], stream=stream)
    ctx.scan_dev_count_batch_bounds_time(with_time, [P.bounds_time(lo, hi, *r) for (lo, hi), r in zip(c.box["box_time"], c.ranges)],
                                         out["box_time"], stream=stream)
    ctx.scan_dev_count_batch_multi(plain, [bounds(row) for row in c.multi], out["multi"], stream=stream)
    ctx.scan_dev_class_hist_batch(with_class, bounds(c.box["class_hist"]), out["class_hist"], stream=stream)
    ctx.scan_dev_time_hist_batch(with_time, bounds(c.box["time_hist"]), c.edges, out["time_hist"], stream=stream)
    ctx.scan_dev_raster_batch(plain, bounds(c.raster), [r[2] for r in c.raster], *c.raster_dims, out["raster"], stream=stream)
    ctx.scan_dev_zrange_raster_batch(plain, bounds(c.zrange), [r[2] for r in c.zrange], *c.zrange_dims, out["zmin"], out["zmax"],
                                     stream=stream)
    ctx.scan_dev_count_batch_polygon(plain, bounds(c.polygon), [r[2] for r in c.polygon], out["polygon"], stream=stream)
    ctx.scan_dev_zsum_raster_batch(plain, bounds(c.zsum), [r[2] for r in c.zsum], *c.zsum_dims, out["zcount"], out["zsum"], stream=stream)


def contributors(c, entry, word):
    if entry == "zsum":
        return np.flatnonzero(c.share[entry][0][:, word]).tolist()
    if entry == "zrange":
        zmin, zmax = c.share[entry]
        return np.flatnonzero(zmin[:, word] != I32_MAX).tolist()
    return np.flatnonzero(c.share[entry][:, word]).tolist()


def describe(c, got, exp, at):
    """What is wrong, entry by entry"""
    out = []
    covered = np.zeros(len(exp), dtype=bool)
    for e in rb.ENTRIES:
        if e == "zsum":
            for name in ("zcount", "zsum"):
                first, words = at[name]
                covered[first:first + words] = True
                g, w = got[first:first + words].view(np.int64), exp[first:first + words].view(np.int64)
                bad = np.flatnonzero(g != w)
                if len(bad):
                    out.append(f"zsum {name}: {len(bad)} of {words} words wrong, (word, got - want, segments) "
                               f"{[(int(b), int(g[b]) - int(w[b]), contributors(c, e, b)) for b in bad[:4]]}")
            continue
        if e == "zrange":
            cells = rb.words_of(c, e)
            for name in ("zmin", "zmax"):
                first, words = at[name]
                covered[first:first + words] = True
                g, w = got.view(np.int32)[2 * first:2 * first + cells], exp.view(np.int32)[2 * first:2 * first + cells]
                bad = np.flatnonzero(g != w)
                if len(bad):
                    out.append(f"zrange {name}: {len(bad)} of {cells} cells wrong, (cell, got, want, segments) "
                               f"{[(int(b), int(g[b]), int(w[b]), contributors(c, e, b)) for b in bad[:4]]}")
                tail = slice(2 * first + cells, 2 * (first + words))
                if not np.array_equal(got.view(np.int32)[tail], exp.view(np.int32)[tail]):
                    out.append(f"zrange {name}: the word behind the last cell changed")
            continue
        first, words = at[e]
        covered[first:first + words] = True
        g, w = got[first:first + words].astype(np.int64), exp[first:first + words].astype(np.int64)
        bad = np.flatnonzero(g != w)
        if len(bad):
            out.append(f"{e}: {len(bad)} of {words} words wrong, (word, got - want, segments) "
                       f"{[(int(b), int(g[b] - w[b]), contributors(c, e, b)) for b in bad[:4]]}")
    guards = np.flatnonzero(~covered & (got != exp))
    if len(guards):
        owner = {first: name for name, (first, words) in at.items()}
        starts = np.asarray(sorted(owner))
        near = [owner[int(starts[max(np.searchsorted(starts, g, side="right") - 1, 0)])] for g in guards[:4]]
        out.append(f"guard words changed: {guards[:4].tolist()} (at or behind the output of {near})")
    return out


def run_case(ctx, seed, stream=None, sync=None, entries=rb.ENTRIES):
    c = rb.case(seed)
    at, total = layout(c)
    pre = preset_words(c, total, at)
    exp = expected(c, pre, at, entries)
    blocks = [ctx.alloc(size + 64) for size in (c.psize, c.csize, c.tsize, 8 * total)]
    try:
        assert all(b % 16 == 0 for b in blocks)
        ctx.to_device(blocks[0], image(c.psize, c.poff, c.xyz, 12))
        ctx.to_device(blocks[1], image(c.csize, c.coff, c.cls, 1))
        ctx.to_device(blocks[2], image(c.tsize, c.toff, c.t, 8))
        ctx.to_device(blocks[3], pre)
        launch_all(ctx, c, blocks[:3], blocks[3], at, stream, entries)
        if sync is not None:
            sync()
        got = np.zeros(total, dtype=np.uint64)
        ctx.to_host(got, blocks[3])  # (waits for the context's stream)
    finally:
        for b in blocks:
            ctx.free(b)
    wrong = describe(c, got, exp, at)
    assert not wrong, (f"seed {seed} (PCQ_TEST_SEED_BASE {rb.SEED_BASE}): S {c.S}, n {c.n}, class phases {c.cphase}, time phases {c.tphase}, "
                       f"positions {c.dist}: " + "; ".join(wrong))
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("seed", rb.SEEDS)
def test_all_ten_entries_against_numpy(gpu_ctx, seed):
    run_case(gpu_ctx, seed)


@pytest.mark.parametrize("seed", rb.SEEDS)
@pytest.mark.parametrize("entry", ["zsum"])
def test_the_mean_height_raster_against_numpy(gpu_ctx, entry, seed):
    """The entry that joined later, alone: counts and z sums as int64 bit patterns, every other word of the buffer as it was"""
    run_case(gpu_ctx, seed, entries=(entry,))


def test_on_a_callers_stream(gpu_ctx):
    """Six of the seeds again, every launch on a stream of the caller's: the caller orders its outputs, so the stream is
    synchronised before the words are read"""
    import torch
    ts = torch.cuda.Stream()
    for seed in STREAM_SEEDS:
        run_case(gpu_ctx, seed, stream=ts.cuda_stream, sync=ts.synchronize)
    run_case(gpu_ctx, STREAM_SEEDS[0])  # (the last call of a test is on the context's own stream)
