"""Every batched entry on a caller's stream.

The context's scratch (segment table, partials) is ordered only by the stream its launches run on; pcq_scratch_stream keeps
one stream in flight per context by draining the previous stream when a call arrives on another one.  Here a launch of each
kind is held back on a caller's stream behind plain torch work, so that its table and partials are live and unread when the
next call of the same kind, with other predicates and other launch-level parameters, arrives on the context's own stream.
Without the drain the held launch would read the second call's table and share its partials: its region would hold another
number.  `assert not ts.query()` behind the held call is what makes the test say something: the call returned while the
stream was still busy (pcq_upload_segment_table: an unchanged table is not uploaded, and nothing waits).

The caller owns the ordering of its outputs (to_host waits for the context's stream only): the tests synchronise their
streams before they read.  Each test has a context of its own and ends with a call on that context's own stream.
"""
import sys
import time

import pytest

import _batch_all_kinds as ak
from _batch_all_kinds import KINDS, NAMES, SMALL

pytestmark = pytest.mark.gpu

ROTATION = 3 * len(KINDS)  # calls of the rotation, and a closing one behind them
FILLER_WORDS, FILLER_ADDS = 1 << 28, 256  # a chain of additions in place over 1 GiB of f32 (2 GiB of traffic each): about ninety milliseconds


def checked(dev, words, q, call, what):
    bad = dev.wrong(words[call], q, call)
    assert bad is None, f"{what} (region {call}, kind {NAMES[q.kind]}, visit {q.visit}): {bad}"


@pytest.mark.parametrize("kind", KINDS, ids=NAMES)
def test_a_held_launch_on_a_callers_stream_survives_the_next_call(kind):
    import torch
    began = time.perf_counter()
    first, changed = ak.query(kind, SMALL, 0), ak.query(kind, SMALL, 1)
    ak.check_not_vacuous(first), ak.check_not_vacuous(changed)
    # what the held launch would add if it read the changed call's table: the first call's launch-level parameters (nqueries,
    # edges, the raster's shape, the class set, which travels in the kernel's arguments; the polygon count's boxes) over the changed
    # predicates (the polygon count's outlines).  Every word of it differs from the right answer where the kind has one word per
    # query, some word elsewhere.
    misread = ak.query(kind, SMALL, first.visit, changed.visit)
    assert misread.words == first.words and (misread.want != first.want).any()
    if kind in (ak.ZRANGE, ak.ZSUM, ak.ZSUM_CLASSES):
        assert misread.args[2:] == first.args[2:] and [bytes(p) for p in misread.args[0]] == [bytes(p) for p in changed.args[0]]
    if kind == ak.ZSUM_CLASSES:  # (the changed call changes the set and the table)
        assert set(changed.args[4]) != set(first.args[4]) and [bytes(p) for p in changed.args[0]] != [bytes(p) for p in first.args[0]]
    if kind == ak.POLYGON:
        assert [bytes(p) for p in misread.args[0]] == [bytes(p) for p in first.args[0]] and misread.args[1] == changed.args[1] != first.args[1]
    if first.words <= 8:
        assert (misread.want != first.want).all(), (misread.want, first.want)
    if kind == ak.MULTI:  # (the rows of the changed call hold the same boxes in the slots the held instantiation reads)
        assert (changed.want[:first.words] == misread.want).all()
    A0, A, B, C, D = range(5)
    ctx = ak.pkg.Context(0)
    try:
        dev = ak.Dev(ctx, [first, first, changed, first, changed])
        try:
            # (a fold hides a wrong z behind a preset beyond it: the misread answer is another one in the held call's region too)
            assert (ak.expected(misread, dev.before(A)) != ak.expected(first, dev.before(A))).any()
            ts = torch.cuda.Stream()
            with torch.cuda.stream(ts):
                x = torch.zeros(FILLER_WORDS, device="cuda")
                x.add_(1.0)  # (the first one loads the kernel)
            dev.launch(first, A0, ts.cuda_stream)  # 1: the table travels, the partials grow
            ts.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            at2 = time.perf_counter()
            with torch.cuda.stream(ts):  # 2: the stream is busy
                t0.record()
                for _ in range(FILLER_ADDS):
                    x.add_(1.0)
                t1.record()
            dev.launch(first, A, ts.cuda_stream)  # 3: queued behind the filler, without a wait of the host's
            held = not ts.query()
            at3 = time.perf_counter()
            assert held, "the repeated call returned only when the stream had run empty: its launch was never held back"
            dev.launch(changed, B)  # 4: the same kind, another table, on the context's stream
            at4 = time.perf_counter()
            dev.launch(first, C, ts.cuda_stream)  # 5
            ts.synchronize()  # 6
            dev.launch(changed, D)  # (the last call of a test is on the context's own stream)
            words = dev.regions()
            filler = t0.elapsed_time(t1)
            print(f"\n{NAMES[kind]}: filler {filler:.1f} ms on the stream; host: step 2 to the end of step 3 {1e3 * (at3 - at2):.2f} ms, "
                  f"to the end of step 4 {1e3 * (at4 - at2):.1f} ms; test {time.perf_counter() - began:.2f} s", file=sys.stderr)
            checked(dev, words, first, A0, "the warm-up call on the caller's stream")
            checked(dev, words, first, A, "the call held back on the caller's stream")
            checked(dev, words, changed, B, "the changed call on the context's stream")
            checked(dev, words, first, C, "the first call again on the caller's stream")
            checked(dev, words, changed, D, "the changed call again on the context's stream")
            assert float(x[0]) == float(x[-1]) == 1.0 + FILLER_ADDS  # (the filler ran)
        finally:
            dev.free()
    finally:
        ctx.close()


def test_two_callers_streams_and_the_contexts_in_rotation():
    """36 calls, each kind once on each of two caller's streams and on the context's stream, a stream after another; nothing
    is read or synchronised by the test before the end"""
    import torch
    began = time.perf_counter()
    visits, queries = [0] * len(KINDS), []
    for call in range(ROTATION):
        kind = (call // 3 + call % 3) % len(KINDS)
        queries.append(ak.query(kind, call % 2, visits[kind]))
        visits[kind] += 1
    queries.append(ak.query(ak.BOX, SMALL, visits[ak.BOX]))  # (the last call of a test is on the context's own stream)
    assert all({queries[c].kind for c in range(r, ROTATION, 3)} == set(KINDS) for r in range(3))
    for q in queries:
        ak.check_not_vacuous(q)
    ctx = ak.pkg.Context(0)
    try:
        dev = ak.Dev(ctx, queries)
        try:
            streams = [torch.cuda.Stream(), torch.cuda.Stream(), None]
            for call, q in enumerate(queries):
                s = streams[call % 3] if call < ROTATION else None
                dev.launch(q, call, s.cuda_stream if s is not None else None)
            streams[0].synchronize(), streams[1].synchronize()
            words = dev.regions()
            failures = []
            for call, q in enumerate(queries):
                bad = dev.wrong(words[call], q, call)
                if bad is not None:
                    on = ("the first caller's stream", "the second caller's stream", "the context's stream")[call % 3 if call < ROTATION else 2]
                    failures.append(f"call {call}: kind {NAMES[q.kind]} after kind {NAMES[queries[call - 1].kind] if call else None}, "
                                    f"visit {q.visit}, set {('small', 'large')[q.set]}, on {on}: {bad}")
            assert not failures, f"{len(failures)} of {len(queries)} calls wrong, the first: {failures[0]}"
        finally:
            dev.free()
    finally:
        ctx.close()
    print(f"\nrotation: {time.perf_counter() - began:.2f} s", file=sys.stderr)
