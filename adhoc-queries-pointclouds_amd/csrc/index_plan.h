// index_plan.h — what an indexed scan of each predicate kind prunes with, and everything its host path decides from that
// (chunk_index.hip: indexed_scan).  Pure host arithmetic without a HIP include: tests/native/index_plan_driver.cpp compiles it
// with g++ alone.
#pragma once

#include <cstdint>

#include "pcq.h"

// The parts of an index object, as a mask.  Slot p of pcq_index::part holds the part with bit 1 << p.
enum { PART_BOXES = 1, PART_HIST = 2, PART_TIMES = 4 };
constexpr int INDEX_PARTS = 3;
constexpr int INDEX_PART_BITS[INDEX_PARTS] = {PART_BOXES, PART_HIST, PART_TIMES};  // (the order missing parts are built in)
constexpr int index_part_slot(int part) { return part >> 1; }
static_assert(index_part_slot(PART_BOXES) == 0 && index_part_slot(PART_HIST) == 1 && index_part_slot(PART_TIMES) == 2, "slot p holds bit 1 << p");

// Boxes and time records describe 4096 points, class histograms 65536; the buffer emit's count pass works in tiles of 2048.
constexpr uint64_t INDEX_BOUNDS_CHUNK = 4096, INDEX_CLASS_CHUNK = 65536, EMIT_TILE_POINTS = 2048;

struct IndexPlan {
    int parts;             // PART_* the kind prunes with; 0: the kind has no index (plain scan, all-zero statistics)
    int unit;              // the part whose chunks the grid and the statistics are in
    bool counts_on_build;  // one part: the call that builds it counts on its way (built = 1, scanned = chunks, no pruned pass);
                           // false (two parts): missing parts are built without a count, then the pruned pass always runs
    bool from_hist;        // a count is a sum of histogram bins added straight into the counter: no partials, no finish
    bool tiles_of_n;       // EmitIndex::covered_tiles = n / 2048 (whole tiles); false: chunks x 2
    bool tail;             // a count scans the ragged end behind the last whole chunk with pcq_scan_dev
    uint64_t tail_cls_w;   // ... whose `cls` moves on by this many bytes per point; 0: the tail has no `cls`
    bool live_only;        // a predicate that can match nothing (empty box, empty or NaN range) falls through as well
};
constexpr IndexPlan index_plan(int pred_kind) {
    switch (pred_kind) {
    case PCQ_PRED_BOUNDS: return {PART_BOXES, PART_BOXES, true, false, false, true, 0, false};
    case PCQ_PRED_CLASS: return {PART_HIST, PART_HIST, true, true, true, false, 0, false};
    case PCQ_PRED_BOUNDS_CLASS: return {PART_BOXES | PART_HIST, PART_BOXES, false, false, false, true, 1, false};
    case PCQ_PRED_TIME: return {PART_TIMES, PART_TIMES, true, false, false, true, 8, false};
    case PCQ_PRED_BOUNDS_TIME: return {PART_BOXES | PART_TIMES, PART_BOXES, false, false, false, true, 8, true};
    default: return {};  // (a world-space box among them)
    }
}

// The column a part describes; a part is kept for as long as this pointer and n stay the same.
inline const void *index_part_column(int part, const pcq_columns &cols) { return part == PART_BOXES ? cols.xyz : cols.cls; }

// What a part covers: packed, 16-byte aligned positions with at least one whole chunk; packed class bytes; packed f64 times,
// 16-byte aligned (two times per load), with at least one whole chunk.
inline bool index_part_covers(int part, const pcq_columns &cols) {
    switch (part) {
    case PART_BOXES: return cols.xyz_stride == 12 && ((uintptr_t)cols.xyz & 15) == 0 && cols.n >= INDEX_BOUNDS_CHUNK;
    case PART_HIST: return cols.cls && cols.cls_stride == 1 && cols.n > 0;
    case PART_TIMES: return cols.cls && cols.cls_stride == 8 && ((uintptr_t)cols.cls & 15) == 0 && cols.n >= INDEX_BOUNDS_CHUNK;
    default: return false;
    }
}
inline bool index_covers(const IndexPlan &pl, const pcq_columns &cols) {
    bool ok = pl.parts != 0;
    for (int part : INDEX_PART_BITS)
        if (pl.parts & part) ok = ok && index_part_covers(part, cols);
    return ok;
}

// Chunks of a part over n points: whole chunks of boxes and time records (the ragged end is the tail), every class chunk.
constexpr uint64_t index_chunks(int part, uint64_t n) {
    return part == PART_HIST ? (n + INDEX_CLASS_CHUNK - 1) / INDEX_CLASS_CHUNK : n / INDEX_BOUNDS_CHUNK;
}
constexpr uint64_t index_covered_tiles(const IndexPlan &pl, uint64_t n) {
    return pl.tiles_of_n ? n / EMIT_TILE_POINTS : index_chunks(pl.unit, n) * (INDEX_BOUNDS_CHUNK / EMIT_TILE_POINTS);
}

// The columns of the ragged end from point `rest_first` on: its positions (when there are any), ITS class bytes or times, no colour.
inline pcq_columns index_tail_columns(const IndexPlan &pl, const pcq_columns &cols, uint64_t rest_first) {
    pcq_columns tail = cols;
    tail.xyz = cols.xyz ? (const uint8_t *)cols.xyz + 12 * rest_first : nullptr;
    tail.cls = pl.tail_cls_w ? (const uint8_t *)cols.cls + pl.tail_cls_w * rest_first : nullptr;
    if (pl.tail_cls_w) tail.cls_stride = pl.tail_cls_w;
    tail.rgb = nullptr;
    tail.n = cols.n - rest_first;
    return tail;
}
