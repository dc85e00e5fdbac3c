// The plan of the indexed scans (csrc/index_plan.h), checked on the CPU: for every predicate kind the parts it prunes with,
// what the index covers at the edges of its layouts, the chunk counts, and the columns of the ragged tail against numbers
// worked out by hand from the table in chunk_index.hip.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "index_plan.h"

static int failures = 0;
static long cases = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        cases++;                                          \
        if (!(cond)) {                                    \
            if (failures++ < 20) {                        \
                fprintf(stderr, "FAILED %s: ", #cond);    \
                fprintf(stderr, __VA_ARGS__);             \
                fprintf(stderr, "\n");                    \
            }                                             \
        }                                                 \
    } while (0)

static const uintptr_t XYZ = 0x100000, CLS = 0x900000;  // both 16-byte aligned; the plan never reads through the pointers

static pcq_columns columns(uint64_t n, uintptr_t xyz, uint64_t xyz_stride, uintptr_t cls, uint64_t cls_stride) {
    pcq_columns c{};
    c.xyz = (const void *)xyz, c.cls = (const void *)cls, c.rgb = (const void *)0x1f00000;
    c.xyz_stride = xyz_stride, c.cls_stride = cls_stride, c.rgb_stride = 6, c.n = n;
    return c;
}

// The table, restated kind by kind: which layouts are covered ...
static bool boxes_ok(const pcq_columns &c) { return c.xyz_stride == 12 && (uintptr_t)c.xyz % 16 == 0 && c.n >= 4096; }
static bool hist_ok(const pcq_columns &c) { return c.cls != nullptr && c.cls_stride == 1 && c.n != 0; }
static bool times_ok(const pcq_columns &c) { return c.cls != nullptr && c.cls_stride == 8 && (uintptr_t)c.cls % 16 == 0 && c.n >= 4096; }
static bool covered(int kind, const pcq_columns &c) {
    switch (kind) {
    case PCQ_PRED_BOUNDS: return boxes_ok(c);
    case PCQ_PRED_CLASS: return hist_ok(c);
    case PCQ_PRED_BOUNDS_CLASS: return boxes_ok(c) && hist_ok(c);
    case PCQ_PRED_TIME: return times_ok(c);
    case PCQ_PRED_BOUNDS_TIME: return boxes_ok(c) && times_ok(c);
    default: return false;
    }
}

int main() {
    const int kinds[] = {PCQ_PRED_BOUNDS, PCQ_PRED_CLASS, PCQ_PRED_BOUNDS_F64, PCQ_PRED_TIME, PCQ_PRED_BOUNDS_CLASS, PCQ_PRED_BOUNDS_TIME};

    // the parts, the unit of the statistics, who counts on the building call
    struct Row {
        int kind, parts, unit;
        bool counts_on_build, from_hist, tiles_of_n, tail;
        uint64_t tail_cls_w;
        bool live_only;
    };
    const Row rows[] = {
        {PCQ_PRED_BOUNDS, PART_BOXES, PART_BOXES, true, false, false, true, 0, false},
        {PCQ_PRED_CLASS, PART_HIST, PART_HIST, true, true, true, false, 0, false},
        {PCQ_PRED_BOUNDS_CLASS, PART_BOXES | PART_HIST, PART_BOXES, false, false, false, true, 1, false},
        {PCQ_PRED_TIME, PART_TIMES, PART_TIMES, true, false, false, true, 8, false},
        {PCQ_PRED_BOUNDS_TIME, PART_BOXES | PART_TIMES, PART_BOXES, false, false, false, true, 8, true},
        {PCQ_PRED_BOUNDS_F64, 0, 0, false, false, false, false, 0, false},
    };
    for (const Row &r : rows) {
        const IndexPlan p = index_plan(r.kind);
        CHECK(p.parts == r.parts && p.unit == r.unit, "kind %d: parts %d unit %d", r.kind, p.parts, p.unit);
        CHECK(p.counts_on_build == r.counts_on_build && p.from_hist == r.from_hist && p.tiles_of_n == r.tiles_of_n, "kind %d: count path", r.kind);
        CHECK(p.tail == r.tail && p.tail_cls_w == r.tail_cls_w && p.live_only == r.live_only, "kind %d: tail", r.kind);
        // one part <=> the building call counts on its way; the unit is one of the parts
        const int nparts = !!(p.parts & PART_BOXES) + !!(p.parts & PART_HIST) + !!(p.parts & PART_TIMES);
        CHECK(p.counts_on_build == (nparts == 1) && (p.parts == 0 || (p.parts & p.unit) == p.unit), "kind %d: %d parts", r.kind, nparts);
    }
    CHECK(index_plan(12345).parts == 0 && !index_covers(index_plan(12345), columns(1 << 20, XYZ, 12, CLS, 1)), "an unknown kind has no index");
    CHECK(index_part_slot(PART_BOXES) == 0 && index_part_slot(PART_HIST) == 1 && index_part_slot(PART_TIMES) == 2, "slots");
    {
        const pcq_columns c = columns(5000, XYZ, 12, CLS, 1);
        CHECK(index_part_column(PART_BOXES, c) == c.xyz && index_part_column(PART_HIST, c) == c.cls && index_part_column(PART_TIMES, c) == c.cls,
              "the column a part is keyed on");
    }

    // index_covers at its edges
    for (int kind : kinds) {
        const IndexPlan p = index_plan(kind);
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)100, (uint64_t)4095, (uint64_t)4096, (uint64_t)4097, (uint64_t)70000})
            for (uintptr_t xoff : {0, 4, 8})
                for (uint64_t xs : {12, 34})
                    for (uintptr_t coff : {0, 4, 8})
                        for (uint64_t cs : {1, 8, 34})
                            for (int null_cls = 0; null_cls < 2; null_cls++) {
                                const pcq_columns c = columns(n, XYZ + xoff, xs, null_cls ? 0 : CLS + coff, cs);
                                CHECK(index_covers(p, c) == covered(kind, c),
                                      "kind %d n %" PRIu64 " xyz +%d stride %" PRIu64 " cls %s+%d stride %" PRIu64, kind, n, (int)xoff, xs,
                                      null_cls ? "null " : "", (int)coff, cs);
                            }
    }
    // ... a few of them spelled out
    CHECK(!index_covers(index_plan(PCQ_PRED_BOUNDS), columns(4095, XYZ, 12, 0, 1)) && index_covers(index_plan(PCQ_PRED_BOUNDS), columns(4096, XYZ, 12, 0, 1)),
          "bounds: one whole chunk, the class column does not matter");
    CHECK(!index_covers(index_plan(PCQ_PRED_BOUNDS), columns(4096, XYZ + 4, 12, 0, 1)), "bounds: positions 4 bytes off alignment");
    CHECK(index_covers(index_plan(PCQ_PRED_CLASS), columns(1, XYZ + 4, 34, CLS + 3, 1)) && !index_covers(index_plan(PCQ_PRED_CLASS), columns(0, XYZ, 12, CLS, 1)) &&
              !index_covers(index_plan(PCQ_PRED_CLASS), columns(100, XYZ, 12, CLS, 34)),
          "class: any alignment, any positions, n > 0, packed");
    CHECK(index_covers(index_plan(PCQ_PRED_TIME), columns(4096, 0, 12, CLS, 8)) && !index_covers(index_plan(PCQ_PRED_TIME), columns(4096, 0, 12, CLS + 8, 8)),
          "time: positions may be null, times 16-byte aligned");
    CHECK(!index_covers(index_plan(PCQ_PRED_BOUNDS_CLASS), columns(4096, XYZ, 12, 0, 1)) && !index_covers(index_plan(PCQ_PRED_BOUNDS_TIME), columns(4096, XYZ, 12, CLS, 1)),
          "two parts: both must be covered");

    // index_chunks: whole chunks of 4096 for boxes and time records, every chunk of 65536 for histograms
    {
        const uint64_t ns[] = {0, 1, 4095, 4096, 4097, 65535, 65536, 65537};
        const uint64_t whole[] = {0, 0, 0, 1, 1, 15, 16, 16}, cls[] = {0, 1, 1, 1, 1, 1, 1, 2};
        for (int i = 0; i < 8; i++) {
            CHECK(index_chunks(PART_BOXES, ns[i]) == whole[i] && index_chunks(PART_TIMES, ns[i]) == whole[i], "n %" PRIu64, ns[i]);
            CHECK(index_chunks(PART_HIST, ns[i]) == cls[i], "n %" PRIu64 ": %" PRIu64 " class chunks", ns[i], index_chunks(PART_HIST, ns[i]));
            // tiles of 2048 the buffer emit takes from the index: two per whole chunk; a class scan alone: the whole tiles of n
            CHECK(index_covered_tiles(index_plan(PCQ_PRED_BOUNDS), ns[i]) == 2 * whole[i] && index_covered_tiles(index_plan(PCQ_PRED_TIME), ns[i]) == 2 * whole[i] &&
                      index_covered_tiles(index_plan(PCQ_PRED_BOUNDS_CLASS), ns[i]) == 2 * whole[i] &&
                      index_covered_tiles(index_plan(PCQ_PRED_BOUNDS_TIME), ns[i]) == 2 * whole[i],
                  "covered tiles, n %" PRIu64, ns[i]);
            CHECK(index_covered_tiles(index_plan(PCQ_PRED_CLASS), ns[i]) == ns[i] / 2048, "covered tiles of a class scan, n %" PRIu64, ns[i]);
        }
        CHECK(index_covered_tiles(index_plan(PCQ_PRED_CLASS), 65537) == 32 && index_covered_tiles(index_plan(PCQ_PRED_BOUNDS), 65537) == 32 &&
                  index_covered_tiles(index_plan(PCQ_PRED_CLASS), 6143) == 2 && index_covered_tiles(index_plan(PCQ_PRED_BOUNDS), 8191) == 2 &&
                  index_covered_tiles(index_plan(PCQ_PRED_CLASS), 8191) == 3,
              "covered tiles by hand");
    }

    // The ragged tail.  n = 4096: one whole chunk, nothing behind it.  n = 4097: one point from 4096 on.  n = 8191: still one whole
    // chunk, 4095 points behind it.  Positions move on by 12 * 4096 = 49152 = 0xc000 bytes, class bytes by 4096 = 0x1000, times by
    // 8 * 4096 = 32768 = 0x8000.
    for (uint64_t n : {(uint64_t)4096, (uint64_t)4097, (uint64_t)8191}) {
        const uint64_t first = 4096, rest = n - first;
        for (int kind : {PCQ_PRED_BOUNDS, PCQ_PRED_BOUNDS_CLASS, PCQ_PRED_TIME, PCQ_PRED_BOUNDS_TIME}) {
            const IndexPlan p = index_plan(kind);
            CHECK(p.tail && index_chunks(p.unit, n) * INDEX_BOUNDS_CHUNK == first, "kind %d n %" PRIu64 ": the tail starts at 4096", kind, n);
        }
        if (rest == 0) continue;  // (rest_first == n: the driver scans no tail)
        {   // BOUNDS: xyz + 12 * rest_first; cls and rgb null
            const pcq_columns t = index_tail_columns(index_plan(PCQ_PRED_BOUNDS), columns(n, XYZ, 12, CLS, 1), first);
            CHECK((uintptr_t)t.xyz == 0x10c000 && t.xyz_stride == 12 && t.cls == nullptr && t.rgb == nullptr && t.n == rest, "bounds tail, n %" PRIu64, n);
        }
        {   // BOUNDS_CLASS: xyz + 12 * rest_first, cls + rest_first, cls_stride 1
            const pcq_columns t = index_tail_columns(index_plan(PCQ_PRED_BOUNDS_CLASS), columns(n, XYZ, 12, CLS + 3, 1), first);
            CHECK((uintptr_t)t.xyz == 0x10c000 && (uintptr_t)t.cls == 0x901003 && t.cls_stride == 1 && t.rgb == nullptr && t.n == rest,
                  "box AND class tail, n %" PRIu64, n);
        }
        {   // TIME: cls + 8 * rest_first; xyz + 12 * rest_first when there are positions
            const pcq_columns t = index_tail_columns(index_plan(PCQ_PRED_TIME), columns(n, XYZ, 12, CLS, 8), first);
            CHECK((uintptr_t)t.xyz == 0x10c000 && (uintptr_t)t.cls == 0x908000 && t.cls_stride == 8 && t.rgb == nullptr && t.n == rest, "time tail, n %" PRIu64, n);
            const pcq_columns u = index_tail_columns(index_plan(PCQ_PRED_TIME), columns(n, 0, 12, CLS, 8), first);
            CHECK(u.xyz == nullptr && (uintptr_t)u.cls == 0x908000 && u.n == rest, "time tail without positions, n %" PRIu64, n);
        }
        {   // BOUNDS_TIME: xyz + 12 * rest_first, cls + 8 * rest_first
            const pcq_columns t = index_tail_columns(index_plan(PCQ_PRED_BOUNDS_TIME), columns(n, XYZ, 12, CLS, 8), first);
            CHECK((uintptr_t)t.xyz == 0x10c000 && (uintptr_t)t.cls == 0x908000 && t.cls_stride == 8 && t.rgb == nullptr && t.n == rest,
                  "box AND time tail, n %" PRIu64, n);
        }
    }
    CHECK(!index_plan(PCQ_PRED_CLASS).tail, "a class count has no tail: the last histogram holds the ragged end");

    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("ok %ld cases\n", cases);
    return 0;
}
