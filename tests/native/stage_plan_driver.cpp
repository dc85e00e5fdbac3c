// The staging plan of the host / file scans (csrc/stage_plan.h), checked on the CPU: for every predicate kind x collector
// kind x layout x n x chunk_points the plan's invariants, and six plans pinned to numbers worked out by hand.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "stage_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures++ < 20) {                        \
                fprintf(stderr, "FAILED %s: ", #cond);    \
                fprintf(stderr, __VA_ARGS__);             \
                fprintf(stderr, "\n");                    \
            }                                             \
        }                                                 \
    } while (0)

// What pcq_validate_scan requires (include/pcq.h, pcq_columns and pcq_predicate), restated kind by kind.
struct Needs {
    bool xyz, cls, rgb;
    uint64_t w;
};
static Needs required(int kind, int coll, bool rgb_given) {
    const bool records = coll != COLL_COUNT;
    switch (kind) {
    case PCQ_PRED_BOUNDS:
    case PCQ_PRED_BOUNDS_F64: return {true, records, records && rgb_given, 1};
    case PCQ_PRED_CLASS: return {records, true, records && rgb_given, 1};
    case PCQ_PRED_TIME: return {records, true, false, 8};          // "the time column is always required; the positions only for buffer and grid collectors"
    case PCQ_PRED_BOUNDS_CLASS: return {true, true, records && rgb_given, 1};  // "both always read, even for a count"
    default: return {true, true, false, 8};                       // PCQ_PRED_BOUNDS_TIME; `rgb` is ignored
    }
}

static uint64_t up4(uint64_t v) { return (v + 3) & ~3ull; }

static void check_plan(const pcq_columns &cols, int kind, int coll, uint64_t chunk_points, bool las, const char *what) {
    const StagePlan pl = stage_plan(cols, kind, coll, chunk_points);
    const Needs rq = required(kind, coll, cols.rgb != nullptr);
    const ScanNeeds sn = scan_needs(kind, coll);
    CHECK(sn.xyz == rq.xyz && sn.cls == rq.cls && (sn.rgb && cols.rgb) == rq.rgb && sn.cls_w == rq.w, "%s kind %d coll %d", what, kind, coll);
    CHECK(pl.ok, "%s kind %d coll %d: refused", what, kind, coll);
    if (!pl.ok) return;
    CHECK(pl.need_xyz == rq.xyz && pl.need_cls == rq.cls && pl.need_rgb == rq.rgb && pl.w == rq.w, "%s kind %d coll %d", what, kind, coll);
    CHECK(pl.aos == las, "%s kind %d coll %d: aos %d", what, kind, coll, (int)pl.aos);
    const uint64_t n = cols.n, chunk = pl.chunk;
    CHECK(chunk % 4 == 0 && chunk >= 4 && chunk <= (up4(n) > 4 ? up4(n) : 4), "%s: chunk %" PRIu64 " n %" PRIu64, what, chunk, n);
    CHECK(chunk * pl.bytes_per_point <= (512ull << 20), "%s: chunk bytes", what);
    CHECK(pl.stage_need >= pl.bytes(chunk), "%s: stage_need %zu < %zu", what, pl.stage_need, pl.bytes(chunk));
    const uint64_t last = n % chunk ? n % chunk : (n < chunk ? n : chunk);
    for (uint64_t cnt : {n < chunk ? n : chunk, last}) {
        if (pl.aos) {
            // the needed columns of the records [0, cnt): from the lowest needed pointer to the last needed byte of the last record
            uintptr_t lo = UINTPTR_MAX, hi = 0;
            auto col = [&](const void *p, uint64_t sz) {
                const uintptr_t a = (uintptr_t)p;
                if (a < lo) lo = a;
                if (a + sz > hi) hi = a + sz;
            };
            if (rq.xyz) col(cols.xyz, 12);
            if (rq.cls) col(cols.cls, rq.w);
            if (rq.rgb) col(cols.rgb, 6);
            CHECK(pl.aos_base == lo, "%s: aos base", what);
            CHECK(pl.bytes(cnt) == (cnt - 1) * pl.stride + (hi - lo), "%s: aos bytes %zu", what, pl.bytes(cnt));
            CHECK(pl.bytes(cnt) <= cnt * pl.stride, "%s: aos transfer runs behind the last record", what);
        } else {
            CHECK(pl.off_xyz % 16 == 0 && pl.off_cls % 16 == 0 && pl.off_rgb % 16 == 0, "%s: region alignment", what);
            size_t end = 0;  // regions in the order xyz < cls < rgb, each behind the one before
            if (rq.xyz) {
                CHECK(pl.off_xyz >= end, "%s: xyz region", what);
                end = pl.off_xyz + cnt * 12;
            }
            if (rq.cls) {
                CHECK(pl.off_cls >= end && pl.off_cls >= (rq.xyz ? pl.off_xyz + chunk * 12 : 0), "%s: cls region overlaps xyz", what);
                end = pl.off_cls + cnt * rq.w;
            }
            if (rq.rgb) {
                CHECK(pl.off_rgb >= end && pl.off_rgb >= pl.off_cls + (rq.cls ? chunk * rq.w : 0), "%s: rgb region overlaps cls", what);
                end = pl.off_rgb + cnt * 6;
            }
            CHECK(pl.bytes(cnt) == end, "%s: transfer of %zu bytes, last needed region ends at %zu", what, pl.bytes(cnt), end);
        }
    }
}

static pcq_columns last_cols(uint64_t n, uint64_t cls_stride, bool rgb) {
    pcq_columns c{};
    const uintptr_t base = 0x10000;  // (only the differences matter: the plan never reads through the pointers)
    c.xyz = (const void *)base;
    c.cls = (const void *)(base + 15 * n + 3);
    c.rgb = rgb ? (const void *)(base + 20 * n) : nullptr;
    c.xyz_stride = 12, c.cls_stride = cls_stride, c.rgb_stride = 6, c.n = n;
    return c;
}
static pcq_columns las_cols(uint64_t n, uint64_t reclen, bool time, bool rgb) {
    pcq_columns c{};
    const uintptr_t base = 0x10000 + 227;
    c.xyz = (const void *)base;
    c.cls = (const void *)(base + (time ? 20 : 15));
    c.rgb = rgb ? (const void *)(base + (reclen == 26 ? 20 : 28)) : nullptr;
    c.xyz_stride = c.cls_stride = c.rgb_stride = reclen, c.n = n;
    return c;
}

int main() {
    const int kinds[] = {PCQ_PRED_BOUNDS, PCQ_PRED_CLASS, PCQ_PRED_BOUNDS_F64, PCQ_PRED_TIME, PCQ_PRED_BOUNDS_CLASS, PCQ_PRED_BOUNDS_TIME};
    const int colls[] = {COLL_COUNT, COLL_BUFFER, COLL_GRID};
    long plans = 0;
    for (uint64_t cp : {(uint64_t)4, (uint64_t)4096, (uint64_t)1 << 20}) {
        for (uint64_t n : {(uint64_t)1, (uint64_t)3, (uint64_t)4, (uint64_t)5, cp - 1, cp, cp + 1, 2 * cp + 1}) {
            for (int kind : kinds)
                for (int coll : colls) {
                    const bool time = pred_tests_time(kind);
                    for (int rgb = 0; rgb < 2; rgb++) {
                        check_plan(last_cols(n, time ? 8 : 1, rgb), kind, coll, cp, false, "LAST"), plans++;
                        for (uint64_t reclen : {20, 26, 28, 34}) {
                            if (time && reclen != 28 && reclen != 34) continue;  // (formats 0 and 2 have no GPS time)
                            if (rgb && reclen != 26 && reclen != 34) continue;   // (formats 0 and 1 have no colour)
                            check_plan(las_cols(n, reclen, time, rgb), kind, coll, cp, true, "LAS"), plans++;
                        }
                    }
                }
        }
        // chunk_points counts 12-byte positions: a class-only count (1 B per point) takes 12 x the points per chunk of a bounds
        // count, a time count (8 B) 1.5 x — in whole multiples of 4 points
        const uint64_t big = 100 * cp;
        const uint64_t cb = stage_plan(last_cols(big, 1, false), PCQ_PRED_BOUNDS, COLL_COUNT, cp).chunk;
        CHECK(stage_plan(last_cols(big, 1, false), PCQ_PRED_CLASS, COLL_COUNT, cp).chunk == 12 * cb, "class count chunk, chunk_points %" PRIu64, cp);
        CHECK(stage_plan(last_cols(big, 8, false), PCQ_PRED_TIME, COLL_COUNT, cp).chunk == up4(cb * 3 / 2), "time count chunk, chunk_points %" PRIu64, cp);
    }
    // columns that are neither packed nor one record are refused
    {
        pcq_columns c = last_cols(100, 1, false);
        c.cls_stride = 2;
        CHECK(!stage_plan(c, PCQ_PRED_BOUNDS, COLL_BUFFER, 4096).ok, "strided class column accepted");
        CHECK(stage_plan(c, PCQ_PRED_BOUNDS, COLL_COUNT, 4096).ok, "a count does not read the class column");
    }

    // Six plans by hand, from scan_host_impl as it stood before the plan was split off; chunk_points = 2^20, so a chunk is
    // B = 2^20 * 12 = 12582912 bytes of columns; n = 40 000 000 (more than every chunk below).  With p = bytes per point:
    // chunk = floor(B / p) rounded up to a multiple of 4; stage_need = chunk * p + 64; regions: xyz at 0, cls behind
    // align16(chunk * 12) when positions are staged, rgb behind align16(chunk * w) more.
    const uint64_t N = 40000000, CP = (uint64_t)1 << 20;
    {   // LAST bounds count: positions only, p = 12: chunk = 1048576; a chunk's transfer = 12 * cnt
        const StagePlan p = stage_plan(last_cols(N, 1, true), PCQ_PRED_BOUNDS, COLL_COUNT, CP);
        CHECK(p.ok && !p.aos && p.need_xyz && !p.need_cls && !p.need_rgb && p.bytes_per_point == 12 && p.chunk == 1048576 && p.stage_need == 12582976 &&
              p.off_xyz == 0 && p.bytes(1048576) == 12582912 && p.bytes(5) == 60, "LAST bounds count");
    }
    {   // LAST bounds buffer with colour: p = 12 + 1 + 6 = 19: floor(12582912 / 19) = 662258 -> 662260; stage_need = 662260 * 19 + 64;
        // cls at 662260 * 12 = 7947120 (a multiple of 16), rgb at 7947120 + align16(662260) = 7947120 + 662272 = 8609392;
        // a whole chunk's transfer ends at 8609392 + 662260 * 6 = 12582952
        const StagePlan p = stage_plan(last_cols(N, 1, true), PCQ_PRED_BOUNDS, COLL_BUFFER, CP);
        CHECK(p.ok && !p.aos && p.need_xyz && p.need_cls && p.need_rgb && p.w == 1 && p.bytes_per_point == 19 && p.chunk == 662260 &&
              p.stage_need == 12583004 && p.off_xyz == 0 && p.off_cls == 7947120 && p.off_rgb == 8609392 && p.bytes(662260) == 12582952 &&
              p.bytes(7) == 8609392 + 42, "LAST bounds buffer with colour");
    }
    {   // LAST class count: class bytes only, p = 1: chunk = 12582912 (12 x the bounds count's), at offset 0; transfer = cnt
        const StagePlan p = stage_plan(last_cols(N, 1, true), PCQ_PRED_CLASS, COLL_COUNT, CP);
        CHECK(p.ok && !p.aos && !p.need_xyz && p.need_cls && !p.need_rgb && p.w == 1 && p.bytes_per_point == 1 && p.chunk == 12582912 &&
              p.stage_need == 12582976 && p.off_cls == 0 && p.bytes(12582912) == 12582912 && p.bytes(3) == 3, "LAST class count");
    }
    {   // LAST time count: f64 times only, p = 8: chunk = 1572864 (1.5 x), at offset 0; transfer = 8 * cnt
        const StagePlan p = stage_plan(last_cols(N, 8, false), PCQ_PRED_TIME, COLL_COUNT, CP);
        CHECK(p.ok && !p.aos && !p.need_xyz && p.need_cls && !p.need_rgb && p.w == 8 && p.bytes_per_point == 8 && p.chunk == 1572864 &&
              p.stage_need == 12582976 && p.off_cls == 0 && p.bytes(1572864) == 12582912 && p.bytes(3) == 24, "LAST time count");
    }
    {   // LAST bounds+time grid: positions and times, no colour even when one is given, p = 20: floor(12582912 / 20) = 629145 -> 629148;
        // stage_need = 629148 * 20 + 64; times at 629148 * 12 = 7549776 (a multiple of 16); a whole chunk ends at 7549776 + 629148 * 8
        const StagePlan p = stage_plan(last_cols(N, 8, true), PCQ_PRED_BOUNDS_TIME, COLL_GRID, CP);
        CHECK(p.ok && !p.aos && p.need_xyz && p.need_cls && !p.need_rgb && p.w == 8 && p.bytes_per_point == 20 && p.chunk == 629148 &&
              p.stage_need == 12583024 && p.off_cls == 7549776 && p.bytes(629148) == 12582960 && p.bytes(1) == 7549776 + 8, "LAST bounds+time grid");
    }
    {   // LAS format 3 (34-byte records: xyz + 0, class + 15, colour + 28) bounds buffer: one interleaved range from the positions to
        // the end of the colour, span 34, p = 34: floor(12582912 / 34) = 370085 -> 370088; stage_need = 370088 * 34 + 64; transfer = 34 * cnt
        const pcq_columns c = las_cols(N, 34, false, true);
        const StagePlan p = stage_plan(c, PCQ_PRED_BOUNDS, COLL_BUFFER, CP);
        CHECK(p.ok && p.aos && p.need_xyz && p.need_cls && p.need_rgb && p.aos_base == (uintptr_t)c.xyz && p.stride == 34 && p.span == 34 &&
              p.bytes_per_point == 34 && p.chunk == 370088 && p.stage_need == 12583056 && p.bytes(370088) == 12582992 && p.bytes(2) == 68,
              "LAS format 3 bounds buffer");
        // (format 1, 28-byte records without colour: the range ends behind the class byte, 16 bytes into the last record)
        const StagePlan q = stage_plan(las_cols(N, 28, false, false), PCQ_PRED_BOUNDS, COLL_BUFFER, CP);
        CHECK(q.ok && q.aos && q.span == 16 && q.bytes(10) == 9 * 28 + 16, "LAS format 1 bounds buffer");
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("ok %ld plans\n", plans);
    return 0;
}
