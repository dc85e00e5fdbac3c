// stage_plan.h — what a scan reads, and how a host / file scan lays it out in the staging ring (host_stream.hip).
// Pure host arithmetic without a HIP include: tests/native/stage_plan_driver.cpp compiles it with g++ alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "pcq.h"

#ifndef __host__  // (a host-only compiler: the kind helpers below are shared with the kernels)
#define __host__
#define __device__
#endif

enum { COLL_COUNT = 0, COLL_BUFFER = 1, COLL_GRID = 2 };

// The kinds by what they test.  The combined kinds (PCQ_PRED_BOUNDS_CLASS / _TIME) test the integer box (lo, width, empty)
// AND the attribute in pcq_columns.cls: a class byte or an f64 GPS time.
__host__ __device__ constexpr bool pred_has_box(int k) { return k == PCQ_PRED_BOUNDS || k == PCQ_PRED_BOUNDS_CLASS || k == PCQ_PRED_BOUNDS_TIME; }
__host__ __device__ constexpr bool pred_is_combined(int k) { return k == PCQ_PRED_BOUNDS_CLASS || k == PCQ_PRED_BOUNDS_TIME; }
__host__ __device__ constexpr bool pred_tests_time(int k) { return k == PCQ_PRED_TIME || k == PCQ_PRED_BOUNDS_TIME; }

// Which columns a scan of predicate kind `k` into a collector of kind `coll` reads (pcq_validate_scan requires exactly these,
// the staging plan moves exactly these).  The predicate's own column ("cls") is a class byte or an f64 GPS time — read by every
// scan of that kind; the combined kinds read it and the positions; buffer and grid collectors build a record from every column,
// but a time record has no colour (las.rs:345-355).
struct ScanNeeds {
    bool xyz, cls;
    bool rgb;        // when the caller gives one
    uint64_t cls_w;  // bytes per point of the predicate's column
};
constexpr ScanNeeds scan_needs(int k, int coll) {
    const bool time = pred_tests_time(k), records = coll != COLL_COUNT;
    const bool pred_col = k == PCQ_PRED_CLASS || time || pred_is_combined(k);
    return ScanNeeds{!pred_col || pred_is_combined(k) || records, pred_col || records, records && !time, time ? 8u : 1u};
}

constexpr size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct StagePlan {
    bool ok;                   // false: the columns are neither packed blocks (LAST) nor one interleaved record (LAS)
    bool aos;                  // LAS records: one interleaved range
    bool need_xyz, need_cls, need_rgb;
    uint64_t w;                // bytes per point of the predicate's column
    uint64_t bytes_per_point;  // staged bytes per point (without per-region alignment slack)
    uintptr_t aos_base;        // lowest needed column pointer of the first record
    uint64_t stride;           // aos stride
    uint64_t span;             // bytes from aos_base to the end of the last needed column of a record
    uint64_t chunk;            // points per chunk
    size_t off_xyz, off_cls, off_rgb;  // region offsets inside a staging buffer (SoA case)
    size_t stage_need;         // bytes a staging buffer must hold

    // bytes of a staging buffer that a chunk of `cnt` points fills (what is transferred)
    size_t bytes(uint64_t cnt) const {
        // AoS: up to the last needed byte of the last record (never past the caller's mapping)
        if (aos) return (size_t)((cnt - 1) * stride + span);
        if (need_rgb) return off_rgb + (size_t)cnt * 6;
        if (need_cls) return off_cls + (size_t)cnt * w;
        return (size_t)cnt * 12;
    }
};

// The column "pointers" of `cols` are host addresses or byte offsets into a file: only their differences matter here.
inline StagePlan stage_plan(const pcq_columns &cols, int pred_kind, int coll_kind, uint64_t chunk_points) {
    StagePlan pl{};
    const ScanNeeds need = scan_needs(pred_kind, coll_kind);
    const uint64_t w = pl.w = need.cls_w;
    pl.need_xyz = need.xyz;
    pl.need_cls = need.cls;
    pl.need_rgb = need.rgb && cols.rgb != nullptr;
    const uintptr_t hx = (uintptr_t)cols.xyz, hc = (uintptr_t)cols.cls, hr = (uintptr_t)cols.rgb;
    // AoS (LAS): every needed column has the same stride and lives inside one record
    {
        const uint64_t st = pl.need_xyz ? cols.xyz_stride : cols.cls_stride;
        bool same = st > 12 || (!pl.need_xyz && st > w);
        if (pl.need_xyz && cols.xyz_stride != st) same = false;
        if (pl.need_cls && cols.cls_stride != st) same = false;
        if (pl.need_rgb && cols.rgb_stride != st) same = false;
        bool any = false;
        uintptr_t lo = 0, hi = 0;
        auto upd = [&](uintptr_t p, uint64_t sz) {
            if (!any || p < lo) lo = p;
            if (!any || p + sz > hi) hi = p + sz;
            any = true;
        };
        if (pl.need_xyz) upd(hx, 12);
        if (pl.need_cls) upd(hc, w);
        if (pl.need_rgb) upd(hr, 6);
        if (same && any && (uint64_t)(hi - lo) <= st && st > 1) {
            pl.aos = true;
            pl.aos_base = lo;
            pl.stride = st;
            pl.span = (uint64_t)(hi - lo);
            pl.bytes_per_point = st;
        }
    }
    if (!pl.aos) {
        if ((pl.need_xyz && cols.xyz_stride != 12) || (pl.need_cls && cols.cls_stride != w) || (pl.need_rgb && cols.rgb_stride != 6))
            return pl;  // (ok = false)
        pl.bytes_per_point = (pl.need_xyz ? 12 : 0) + (pl.need_cls ? w : 0) + (pl.need_rgb ? 6 : 0);
    }
    pl.ok = true;

    // "chunk_points" is given in points of a positions column (12 B each); what matters to the pipeline is the BYTES per
    // chunk, so a class-only scan (1 B per point) takes 12 x as many points per chunk, a time count (8 B) 1.5 x, and a
    // record scan of a wide LAS format fewer — otherwise a class query would move 2 MB per chunk and drown in per-chunk overhead
    uint64_t chunk = chunk_points * 12 / (pl.bytes_per_point ? pl.bytes_per_point : 1);
    if (chunk < 4) chunk = 4;
    if (chunk > cols.n) chunk = cols.n;
    // keep each staging buffer <= 512 MiB
    const uint64_t max_stage = 512ull << 20;
    if (chunk * pl.bytes_per_point > max_stage) chunk = max_stage / pl.bytes_per_point;
    if (chunk < 1) chunk = 1;
    chunk = (chunk + 3) & ~3ull;  // multiples of 4 points keep 12-byte blocks 16-byte aligned per chunk
    pl.chunk = chunk;
    pl.stage_need = (size_t)(chunk * pl.bytes_per_point) + 64;

    // every region starts 16-byte aligned (a time column: K3's fast path)
    pl.off_xyz = 0;
    pl.off_cls = pl.need_xyz ? align16((size_t)chunk * 12) : 0;
    pl.off_rgb = pl.off_cls + (pl.need_cls ? align16((size_t)chunk * w) : 0);
    return pl;
}
