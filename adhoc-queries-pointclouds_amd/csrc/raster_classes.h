// raster_classes.h — a class SET as a second test of the raster kernels (raster_cells.h): what a kernel needs to keep, of the points
// that pass the box, those whose class byte is in a set of the 256 classes.  Instantiated by the class-filtered mean-height raster
// (scan_zsum_classes.hip) and, with two sets at once, by the canopy-height raster (scan_zrange_classes.hip); the density raster could
// include it for an entry of its own.  The fill of a segment with the class column stands at the end.
//
//   the set       eight dwords, class c in the set when bit (c & 31) of word c >> 5 is set.  They are kernel arguments (uniform), not
//                 part of the segment table: the table cache is keyed on columns, predicates and kind, and a set stored in the table
//                 would be served stale to the next call with another set.  At entry the wave spreads them into a table of 256
//                 bytes of its LDS (class_table_fill: byte c is 1 when class c is in the set), so that the test of a class byte is
//                 one ds_read_u8 at the byte's own value.  Tested against it: a tree of selects over the eight words in registers,
//                 about fifteen VALU instructions per byte and sixty per tile — 10.9 ms against 9.6 with the table at 2048 cells,
//                 where one wave per SIMD hides nothing (profiles/zsum_classes_rate.log).
//   the cursor    COL_RASTER_U8 for seg_seek (scan_tiles.h): RasterCol (origin, cell widths, magics) and, of SegCol<COL_U8>, the class
//                 block rounded down to a dword, the shift and lane 63's off_hi — a class block may start at any byte.  Everything of a
//                 segment through SGPRs at a seek.  The registers and loads are those of the box AND class count (PipeRegs<TILES,
//                 COL_U8>, col2_load: two dwords per lane and tile behind the positions, counted by the waits).
//   the verdicts  after v_alignbit lane l holds the class bytes of points 4l .. 4l + 3 of a tile, while the cell and z of a point live
//                 in the lane where the point's first dword lies, in one of the six slots of a tile.  class_verdict_word puts "byte i
//                 is in the set" at bit 8i + 7 of the lane's word, where the box AND class count has "byte i equals the class"
//                 (zero_bytes), so the transport is that kernel's (verdict_at): a ds_bpermute by the per-lane constants addr_a / bit_a /
//                 addr_b / bit_b of Col2<COL_U8>, computed once by col2_lanes, brings the verdict of the point that starts in the lane
//                 to the lane, and a ballot makes the wave mask that is ANDed into the slot's start mask.  The transport touches no
//                 LDS memory (ds_bpermute moves registers); no scratch, and nothing per segment leaves the SGPRs.
#pragma once

#include "pcq_internal.h"
#include "raster_cells.h"
#include "scan_tiles.h"

namespace {

// The set of a launch, by value among the kernel's arguments.
struct ClassSet {
    uint32_t w[8];
};

constexpr uint32_t CLASS_TABLE_BYTES = 256;  // of a workgroup's LDS, in front of the raster's words

// The set into the wave's table: lane l writes the bytes of classes 4l .. 4l + 3.  (The selects run once per kernel.)
__device__ __forceinline__ void class_table_fill(uint32_t *table, const ClassSet &s, int lane) {
    const uint32_t a0 = (lane & 8) ? s.w[1] : s.w[0], a1 = (lane & 8) ? s.w[3] : s.w[2];
    const uint32_t a2 = (lane & 8) ? s.w[5] : s.w[4], a3 = (lane & 8) ? s.w[7] : s.w[6];
    const uint32_t b0 = (lane & 16) ? a1 : a0, b1 = (lane & 16) ? a3 : a2;
    const uint32_t nib = (((lane & 32) ? b1 : b0) >> (4 * (lane & 7))) & 0xfu;  // classes 4l .. 4l + 3: bits 4 (l & 7) .. of word l >> 3
    table[lane] = (nib & 1u) | (nib & 2u) << 7 | (nib & 4u) << 14 | (nib & 8u) << 21;
}
// Class byte c is in the set: 1 or 0.
__device__ __forceinline__ uint32_t class_in_set(const uint32_t *table, uint32_t c) { return reinterpret_cast<const uint8_t *>(table)[c]; }
// The four class bytes of a lane (points 4l .. 4l + 3 of a tile) into the verdict word verdict_at reads: bit 8i + 7 (vbit<COL_U8>) says
// that byte i is in the set.
__device__ __forceinline__ uint32_t class_verdict_word(uint32_t bytes, const uint32_t *table) {
    return class_in_set(table, bytes & 0xffu) << 7 | class_in_set(table, (bytes >> 8) & 0xffu) << 15 |
           class_in_set(table, (bytes >> 16) & 0xffu) << 23 | class_in_set(table, bytes >> 24) << 31;
}
// The six slots' class masks of a tile: bit l of va[k] is the verdict of the point that lane l starts among j = 0..2 of load k, bit l of
// vb[k] that of the second point, which starts at j = 3 where j0 == 0 (it means nothing in the other lanes: s3[k] has start_lanes there).
// (Issued in front of the box masks, with the ballots behind them, so that the compares run while the LDS operations are under way,
// the pass takes the same time: 9.63 against 9.64 ms at 2048 cells.)
__device__ __forceinline__ void class_slot_masks(const Col2Regs<COL_U8> &r, uint32_t shift, const Col2<COL_U8> &lanes, const uint32_t *table,
                                                 uint64_t (&va)[3], uint64_t (&vb)[3]) {
    const uint32_t V = class_verdict_word(__builtin_amdgcn_alignbit((uint32_t)r.hi, (uint32_t)r.lo, shift), table);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        va[k] = __ballot(verdict_at(V, lanes.addr_a[k], lanes.bit_a[k]));
        vb[k] = __ballot(verdict_at(V, lanes.addr_b[k], lanes.bit_b[k]));
    }
}

// TWO sets at once (scan_zrange_classes.hip: the lowest z of a `low` set and the highest z of a `high` set from one pass).  One
// table: bit 0 of byte c says that class c is in the low set, bit 1 that it is in the high set, so a class byte still costs one
// ds_read_u8.  One verdict word: byte i of the lane's word has its low verdict at bit 8i + 6 and its high verdict at bit 8i + 7
// (vbit<COL_U8> and the bit below it), so one ds_bpermute per slot brings both verdicts of a point to its lane and a shift by
// bit - 1 leaves them in bits 0 and 1; a ballot per set makes the masks.  Six ds_bpermute per tile, as for one set, and twelve
// ballots.  (The other form, two verdict words and twelve ds_bpermute, was compiled beside it: DESIGN.md §4 "How high above the
// ground is this box" has the counts.)
__device__ __forceinline__ uint32_t class_nibble(const ClassSet &s, int lane) {  // classes 4l .. 4l + 3 of the set: bits 0 .. 3
    const uint32_t a0 = (lane & 8) ? s.w[1] : s.w[0], a1 = (lane & 8) ? s.w[3] : s.w[2];
    const uint32_t a2 = (lane & 8) ? s.w[5] : s.w[4], a3 = (lane & 8) ? s.w[7] : s.w[6];
    const uint32_t b0 = (lane & 16) ? a1 : a0, b1 = (lane & 16) ? a3 : a2;
    return (((lane & 32) ? b1 : b0) >> (4 * (lane & 7))) & 0xfu;
}
__device__ __forceinline__ uint32_t nibble_bytes(uint32_t nib) { return (nib & 1u) | (nib & 2u) << 7 | (nib & 4u) << 14 | (nib & 8u) << 21; }
constexpr uint32_t CLASS_LOW = 1u, CLASS_HIGH = 2u;  // the bits of a byte of the two-set table
__device__ __forceinline__ void class_table_fill2(uint32_t *table, const ClassSet &low, const ClassSet &high, int lane) {
    table[lane] = nibble_bytes(class_nibble(low, lane)) | nibble_bytes(class_nibble(high, lane)) << 1;
}
// Class byte c against both sets: CLASS_LOW | CLASS_HIGH, either or 0.
__device__ __forceinline__ uint32_t class_in_sets(const uint32_t *table, uint32_t c) { return reinterpret_cast<const uint8_t *>(table)[c]; }
__device__ __forceinline__ uint32_t class_verdict_word2(uint32_t bytes, const uint32_t *table) {
    return class_in_sets(table, bytes & 0xffu) << 6 | class_in_sets(table, (bytes >> 8) & 0xffu) << 14 |
           class_in_sets(table, (bytes >> 16) & 0xffu) << 22 | class_in_sets(table, bytes >> 24) << 30;
}
// The twelve class masks of a tile: class_slot_masks for the low set (la, lb) and the high set (ha, hb).
__device__ __forceinline__ void class_slot_masks2(const Col2Regs<COL_U8> &r, uint32_t shift, const Col2<COL_U8> &lanes, const uint32_t *table,
                                                  uint64_t (&la)[3], uint64_t (&lb)[3], uint64_t (&ha)[3], uint64_t (&hb)[3]) {
    const uint32_t V = class_verdict_word2(__builtin_amdgcn_alignbit((uint32_t)r.hi, (uint32_t)r.lo, shift), table);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t a = (uint32_t)__builtin_amdgcn_ds_bpermute((int)lanes.addr_a[k], (int)V) >> (lanes.bit_a[k] - 1);
        const uint32_t b = (uint32_t)__builtin_amdgcn_ds_bpermute((int)lanes.addr_b[k], (int)V) >> (lanes.bit_b[k] - 1);
        la[k] = __ballot((a & CLASS_LOW) != 0), ha[k] = __ballot((a & CLASS_HIGH) != 0);
        lb[k] = __ballot((b & CLASS_LOW) != 0), hb[k] = __ballot((b & CLASS_HIGH) != 0);
    }
}

// The cursor kind: the raster's constants and the class column, no `pat`.
constexpr int COL_RASTER_U8 = 4;
template <>
struct BatchSeg<COL_RASTER_U8> {
    typedef DevRasterClassSegment type;
};
template <>
struct SegCol<COL_RASTER_U8> {
    RasterCol r;
    const uint8_t *cbase;  // the class bytes, rounded down to a dword (uniform)
    uint32_t shift;        // 8 x the misalignment (uniform)
    uint32_t off_hi;       // this lane's second dword of a tile (lane 63 of an aligned block: its first)
};
typedef SegCol<COL_RASTER_U8> RasterClassCol;
__device__ __forceinline__ void segcol_seek(RasterClassCol &c, const DevRasterClassSegment &g, int lane) {
    int32_t lox = g.lo[0], loy = g.lo[1];
    uint32_t cwx = g.cw[0], cwy = g.cw[1], mx = g.magic[0], my = g.magic[1];
    uint64_t cls = (uint64_t)(uintptr_t)g.cls;
    asm volatile("" : "+s"(lox), "+s"(loy), "+s"(cwx), "+s"(cwy), "+s"(mx), "+s"(my), "+s"(cls));
    c.r.lox = lox, c.r.loy = loy, c.r.cwx = cwx, c.r.cwy = cwy, c.r.mx = mx, c.r.my = my;
    const uint32_t mis = (uint32_t)cls & 3u;
    c.cbase = reinterpret_cast<const uint8_t *>((uintptr_t)(cls - mis));
    c.shift = 8 * mis;
    c.off_hi = lane == 63 && mis == 0 ? 4 * lane : 4 * lane + 4;  // (col2_setup: nothing of the tile lies behind an aligned block's dword 63)
}
// the lane constants with the cursor's segment, for pipe_load (`pat` is not used)
__device__ __forceinline__ Col2<COL_U8> col2_of(Col2<COL_U8> lanes, const RasterClassCol &c) {
    lanes.base = c.cbase;
    lanes.off_hi = c.off_hi;
    lanes.shift = c.shift;
    return lanes;
}
template <>
struct PipeCol<COL_RASTER_U8> {
    static constexpr int value = COL_U8;
};

// raster_segment_fill for a table with the class column: its refusal first, then the pointer and the raster's fill.
inline int raster_segment_fill(const char *prefix, DevRasterClassSegment &g, const pcq_predicate &pred, const pcq_columns &col, const uint32_t *cw,
                               uint32_t nx, uint32_t ny, size_t i) {
    if (col.n && (col.cls_stride != 1 || !col.cls))
        return pcq_fail(PCQ_ERR_ARG, "%s: LAST classification blocks only (stride 1, not null), segment %zu", prefix, i);
    g.cls = (const uint8_t *)col.cls;
    return raster_segment_fill(prefix, static_cast<DevRasterSegment &>(g), pred, col, cw, nx, ny, i);
}

}  // namespace
