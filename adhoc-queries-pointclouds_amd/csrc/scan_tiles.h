// scan_tiles.h — what the count kernels (scan_count.hip, scan_count_batch.hip, scan_count_multi.hip, scan_class_hist.hip,
// scan_time_hist.hip, scan_raster.hip, scan_zrange.hip, scan_polygon.hip, scan_time.hip) and the chunk index (chunk_index.hip) share: the mask algebra of a 768-dword tile of packed LAST positions,
// K1's second column (class bytes or GPS times), the register sets of the software pipeline with their loads and counted waits
// (PipeRegs for the K1 family, VecRegs for the one-column kernels K2 and K3), the software pipeline of every kernel that walks a
// segment table with seg_seek (pipe_scan: the batched K1, the class and time histograms, the polygon count and the density, height and
// canopy-height rasters call it with their own eval; the one-file kernels, the multi-box count, whose cursor carries eight boxes and
// no `empty`, and the three rasters that add 64-bit words write their loop out: see scan_count.hip and those rasters' files) and the batched K1 (k_bounds_count_batch_pipe: one template for the box, box AND class and box AND time
// kinds).  The host side of a K1-family batched launch is k1_batch_launch (scan_batch_host.h); the finish reduction of every
// count is pcq_launch_finish_counts (scan_count_multi.hip).  See scan_count.hip for the design.
#pragma once

#include "pcq_internal.h"

namespace {

constexpr int BLOCK = 256;
constexpr int TILE_POINTS = 256;  // per wave: 768 dwords = 3 x (64 lanes x 16 B)
constexpr int K1_TILES = 2;       // adjacent 3 KiB tiles per step (profiles/r01_k1_one_wave_blocks.log)
constexpr int K1_WAVES_PER_CU = 3;  // 7.19 TB/s at 3.0, 6.6-6.86 at 2.5 / 3.1 / 4 (tools/k1_grid_sweep.py)
constexpr int K2_LOADS = 4;       // 1 KiB loads per step of the class kernels
constexpr int K2_WAVES_PER_CU = 4;  // profiles/r01_k2_sweep.log

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr uint64_t R0 = 0x9249249249249249ull;  // lanes with lane % 3 == 0
constexpr uint64_t R1 = 0x2492492492492492ull;  // lane % 3 == 1
constexpr uint64_t R2 = 0x4924924924924924ull;  // lane % 3 == 2

// lanes l for which dword (k, l, j) of a tile is the first component of a point:
// (k + l + j) % 3 == 0  <=>  l % 3 == (3 - (k + j) % 3) % 3
__device__ __forceinline__ constexpr uint64_t start_lanes(int s) {
    return (s % 3) == 0 ? R0 : ((s % 3) == 1 ? R2 : R1);
}

__device__ __forceinline__ v4i ld_nt(const v4i *p) { return __builtin_nontemporal_load(p); }

// Bytes of a dword equal to zero -> 0x80 in that byte (exact, no borrow artefacts).
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) {
    const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return ~(t | x | 0x7f7f7f7fu);
}
template <int V>
struct IntC {};

// K1's second column (the combined kinds): none, class bytes, or f64 GPS times.
enum { COL_NONE = 0, COL_U8 = 1, COL_F64 = 2 };

// Per-lane constants of the second column.  A point p of a tile (0..255) has its verdict in bit vbit(p) of the verdict word
// of lane vlane(p): COL_U8 — the class bytes of points 4l .. 4l + 3 in lane l (bits 7, 15, 23, 31: zero_bytes);
// COL_F64 — the times of points 2l, 2l + 1 (bits 0, 1) and 128 + 2l, 129 + 2l (bits 2, 3) in lane l.  In load k of a
// tile, lane l holds dwords 256 k + 4 l + j; the first point that starts there is pa = (256 k + 4 l + j0) / 3, and when
// j0 == 0 a second one starts at j = 3: pa + 1.  sel_a[k] / sel_b[k]: the byte address (for ds_bpermute) of the lane
// holding that point's verdict, and its bit in the word.
template <int COL>
struct Col2 {};
template <>
struct Col2<COL_U8> {
    const uint8_t *base;      // the body's class bytes, rounded down to a dword (uniform)
    uint32_t off_lo, off_hi;  // this lane's dword of a tile and the one behind it (lane 63 of an aligned column: itself)
    uint32_t shift, pat;      // 8 x the misalignment; the class byte in every byte
    uint32_t addr_a[3], bit_a[3], addr_b[3], bit_b[3];
};
template <>
struct Col2<COL_F64> {
    const uint8_t *base;  // the body's times (8-byte aligned)
    double t0, t1;
    uint32_t addr_a[3], bit_a[3], addr_b[3], bit_b[3];
};
template <int COL>
__device__ __forceinline__ uint32_t vlane(uint32_t p) { return COL == COL_U8 ? p >> 2 : (p & 127) >> 1; }
template <int COL>
__device__ __forceinline__ uint32_t vbit(uint32_t p) { return COL == COL_U8 ? 8 * (p & 3) + 7 : 2 * (p >> 7) + (p & 1); }
template <int COL>
__device__ __forceinline__ void col2_lanes(Col2<COL> &c, int lane) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t j0 = (3 - (uint32_t)(k + lane) % 3) % 3;
        const uint32_t pa = (256 * k + 4 * lane + j0) / 3, pb = (pa + 1) & 255;  // (pb: only lanes with j0 == 0 use it)
        c.addr_a[k] = 4 * vlane<COL>(pa), c.bit_a[k] = vbit<COL>(pa);
        c.addr_b[k] = 4 * vlane<COL>(pb), c.bit_b[k] = vbit<COL>(pb);
    }
}
__device__ __forceinline__ Col2<COL_U8> col2_setup(const uint8_t *col, const DevPred &pred, int lane, IntC<COL_U8>) {
    Col2<COL_U8> c;
    const uint32_t mis = (uint32_t)((uintptr_t)col & 3);
    c.base = col - mis;
    c.off_lo = 4 * lane;
    c.off_hi = lane == 63 && mis == 0 ? 4 * lane : 4 * lane + 4;  // (nothing of the tile lies behind an aligned column's dword 63)
    c.shift = 8 * mis;
    c.pat = 0x01010101u * (pred.cls & 0xffu);
    col2_lanes<COL_U8>(c, lane);
    return c;
}
__device__ __forceinline__ Col2<COL_F64> col2_setup(const uint8_t *col, const DevPred &pred, int lane, IntC<COL_F64>) {
    Col2<COL_F64> c;
    c.base = col;
    c.t0 = pred.wmin[0], c.t1 = pred.wmax[0];
    col2_lanes<COL_F64>(c, lane);
    return c;
}
__device__ __forceinline__ Col2<COL_NONE> col2_setup(const uint8_t *, const DevPred &, int, IntC<COL_NONE>) { return {}; }

// A tile's second-column registers.
template <int COL>
struct Col2Regs {};
template <>
struct Col2Regs<COL_U8> {
    int lo, hi;
};
template <>
struct Col2Regs<COL_F64> {
    v4i a, b;
};
__device__ __forceinline__ double time_of(int lo, int hi) {  // the f64 whose two dwords a load delivered
    return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}
__device__ __forceinline__ bool t_in(int lo, int hi, double t0, double t1) {
    const double t = time_of(lo, hi);
    return (t >= t0) & (t < t1);  // Range<f64>::contains: NaN is no match
}
__device__ __forceinline__ uint32_t verdict_word(const Col2Regs<COL_U8> &r, const Col2<COL_U8> &c) {
    return zero_bytes(__builtin_amdgcn_alignbit((uint32_t)r.hi, (uint32_t)r.lo, c.shift) ^ c.pat);
}
__device__ __forceinline__ uint32_t verdict_word(const Col2Regs<COL_F64> &r, const Col2<COL_F64> &c) {
    return (uint32_t)t_in(r.a[0], r.a[1], c.t0, c.t1) | (uint32_t)t_in(r.a[2], r.a[3], c.t0, c.t1) << 1 |
           (uint32_t)t_in(r.b[0], r.b[1], c.t0, c.t1) << 2 | (uint32_t)t_in(r.b[2], r.b[3], c.t0, c.t1) << 3;
}
// the verdict of the point held at (addr, bit), brought to this lane
__device__ __forceinline__ bool verdict_at(uint32_t V, uint32_t addr, uint32_t bit) {
    return (((uint32_t)__builtin_amdgcn_ds_bpermute((int)addr, (int)V) >> bit) & 1u) != 0;
}

struct LaneBox {
    int lo[3];        // lo[(lane%3 + t) % 3], t = 0..2
    uint32_t w[3];
};

__device__ __forceinline__ LaneBox rotate_box(const int32_t (&lo)[3], const uint32_t (&w)[3], int lane) {
    const int r = lane % 3;
    LaneBox b;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int c = (r + t) % 3;
        b.lo[t] = c == 0 ? lo[0] : (c == 1 ? lo[1] : lo[2]);
        b.w[t] = c == 0 ? w[0] : (c == 1 ? w[1] : w[2]);
    }
    return b;
}

// Count of matching points in one 768-dword wave tile, mask-algebra form (wave-uniform result).  COL: the points' verdicts
// of the second column (verdict word V) are ANDed into the start bits.
template <int COL = COL_NONE>
__device__ __forceinline__ uint32_t tile_count_regs(const v4i (&v)[3], const LaneBox &b, const Col2<COL> &c2 = {}, uint32_t V = 0) {
    uint64_t m[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int t = (k + j) % 3;
            m[k][j] = __ballot((uint32_t)(v[k][j] - b.lo[t]) <= b.w[t]);
        }
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint64_t m0 = m[k][0], m1 = m[k][1], m2 = m[k][2], m3 = m[k][3];
        // dwords 4l+4, 4l+5: lane l+1 of this load, or lane 0 of the next one.  The tile ends on a
        // point boundary, so nothing is carried out of k == 2.
        const uint64_t c0 = k < 2 ? m[k < 2 ? k + 1 : k][0] : 0ull;
        const uint64_t c1 = k < 2 ? m[k < 2 ? k + 1 : k][1] : 0ull;
        const uint64_t n0 = (m0 >> 1) | (c0 << 63);
        const uint64_t n1 = (m1 >> 1) | (c1 << 63);
        const uint64_t a = m1 & m2;
        const uint64_t t0 = m0 & a;      // dwords j=0,1,2 of lane l
        const uint64_t t1 = a & m3;      // j=1,2,3
        const uint64_t bb = m3 & n0;
        const uint64_t t2 = m2 & bb;     // j=2,3 and next lane's 0
        const uint64_t t3 = bb & n1;     // j=3 and next lane's 0,1
        const uint64_t s012 = (t0 & start_lanes(k)) | (t1 & start_lanes(k + 1)) | (t2 & start_lanes(k + 2));
        if constexpr (COL == COL_NONE) {
            cnt += (uint32_t)__popcll(s012) + (uint32_t)__popcll(t3 & start_lanes(k + 3));
        } else {  // one start among j = 0..2 per lane, and a second one at j = 3 where j0 == 0
            const uint64_t va = __ballot(verdict_at(V, c2.addr_a[k], c2.bit_a[k])), vb = __ballot(verdict_at(V, c2.addr_b[k], c2.bit_b[k]));
            cnt += (uint32_t)__popcll(s012 & va) + (uint32_t)__popcll(t3 & start_lanes(k + 3) & vb);
        }
    }
    return cnt;
}

// The verdicts of a tile's points, not counted (scan_class_hist.hip): bit l of t[k][j] says that the three dwords from dword
// (k, l, j) of the tile on pass the tests of x, y and z in this order — the box verdict of the point that starts there.  It
// means nothing where no point starts (tile_count_regs ANDs start_lanes into it; a caller that looks a point up by its first
// dword needs no such mask).  The mask algebra is that of tile_count_regs.
__device__ __forceinline__ void tile_start_masks(const v4i (&v)[3], const LaneBox &b, uint64_t (&t)[3][4]) {
    uint64_t m[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = (k + j) % 3;
            m[k][j] = __ballot((uint32_t)(v[k][j] - b.lo[c]) <= b.w[c]);
        }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint64_t m0 = m[k][0], m1 = m[k][1], m2 = m[k][2], m3 = m[k][3];
        const uint64_t c0 = k < 2 ? m[k < 2 ? k + 1 : k][0] : 0ull;  // (nothing is carried out of k == 2: the tile ends on a point boundary)
        const uint64_t c1 = k < 2 ? m[k < 2 ? k + 1 : k][1] : 0ull;
        const uint64_t n0 = (m0 >> 1) | (c0 << 63);
        const uint64_t n1 = (m1 >> 1) | (c1 << 63);
        const uint64_t a = m1 & m2;
        const uint64_t bb = m3 & n0;
        t[k][0] = m0 & a;    // dwords j=0,1,2 of lane l
        t[k][1] = a & m3;    // j=1,2,3
        t[k][2] = m2 & bb;   // j=2,3 and next lane's 0
        t[k][3] = bb & n1;   // j=3 and next lane's 0,1
    }
}

__device__ __forceinline__ uint32_t tile_count_masks(const v4i *tile, int lane, const LaneBox &b) {
    v4i v[3];
    v[0] = ld_nt(tile + lane);
    v[1] = ld_nt(tile + 64 + lane);
    v[2] = ld_nt(tile + 128 + lane);
    return tile_count_regs(v, b);
}

// Software pipeline: asm volatile statements keep their order; the empty asm behind each s_waitcnt re-defines the
// registers it guards, so no use can be hoisted above the wait.
constexpr int col2_loads(int col) { return col == COL_NONE ? 0 : 2; }  // per tile
template <int TILES, int COL = COL_NONE>
struct PipeRegs {
    static constexpr int LOADS = TILES * (3 + col2_loads(COL));  // what a counted wait leaves in flight
    v4i r[TILES][3];
    Col2Regs<COL> c[TILES];
};
template <int TILES>
struct PipeRegs<TILES, COL_NONE> {
    static constexpr int LOADS = TILES * 3;
    v4i r[TILES][3];
};
// the second column of tile `tile` (two loads per lane, issued behind the positions: the waits count them)
__device__ __forceinline__ void col2_load(Col2Regs<COL_U8> &r, const Col2<COL_U8> &c, uint64_t tile) {
    const uint8_t *tb = c.base + tile * 256;
    asm volatile("global_load_dword %0, %2, %4 nt\n\tglobal_load_dword %1, %3, %4 nt"
                 : "=&v"(r.lo), "=&v"(r.hi)
                 : "v"(c.off_lo), "v"(c.off_hi), "s"(tb)
                 : "memory");
}
__device__ __forceinline__ void col2_load(Col2Regs<COL_F64> &r, const Col2<COL_F64> &c, uint64_t tile) {
    const uint8_t *tb = c.base + tile * 2048;
    asm volatile("global_load_dwordx4 %0, %2, %3 nt\n\tglobal_load_dwordx4 %1, %2, %3 offset:1024 nt"
                 : "=&v"(r.a), "=&v"(r.b)
                 : "v"(16u * (uint32_t)__lane_id()), "s"(tb)
                 : "memory");
}
// the same with plain loads (the leftover tiles, outside the pipeline)
__device__ __forceinline__ void col2_load_plain(Col2Regs<COL_U8> &r, const Col2<COL_U8> &c, uint64_t tile) {
    r.lo = *reinterpret_cast<const int *>(c.base + tile * 256 + c.off_lo);
    r.hi = *reinterpret_cast<const int *>(c.base + tile * 256 + c.off_hi);
}
__device__ __forceinline__ void col2_load_plain(Col2Regs<COL_F64> &r, const Col2<COL_F64> &c, uint64_t tile) {
    const v4i *q = reinterpret_cast<const v4i *>(c.base + tile * 2048) + __lane_id();
    r.a = q[0];
    r.b = q[64];
}
__device__ __forceinline__ void col2_guard(Col2Regs<COL_U8> &r) { asm volatile("" : "+v"(r.lo), "+v"(r.hi)::"memory"); }
__device__ __forceinline__ void col2_guard(Col2Regs<COL_F64> &r) { asm volatile("" : "+v"(r.a), "+v"(r.b)::"memory"); }
// second column of point p (0-based in the body), one lane at a time: the tail behind the last whole tile
__device__ __forceinline__ bool col2_point(const Col2<COL_U8> &c, uint64_t p) { return c.base[c.shift / 8 + p] == (c.pat & 0xffu); }
__device__ __forceinline__ bool col2_point(const Col2<COL_F64> &c, uint64_t p) {
    const double t = reinterpret_cast<const double *>(c.base)[p];
    return (t >= c.t0) & (t < c.t1);
}

template <int TILES, int COL>
__device__ __forceinline__ void pipe_load(PipeRegs<TILES, COL> &R, const v4i *base, uint64_t step, int lane, const Col2<COL> &c2) {
#pragma unroll
    for (int t = 0; t < TILES; t++) {
        const v4i *q = base + (step * TILES + t) * 192 + lane;
        asm volatile("global_load_dwordx4 %0, %3, off nt\n\tglobal_load_dwordx4 %1, %3, off offset:1024 nt\n\t"
                     "global_load_dwordx4 %2, %3, off offset:2048 nt"
                     : "=&v"(R.r[t][0]), "=&v"(R.r[t][1]), "=&v"(R.r[t][2])
                     : "v"(q)
                     : "memory");
    }
    if constexpr (COL != COL_NONE) {
#pragma unroll
        for (int t = 0; t < TILES; t++) col2_load(R.c[t], c2, step * TILES + t);
    }
}
template <int TILES>
__device__ __forceinline__ void pipe_load(PipeRegs<TILES> &R, const v4i *base, uint64_t step, int lane) {
    pipe_load<TILES, COL_NONE>(R, base, step, lane, Col2<COL_NONE>{});
}
// PENDING: the loads of the other register set, which stay in flight
template <int PENDING, int TILES, int COL>
__device__ __forceinline__ void pipe_wait(PipeRegs<TILES, COL> &R) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PENDING) : "memory");
#pragma unroll
    for (int t = 0; t < TILES; t++) asm volatile("" : "+v"(R.r[t][0]), "+v"(R.r[t][1]), "+v"(R.r[t][2])::"memory");
    if constexpr (COL != COL_NONE) {
#pragma unroll
        for (int t = 0; t < TILES; t++) col2_guard(R.c[t]);
    }
}
template <int TILES, int COL>
__device__ __forceinline__ uint64_t pipe_eval(const PipeRegs<TILES, COL> &R, const LaneBox &lb, const Col2<COL> &c2) {
    uint64_t c = 0;
#pragma unroll
    for (int t = 0; t < TILES; t++) {
        if constexpr (COL == COL_NONE) c += tile_count_regs(R.r[t], lb);
        else c += tile_count_regs<COL>(R.r[t], lb, c2, verdict_word(R.c[t], c2));
    }
    return c;
}
template <int TILES>
__device__ __forceinline__ uint64_t pipe_eval(const PipeRegs<TILES> &R, const LaneBox &lb) {
    return pipe_eval<TILES, COL_NONE>(R, lb, Col2<COL_NONE>{});
}

// The register set of the one-column kernels (K2's class bytes, K3's times): LOADS x 1 KiB of a packed column per step.
template <int N>
struct VecRegs {
    static constexpr int LOADS = N;
    v4i r[N];
};
template <int N>
__device__ __forceinline__ void vec_load(VecRegs<N> &R, const v4i *step, int lane) {
#pragma unroll
    for (int k = 0; k < N; k++) {
        const v4i *q = step + 64 * k + lane;
        asm volatile("global_load_dwordx4 %0, %1, off nt" : "=&v"(R.r[k]) : "v"(q) : "memory");
    }
}
template <int PENDING, int N>
__device__ __forceinline__ void pipe_wait(VecRegs<N> &R) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PENDING) : "memory");
#pragma unroll
    for (int k = 0; k < N; k++) asm volatile("" : "+v"(R.r[k])::"memory");
}

// The second column as a kernel's last template argument: none (the plain K1), ClassBytes (PCQ_PRED_BOUNDS_CLASS) or GpsTimes
// (PCQ_PRED_BOUNDS_TIME).  The per-file K1 also takes it as its last argument: the column at the body's first point (class
// bytes: any alignment; times: 8-byte aligned).
struct ClassBytes {
    const uint8_t *p;
};
struct GpsTimes {
    const uint8_t *p;
};
template <typename... Col>
struct ColOf {
    static constexpr int value = COL_NONE;
};
template <>
struct ColOf<ClassBytes> {
    static constexpr int value = COL_U8;
};
template <>
struct ColOf<GpsTimes> {
    static constexpr int value = COL_F64;
};

// Batched K1 (k_bounds_count_batch_pipe<TILES, Col...>): box, box AND class, box AND time over many resident LAST blocks in
// one launch.  One wave per workgroup, TILES tiles per step, software-pipelined like the per-file K1: while the tiles of step
// u are evaluated the loads of step u + stride are in flight (TILES * (3 + col2_loads) per register set).  Steps are numbered
// across all segments (tile_begin counts steps); each of the two register sets remembers the segment its step came from.
// What changes with the segment passes through SGPRs at a seek: the box, and of the second column the class block's address
// and class byte (COL_U8: base, shift, pat, lane 63's off_hi) or the time block's address and the range (COL_F64); the
// addr_* / bit_* lane constants of Col2 are computed once.  The segment tables differ per kind (BatchSeg), each at its own
// pitch in the context's d_segments.
template <int COL>
struct BatchSeg {
    typedef DevSegment type;
};
template <>
struct BatchSeg<COL_U8> {
    typedef DevCombinedSegment type;
};
template <>
struct BatchSeg<COL_F64> {
    typedef DevBoundsTimeSegment type;
};
template <int COL>
struct SegCol {};
template <>
struct SegCol<COL_U8> {
    const uint8_t *cbase;  // the class bytes, rounded down to a dword (uniform)
    uint32_t shift, pat;   // 8 x the misalignment; the class byte in every byte (uniform)
    uint32_t off_hi;       // this lane's second dword of a tile (lane 63 of an aligned block: its first)
};
template <>
struct SegCol<COL_F64> {
    const uint8_t *tbase;  // the segment's times (uniform)
    double t0, t1;         // its range (uniform)
};
template <int COL>
struct SegCursor {
    int s;
    uint64_t begin, end;
    const v4i *base;
    LaneBox lb;
    bool empty;
    SegCol<COL> col;
};
// the second column of the cursor's segment, through SGPRs like the box (seg_seek)
__device__ __forceinline__ void segcol_seek(SegCol<COL_NONE> &, const DevSegment &, int) {}
__device__ __forceinline__ void segcol_seek(SegCol<COL_U8> &c, const DevCombinedSegment &g, int lane) {
    uint64_t cls = (uint64_t)(uintptr_t)g.cls;
    uint32_t pat = g.pat;
    asm volatile("" : "+s"(cls), "+s"(pat));
    const uint32_t mis = (uint32_t)cls & 3u;
    c.cbase = reinterpret_cast<const uint8_t *>((uintptr_t)(cls - mis));
    c.shift = 8 * mis;
    c.pat = pat;
    c.off_hi = lane == 63 && mis == 0 ? 4 * lane : 4 * lane + 4;  // (col2_setup: nothing of the tile lies behind an aligned block's dword 63)
}
__device__ __forceinline__ void segcol_seek(SegCol<COL_F64> &c, const DevBoundsTimeSegment &g, int) {
    uint64_t times = (uint64_t)(uintptr_t)g.times;
    uint64_t b0 = (uint64_t)__double_as_longlong(g.t0), b1 = (uint64_t)__double_as_longlong(g.t1);
    asm volatile("" : "+s"(times), "+s"(b0), "+s"(b1));
    c.tbase = reinterpret_cast<const uint8_t *>((uintptr_t)times);
    c.t0 = __longlong_as_double((long long)b0);
    c.t1 = __longlong_as_double((long long)b1);
}
template <int TILES, int COL>
__device__ __forceinline__ void seg_seek(SegCursor<COL> &c, const typename BatchSeg<COL>::type *__restrict__ segs, int nseg, uint64_t u,
                                         int lane) {
    if (u < c.end) return;
    while (c.s + 1 < nseg && u >= segs[c.s + 1].tile_begin) c.s++;
    const typename BatchSeg<COL>::type &g = segs[c.s];
    c.begin = g.tile_begin;
    c.end = c.begin + g.n / ((uint64_t)TILES * TILE_POINTS);
    c.base = reinterpret_cast<const v4i *>(g.xyz);
    c.empty = g.empty != 0;
    // everything of the segment through SGPRs: left to itself the compiler turns "select of table entries" into a per-lane
    // address and a VECTOR load, and the s_waitcnt vmcnt(0) behind that load would drain the prefetched tiles.  The skip loop
    // above is not covered: from its second iteration on the compiler reads tile_begin with a vector load and waits for it, so a
    // workgroup that jumps over more than one segment drains both register sets once
    int32_t lo[3];
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = g.lo[k];
        w[k] = g.width[k];
        asm volatile("" : "+s"(lo[k]), "+s"(w[k]));
    }
    c.lb = rotate_box(lo, w, lane);
    segcol_seek(c.col, g, lane);
}
// the lane constants with the cursor's segment
__device__ __forceinline__ Col2<COL_NONE> col2_of(Col2<COL_NONE> lanes, const SegCol<COL_NONE> &) { return lanes; }
__device__ __forceinline__ Col2<COL_U8> col2_of(Col2<COL_U8> lanes, const SegCol<COL_U8> &c) {
    lanes.base = c.cbase;
    lanes.off_hi = c.off_hi;
    lanes.shift = c.shift;
    lanes.pat = c.pat;
    return lanes;
}
__device__ __forceinline__ Col2<COL_F64> col2_of(Col2<COL_F64> lanes, const SegCol<COL_F64> &c) {
    lanes.base = c.tbase;
    lanes.t0 = c.t0;
    lanes.t1 = c.t1;
    return lanes;
}
// the second column of a segment's leftover points, one lane per point: what the loop keeps in registers, and its test of point p
template <int COL>
struct SegTail {};
template <>
struct SegTail<COL_U8> {
    const DevCombinedSegment &g;
    uint8_t c8;
};
template <>
struct SegTail<COL_F64> {
    const double *tq;
    double t0, t1;
};
__device__ __forceinline__ SegTail<COL_NONE> seg_tail(const DevSegment &) { return {}; }
__device__ __forceinline__ SegTail<COL_U8> seg_tail(const DevCombinedSegment &g) { return {g, (uint8_t)(g.pat & 0xffu)}; }
__device__ __forceinline__ SegTail<COL_F64> seg_tail(const DevBoundsTimeSegment &g) {
    return {reinterpret_cast<const double *>(g.times), g.t0, g.t1};
}
__device__ __forceinline__ bool seg_point(const SegTail<COL_NONE> &, uint64_t) { return true; }
__device__ __forceinline__ bool seg_point(const SegTail<COL_U8> &c, uint64_t p) { return c.g.cls[p] == c.c8; }
__device__ __forceinline__ bool seg_point(const SegTail<COL_F64> &c, uint64_t p) {
    const double t = c.tq[p];
    return (t >= c.t0) & (t < c.t1);
}

// What a cursor kind loads beside the positions: the count kinds their own column; a kind that only carries constants of its segment
// (COL_RASTER of raster_cells.h, COL_POLYGON of scan_polygon.hip) names COL_NONE here, COL_RASTER_U8 (raster_classes.h) COL_U8.
template <int COL>
struct PipeCol {
    static constexpr int value = COL;
};
// the loads of step `step` of the cursor's segment
template <int TILES, int COL>
__device__ __forceinline__ void cursor_load(PipeRegs<TILES, PipeCol<COL>::value> &R, const SegCursor<COL> &c, uint64_t step, int lane,
                                            const Col2<PipeCol<COL>::value> &lanes) {
    if constexpr (PipeCol<COL>::value == COL_NONE) pipe_load<TILES>(R, c.base, step, lane);
    else pipe_load<TILES, PipeCol<COL>::value>(R, c.base, step, lane, col2_of(lanes, c.col));
}

// THE software pipeline of the batched K1 family (every kernel that walks a segment table with seg_seek): the steps blockIdx.x,
// blockIdx.x + gridDim.x, ... of the launch through two register sets.  While the tiles of step u are evaluated the loads of step
// u + stride are in flight; a counted wait leaves exactly those in flight.  Each register set remembers the segment its step came
// from (its cursor); behind the last step the prefetch is clamped to a step already read, and both sets are landed before the registers
// die.  eval(P, cursor, lanes) is called once for every step of a segment that is not empty: P the step's registers, lanes the
// lane constants of the second column (col2_lanes; of them a kernel pays only for what it reads).
// `segs` is not __restrict__ here, unlike seg_seek's and the kernels' own: with it the skip loop of seg_seek read tile_begin with a
// scalar load in six kernels (no drain of the prefetched tiles there) — better, perhaps, but another kernel than the one that was
// measured, so a change of its own.
template <int TILES, int COL, typename Eval>
__device__ __forceinline__ void pipe_scan(const typename BatchSeg<COL>::type *segs, int nseg, uint64_t total_steps, int lane,
                                          const Eval &eval) {
    constexpr int LD = PipeCol<COL>::value;
    constexpr int LOADS = PipeRegs<TILES, LD>::LOADS;  // per register set
    const uint64_t stride = gridDim.x;
    if (blockIdx.x < total_steps) {
        Col2<LD> lanes{};
        if constexpr (LD == COL_U8) lanes.off_lo = 4 * lane;
        if constexpr (LD != COL_NONE) col2_lanes<LD>(lanes, lane);
        PipeRegs<TILES, LD> A, B;
        SegCursor<COL> ca = {0, 0, 0, nullptr, {}, true, {}}, cb;
        uint64_t u = blockIdx.x;
        seg_seek<TILES, COL>(ca, segs, nseg, u, lane);
        cursor_load<TILES, COL>(A, ca, u - ca.begin, lane, lanes);
        for (;;) {
            const uint64_t u1 = u + stride;
            cb = ca;
            if (u1 < total_steps) seg_seek<TILES, COL>(cb, segs, nseg, u1, lane);
            cursor_load<TILES, COL>(B, cb, (u1 < total_steps ? u1 : u) - cb.begin, lane, lanes);  // clamped at the tail: an L2 hit
            pipe_wait<LOADS>(A);
            if (!ca.empty) eval(A, ca, lanes);
            if (u1 >= total_steps) break;
            const uint64_t u2 = u1 + stride;
            ca = cb;
            if (u2 < total_steps) seg_seek<TILES, COL>(ca, segs, nseg, u2, lane);
            cursor_load<TILES, COL>(A, ca, (u2 < total_steps ? u2 : u1) - ca.begin, lane, lanes);
            pipe_wait<LOADS>(B);
            if (!cb.empty) eval(B, cb, lanes);
            if (u2 >= total_steps) break;
            u = u2;
        }
        pipe_wait<0>(A);  // the clamped tail prefetch is still in flight: land it before the registers die
        pipe_wait<0>(B);
    }
}

template <int TILES, typename... Col>
__global__ __launch_bounds__(64) void k_bounds_count_batch_pipe(const DevSegment *__restrict__ raw, int nseg, uint64_t total_steps,
                                                               uint64_t *__restrict__ partials) {
    constexpr int COL = ColOf<Col...>::value;
    static_assert(sizeof...(Col) <= 1, "one second column at most");
    typedef typename BatchSeg<COL>::type Seg;
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    const Seg *__restrict__ segs = reinterpret_cast<const Seg *>(raw);
    const int lane = threadIdx.x;
    uint64_t total = 0;
    pipe_scan<TILES, COL>(segs, nseg, total_steps, lane, [&](const PipeRegs<TILES, COL> &P, const SegCursor<COL> &c, const Col2<COL> &lanes) {
        total += pipe_eval<TILES, COL>(P, c.lb, col2_of(lanes, c.col));
    });
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {  // fewer-than-a-step leftovers of segment i, one lane per point
        const Seg &g = segs[i];
        if (g.empty) continue;
        const uint64_t n = g.n;
        const int *q0 = reinterpret_cast<const int *>(g.xyz);
        const SegTail<COL> tail = seg_tail(g);
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < ((n + 63) & ~63ull); p += 64) {
            bool pass = false;
            if (p < n) {
                const int *q = q0 + 3 * p;
                pass = ((uint32_t)(q[0] - g.lo[0]) <= g.width[0]) & ((uint32_t)(q[1] - g.lo[1]) <= g.width[1]) &
                       ((uint32_t)(q[2] - g.lo[2]) <= g.width[2]) & seg_point(tail, p);
            }
            total += (uint64_t)__popcll(__ballot(pass));
        }
    }
    if (lane == 0) partials[blockIdx.x] = total;
}

}  // namespace
