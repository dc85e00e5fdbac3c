// scan_tiles.h — the wave-tile count of packed LAST positions, shared by the count kernels (scan_count.hip,
// scan_count_combined.hip) and the chunk index (chunk_index.hip): the mask algebra of a 768-dword tile, K1's second column
// (class bytes or GPS times) and the software-pipeline helpers.  See scan_count.hip for the design.
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
__device__ __forceinline__ bool t_in(int lo, int hi, double t0, double t1) {
    const double t = __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
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

__device__ __forceinline__ uint32_t tile_count_masks(const v4i *tile, int lane, const LaneBox &b) {
    v4i v[3];
    v[0] = ld_nt(tile + lane);
    v[1] = ld_nt(tile + 64 + lane);
    v[2] = ld_nt(tile + 128 + lane);
    return tile_count_regs(v, b);
}

// Software pipeline: asm volatile statements keep their order; the empty asm behind each s_waitcnt re-defines the
// registers it guards, so no use can be hoisted above the wait.
template <int TILES, int COL = COL_NONE>
struct PipeRegs {
    v4i r[TILES][3];
    Col2Regs<COL> c[TILES];
};
template <int TILES>
struct PipeRegs<TILES, COL_NONE> {
    v4i r[TILES][3];
};
constexpr int col2_loads(int col) { return col == COL_NONE ? 0 : 2; }  // per tile
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
template <int TILES, int PENDING, int COL>
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

}  // namespace
