// scan_count.hip — the count-only fast paths of the predicate scan (kernels K1 and K2).
//
// K1 bounds_count restates the loop of search_last_file_by_bounds_optimized
//    (query/src/search/last.rs:117-135) feeding a CountCollector (collect_points.rs:83-85):
//    count of points with lmin <= (x,y,z) <= lmax over the LAST positions block, N x {i32 x,y,z}.
// K2 class_count restates search_last_file_by_classification_optimized (last.rs:253-262):
//    count of classification bytes equal to `cls` over the LAST classification block, N x u8.
//
// Both are pure HBM streaming reads (12 B/point, 1 B/point): no MFMA, no reuse.  Design for gfx950:
//  * every global load is a fully coalesced 16 B/lane access (1 KiB per wave-instruction),
//    issued non-temporal (the stream is read once);
//  * a 12-byte point is not a power of two, so a wave owns a 768-dword tile (= 256 whole points,
//    3 KiB) loaded by three dwordx4 instructions; instead of transposing through LDS, each dword is
//    range-tested against the bound of ITS component ((k + lane + j) mod 3, rotated per lane once)
//    and the 64-bit compare masks (wave64: v_cmp writes an SGPR pair) are combined with scalar
//    shifts/ANDs into "three consecutive dwords pass" bits, popcounted with s_bcnt1 — the VALU sees
//    two instructions per dword, everything else runs on the scalar unit;
//  * ONE-WAVE workgroups, three (class: four) per CU, persistent, software-pipelined by hand: the loads
//    of the next step are in flight (inline-asm global_load_dwordx4 nt + counted s_waitcnt) while the
//    current step is evaluated; per-workgroup partial counts are written with plain stores and folded by
//    a 1-block finishing kernel, so no same-address atomic storm at the tail.
// K1 also counts the combined kinds over LAST blocks (PCQ_PRED_BOUNDS_CLASS / _TIME): the same kernel with a compile-time
//    second column (COL_U8: the class block, COL_F64: the time block), whose loads ride in the same software pipeline.  Each
//    tile's 256 class bytes (one dword per lane) or 256 times (two dwordx4 per lane) are tested per lane into a verdict word;
//    one ds_bpermute per (load, start phase) brings each point's verdict to the lane that holds its first dword, where it is
//    ANDed into the mask algebra before the popcount.  13 / 20 B per point.
// The kernel shapes these replaced (256-thread blocks, unpipelined one-wave forms, other tile counts) live
// in csrc/lab/scan_count_lab.hip and are built only into libpcq_lab.so for the sweeps in tools/.
#include <vector>

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

// The second column as K1's last argument: none (the plain K1, k_bounds_count_w1_pipe<2>), ClassBytes (PCQ_PRED_BOUNDS_CLASS)
// or GpsTimes (PCQ_PRED_BOUNDS_TIME), at the body's first point (class bytes: any alignment; times: 8-byte aligned).
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
__device__ __forceinline__ const uint8_t *col_ptr() { return nullptr; }
template <typename C>
__device__ __forceinline__ const uint8_t *col_ptr(C c) { return c.p; }

template <int TILES, typename... Col>
__global__ __launch_bounds__(64) void k_bounds_count_w1_pipe(const v4i *__restrict__ base, uint64_t n, DevPred pred,
                                                             uint64_t *__restrict__ partials, Col... col) {
    constexpr int COL = ColOf<Col...>::value;
    static_assert(sizeof...(Col) <= 1, "one second column at most");
    const int lane = threadIdx.x;
    const uint64_t tiles = n / TILE_POINTS, steps = tiles / TILES, stride = gridDim.x;
    const LaneBox lb = rotate_box(pred.lo, pred.width, lane);
    const Col2<COL> c2 = col2_setup(col_ptr(col...), pred, lane, IntC<COL>{});
    constexpr int LOADS = TILES * (3 + col2_loads(COL));  // per register set
    uint64_t total = 0;
    if (blockIdx.x < steps) {
        PipeRegs<TILES, COL> A, B;
        uint64_t g = blockIdx.x;
        pipe_load<TILES, COL>(A, base, g, lane, c2);
        for (;;) {
            const uint64_t g1 = g + stride;
            pipe_load<TILES, COL>(B, base, g1 < steps ? g1 : g, lane, c2);  // clamped at the tail: a re-read that hits L2
            pipe_wait<TILES, LOADS, COL>(A);                                 // A has landed, B's loads stay in flight
            total += pipe_eval<TILES, COL>(A, lb, c2);
            if (g1 >= steps) break;
            const uint64_t g2 = g1 + stride;
            pipe_load<TILES, COL>(A, base, g2 < steps ? g2 : g1, lane, c2);
            pipe_wait<TILES, LOADS, COL>(B);
            total += pipe_eval<TILES, COL>(B, lb, c2);
            if (g2 >= steps) break;
            g = g2;
        }
        pipe_wait<TILES, 0, COL>(A);  // the clamped tail prefetch is still in flight: land it before the registers die
        pipe_wait<TILES, 0, COL>(B);
    }
    if (blockIdx.x == 0) {
        for (uint64_t t = steps * TILES; t < tiles; t++) {
            if constexpr (COL == COL_NONE) {
                total += tile_count_masks(base + t * 192, lane, lb);
            } else {
                const v4i *tile = base + t * 192;
                const v4i v[3] = {tile[lane], tile[64 + lane], tile[128 + lane]};
                Col2Regs<COL> r;
                col2_load_plain(r, c2, t);
                total += tile_count_regs<COL>(v, lb, c2, verdict_word(r, c2));
            }
        }
        for (int k = 0; k < 4; k++) {
            const uint64_t p = tiles * TILE_POINTS + (uint64_t)(64 * k + lane);
            bool pass = false;
            if (p < n) {
                const int *q = reinterpret_cast<const int *>(base) + 3 * p;
                pass = ((uint32_t)(q[0] - pred.lo[0]) <= pred.width[0]) & ((uint32_t)(q[1] - pred.lo[1]) <= pred.width[1]) &
                       ((uint32_t)(q[2] - pred.lo[2]) <= pred.width[2]);
                if constexpr (COL != COL_NONE) pass = pass && col2_point(c2, p);
            }
            total += (uint64_t)__popcll(__ballot(pass));
        }
    }
    if (lane == 0) partials[blockIdx.x] = total;
}

// Batched K1, one wave per workgroup, TILES tiles per step, software-pipelined like variants 12..14: while the
// tiles of step u are evaluated the loads of step u + stride are in flight.  Steps are numbered across all
// segments (tile_begin counts steps); each of the two register sets remembers the segment its step came from.
struct SegCursor {
    int s;
    uint64_t begin, end;
    const v4i *base;
    LaneBox lb;
    bool empty;
};
template <int TILES>
__device__ __forceinline__ void seg_seek(SegCursor &c, const DevSegment *__restrict__ segs, int nseg, uint64_t u, int lane) {
    if (u < c.end) return;
    while (c.s + 1 < nseg && u >= segs[c.s + 1].tile_begin) c.s++;
    c.begin = segs[c.s].tile_begin;
    c.end = c.begin + segs[c.s].n / ((uint64_t)TILES * TILE_POINTS);
    c.base = reinterpret_cast<const v4i *>(segs[c.s].xyz);
    c.empty = segs[c.s].empty != 0;
    // the box through SGPRs: left to itself the compiler turns "select of table entries" into a per-lane address and
    // a VECTOR load, and the s_waitcnt vmcnt(0) behind that load would drain the prefetched tiles
    int32_t lo[3];
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = segs[c.s].lo[k];
        w[k] = segs[c.s].width[k];
        asm volatile("" : "+s"(lo[k]), "+s"(w[k]));
    }
    c.lb = rotate_box(lo, w, lane);
}

template <int TILES>
__global__ __launch_bounds__(64) void k_bounds_count_batch_pipe(const DevSegment *__restrict__ segs, int nseg,
                                                               uint64_t total_steps, uint64_t *__restrict__ partials) {
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    const int lane = threadIdx.x;
    const uint64_t stride = gridDim.x;
    uint64_t total = 0;
    if (blockIdx.x < total_steps) {
        PipeRegs<TILES> A, B;
        SegCursor ca = {0, 0, 0, nullptr, {}, true}, cb;
        uint64_t u = blockIdx.x;
        seg_seek<TILES>(ca, segs, nseg, u, lane);
        pipe_load<TILES>(A, ca.base, u - ca.begin, lane);
        for (;;) {
            const uint64_t u1 = u + stride;
            cb = ca;
            if (u1 < total_steps) seg_seek<TILES>(cb, segs, nseg, u1, lane);
            pipe_load<TILES>(B, cb.base, (u1 < total_steps ? u1 : u) - cb.begin, lane);  // clamped at the tail: an L2 hit
            pipe_wait<TILES, 3 * TILES>(A);
            if (!ca.empty) total += pipe_eval<TILES>(A, ca.lb);
            if (u1 >= total_steps) break;
            const uint64_t u2 = u1 + stride;
            ca = cb;
            if (u2 < total_steps) seg_seek<TILES>(ca, segs, nseg, u2, lane);
            pipe_load<TILES>(A, ca.base, (u2 < total_steps ? u2 : u1) - ca.begin, lane);
            pipe_wait<TILES, 3 * TILES>(B);
            if (!cb.empty) total += pipe_eval<TILES>(B, cb.lb);
            if (u2 >= total_steps) break;
            u = u2;
        }
        pipe_wait<TILES, 0>(A);
        pipe_wait<TILES, 0>(B);
    }
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {  // fewer-than-a-step leftovers of segment i
        if (segs[i].empty) continue;
        const uint64_t n = segs[i].n;
        const int *q0 = reinterpret_cast<const int *>(segs[i].xyz);
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < ((n + 63) & ~63ull); p += 64) {
            bool pass = false;
            if (p < n) {
                const int *q = q0 + 3 * p;
                pass = ((uint32_t)(q[0] - segs[i].lo[0]) <= segs[i].width[0]) &
                       ((uint32_t)(q[1] - segs[i].lo[1]) <= segs[i].width[1]) &
                       ((uint32_t)(q[2] - segs[i].lo[2]) <= segs[i].width[2]);
            }
            total += (uint64_t)__popcll(__ballot(pass));
        }
    }
    if (lane == 0) partials[blockIdx.x] = total;
}

// The class segments live in the same device table as the bounds segments, at DevSegment pitch.
__device__ __forceinline__ const DevClassSegment &cseg(const DevSegment *raw, int i) {
    return *reinterpret_cast<const DevClassSegment *>(raw + i);
}

// Batched K2, one wave per workgroup, LOADS 1 KiB loads per step, software-pipelined like k_bounds_count_batch_pipe.
template <int LOADS>
struct ClassRegs {
    v4i r[LOADS];
};
template <int LOADS>
__device__ __forceinline__ void class_load(ClassRegs<LOADS> &R, const v4i *tile, int lane) {
#pragma unroll
    for (int k = 0; k < LOADS; k++) {
        const v4i *q = tile + 64 * k + lane;
        asm volatile("global_load_dwordx4 %0, %1, off nt" : "=&v"(R.r[k]) : "v"(q) : "memory");
    }
}
template <int LOADS, int PENDING>
__device__ __forceinline__ void class_wait(ClassRegs<LOADS> &R) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PENDING) : "memory");
#pragma unroll
    for (int k = 0; k < LOADS; k++) asm volatile("" : "+v"(R.r[k])::"memory");
}
template <int LOADS>
__device__ __forceinline__ uint32_t class_eval(const ClassRegs<LOADS> &R, uint32_t pat) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < LOADS; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) c += __popc(zero_bytes((uint32_t)R.r[k][j] ^ pat));
    return c;
}
struct ClassCursor {
    int s;
    uint64_t begin, end;
    const v4i *body;
    uint32_t pat;
};
template <int LOADS>
__device__ __forceinline__ void class_seek(ClassCursor &c, const DevSegment *__restrict__ raw, int nseg, uint64_t u) {
    if (u < c.end) return;
    while (c.s + 1 < nseg && u >= cseg(raw, c.s + 1).tile_begin) c.s++;
    c.begin = cseg(raw, c.s).tile_begin;
    c.end = c.begin + cseg(raw, c.s).nvec / (64ull * LOADS);
    c.body = reinterpret_cast<const v4i *>(cseg(raw, c.s).cls + cseg(raw, c.s).head);
    c.pat = cseg(raw, c.s).pat;
}

template <int LOADS>
__global__ __launch_bounds__(64) void k_class_count_batch_pipe(const DevSegment *__restrict__ raw, int nseg, uint64_t total_steps,
                                                              uint64_t *__restrict__ partials) {
    constexpr uint64_t STEP_VEC = 64 * LOADS;
    const int lane = threadIdx.x;
    const uint64_t stride = gridDim.x;
    uint32_t cnt = 0;
    if (blockIdx.x < total_steps) {
        ClassRegs<LOADS> A, B;
        ClassCursor ca = {0, 0, 0, nullptr, 0}, cb;
        uint64_t u = blockIdx.x;
        class_seek<LOADS>(ca, raw, nseg, u);
        class_load<LOADS>(A, ca.body + (u - ca.begin) * STEP_VEC, lane);
        for (;;) {
            const uint64_t u1 = u + stride;
            cb = ca;
            if (u1 < total_steps) class_seek<LOADS>(cb, raw, nseg, u1);
            class_load<LOADS>(B, cb.body + ((u1 < total_steps ? u1 : u) - cb.begin) * STEP_VEC, lane);
            class_wait<LOADS, LOADS>(A);
            cnt += class_eval<LOADS>(A, ca.pat);
            if (u1 >= total_steps) break;
            const uint64_t u2 = u1 + stride;
            ca = cb;
            if (u2 < total_steps) class_seek<LOADS>(ca, raw, nseg, u2);
            class_load<LOADS>(A, ca.body + ((u2 < total_steps ? u2 : u1) - ca.begin) * STEP_VEC, lane);
            class_wait<LOADS, LOADS>(B);
            cnt += class_eval<LOADS>(B, cb.pat);
            if (u2 >= total_steps) break;
            u = u2;
        }
        class_wait<LOADS, 0>(A);
        class_wait<LOADS, 0>(B);
    }
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {
        const DevClassSegment g = cseg(raw, i);
        const uint8_t c8 = (uint8_t)(g.pat & 0xff);
        const v4i *bd = reinterpret_cast<const v4i *>(g.cls + g.head);
        for (uint64_t v = (g.nvec / STEP_VEC) * STEP_VEC + lane; v < g.nvec; v += 64) {
            const v4i a = bd[v];
#pragma unroll
            for (int j = 0; j < 4; j++) cnt += __popc(zero_bytes((uint32_t)a[j] ^ g.pat));
        }
        if (lane < 16) {
            const uint64_t p = lane;
            if (p < g.head && g.cls[p] == c8) cnt++;
        } else if (lane < 32) {
            const uint64_t p = g.head + 16 * g.nvec + (lane - 16);
            if (p < g.n && g.cls[p] == c8) cnt++;
        }
    }
    uint64_t w = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) w += __shfl_down((unsigned long long)w, off, 64);
    if (lane == 0) partials[blockIdx.x] = w;
}

// Per-file K2 in the same shape: one wave per workgroup, LOADS KiB per step, software-pipelined.
template <int LOADS>
__global__ __launch_bounds__(64) void k_class_count_pipe(const uint8_t *__restrict__ cls, uint64_t n, uint32_t pat, uint64_t head,
                                                        uint64_t nvec, uint64_t *__restrict__ partials) {
    constexpr uint64_t STEP_VEC = 64 * LOADS;
    const int lane = threadIdx.x;
    const v4i *body = reinterpret_cast<const v4i *>(cls + head);
    const uint64_t steps = nvec / STEP_VEC, stride = gridDim.x;
    uint32_t cnt = 0;
    if (blockIdx.x < steps) {
        ClassRegs<LOADS> A, B;
        uint64_t u = blockIdx.x;
        class_load<LOADS>(A, body + u * STEP_VEC, lane);
        for (;;) {
            const uint64_t u1 = u + stride;
            class_load<LOADS>(B, body + (u1 < steps ? u1 : u) * STEP_VEC, lane);
            class_wait<LOADS, LOADS>(A);
            cnt += class_eval<LOADS>(A, pat);
            if (u1 >= steps) break;
            const uint64_t u2 = u1 + stride;
            class_load<LOADS>(A, body + (u2 < steps ? u2 : u1) * STEP_VEC, lane);
            class_wait<LOADS, LOADS>(B);
            cnt += class_eval<LOADS>(B, pat);
            if (u2 >= steps) break;
            u = u2;
        }
        class_wait<LOADS, 0>(A);
        class_wait<LOADS, 0>(B);
    }
    if (blockIdx.x == 0) {
        const uint8_t c8 = (uint8_t)(pat & 0xff);
        for (uint64_t v = steps * STEP_VEC + lane; v < nvec; v += 64) {  // fewer than a step of leftover vectors
            const v4i a = body[v];
#pragma unroll
            for (int j = 0; j < 4; j++) cnt += __popc(zero_bytes((uint32_t)a[j] ^ pat));
        }
        if (lane < 16) {  // head: [0, head)   tail: [head + 16*nvec, n)   (each < 16 bytes)
            const uint64_t p = lane;
            if (p < head && cls[p] == c8) cnt++;
        } else if (lane < 32) {
            const uint64_t p = head + 16 * nvec + (lane - 16);
            if (p < n && cls[p] == c8) cnt++;
        }
    }
    uint64_t w = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) w += __shfl_down((unsigned long long)w, off, 64);
    if (lane == 0) partials[blockIdx.x] = w;
}

__global__ __launch_bounds__(BLOCK) void k_finish_count(const uint64_t *__restrict__ partials, int nblocks,
                                                        uint64_t *__restrict__ d_count) {
    __shared__ uint64_t s[BLOCK];
    uint64_t t = 0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) t += partials[i];
    s[threadIdx.x] = t;
    __syncthreads();
    for (int off = BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd((unsigned long long *)d_count, (unsigned long long)s[0]);
}

}  // namespace

template <typename... Col>
static int launch_k1(pcq_ctx *ctx, const void *d_xyz, uint64_t n, const DevPred &pred, uint64_t *d_count, hipStream_t s, Col... col) {
    if (n == 0 || pred.empty) return PCQ_OK;
    if (((uintptr_t)d_xyz & 15) != 0) return pcq_fail(PCQ_ERR_ARG, "bounds_count_xyz12: positions block must be 16-byte aligned");
    const uint64_t units = n / ((uint64_t)K1_TILES * TILE_POINTS) + 1;
    uint64_t g = (uint64_t)ctx->num_cus * K1_WAVES_PER_CU;
    if (g > units) g = units;
    int rc = pcq_ensure_partials(ctx, (size_t)g);
    if (rc) return rc;
    hipLaunchKernelGGL((k_bounds_count_w1_pipe<K1_TILES, Col...>), dim3((unsigned)g), dim3(64), 0, s, reinterpret_cast<const v4i *>(d_xyz), n, pred,
                       ctx->d_partials, col...);
    hipLaunchKernelGGL(k_finish_count, dim3(1), dim3(BLOCK), 0, s, ctx->d_partials, (int)g, d_count);
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}

int pcq_launch_bounds_count_xyz12(pcq_ctx *ctx, const void *d_xyz, uint64_t n, const DevPred &pred,
                                  uint64_t *d_count, hipStream_t s) {
    return launch_k1(ctx, d_xyz, n, pred, d_count, s);
}

int pcq_launch_bounds_count_xyz12_col(pcq_ctx *ctx, const void *d_xyz, const void *d_col, uint64_t n, const DevPred &pred, uint64_t *d_count,
                                      hipStream_t s) {
    if (pred.kind == PCQ_PRED_BOUNDS_CLASS) return launch_k1(ctx, d_xyz, n, pred, d_count, s, ClassBytes{(const uint8_t *)d_col});
    if (pred.kind != PCQ_PRED_BOUNDS_TIME) return pcq_fail(PCQ_ERR_ARG, "bounds_count_xyz12_col: predicate kind %d", pred.kind);
    if (((uintptr_t)d_col & 7) != 0) return pcq_fail(PCQ_ERR_ARG, "bounds_count_xyz12_col: time block must be 8-byte aligned");
    return launch_k1(ctx, d_xyz, n, pred, d_count, s, GpsTimes{(const uint8_t *)d_col});
}

int pcq_launch_class_count_u8(pcq_ctx *ctx, const void *d_cls, uint64_t n, uint8_t cls, uint64_t *d_count,
                              hipStream_t s) {
    if (n == 0) return PCQ_OK;
    uint64_t head = (uint64_t)((16 - ((uintptr_t)d_cls & 15)) & 15);
    if (head > n) head = n;
    const uint64_t nvec = (n - head) / 16;
    const uint32_t pat = 0x01010101u * (uint32_t)cls;
    uint64_t g = (uint64_t)ctx->num_cus * K2_WAVES_PER_CU;
    const uint64_t steps = nvec / (64 * K2_LOADS) + 1;
    if (g > steps) g = steps;
    int rc = pcq_ensure_partials(ctx, (size_t)g);
    if (rc) return rc;
    hipLaunchKernelGGL(k_class_count_pipe<K2_LOADS>, dim3((unsigned)g), dim3(64), 0, s, reinterpret_cast<const uint8_t *>(d_cls), n, pat, head,
                       nvec, ctx->d_partials);
    hipLaunchKernelGGL(k_finish_count, dim3(1), dim3(BLOCK), 0, s, ctx->d_partials, (int)g, d_count);
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}

extern "C" int pcq_scan_dev_count_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds,
                                        size_t nsegments, uint64_t *device_total, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || !device_total)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_count_batch: null argument");
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    {
        const int src = pcq_scratch_stream(ctx, s);
        if (src) return src;
    }
    if (nsegments > ctx->segments_cap) {
        if (ctx->d_segments) (void)hipFree(ctx->d_segments);
        if (ctx->h_segments) (void)hipHostFree(ctx->h_segments);
        ctx->d_segments = nullptr;
        ctx->h_segments = nullptr;
        ctx->segments_cap = 0;
        ctx->segments_uploaded = 0;
        size_t cap = nsegments < 64 ? 64 : nsegments;
        PCQ_HIP(hipMalloc((void **)&ctx->d_segments, cap * sizeof(DevSegment)));
        PCQ_HIP(hipHostMalloc((void **)&ctx->h_segments, cap * sizeof(DevSegment), hipHostMallocDefault));
        ctx->segments_cap = cap;
    }
    static_assert(sizeof(DevClassSegment) <= sizeof(DevSegment), "the two segment tables share one buffer");
    const int kind = preds[0].kind;
    // Build the segment table; it is uploaded only when it differs from the one already in HBM
    // (a repeated query re-launches without touching the pinned buffer, so no host-side wait).
    std::vector<DevSegment> table(nsegments);
    memset(table.data(), 0, nsegments * sizeof(DevSegment));
    uint64_t steps = 0;
    for (size_t i = 0; i < nsegments; i++) {
        if (preds[i].kind != kind) return pcq_fail(PCQ_ERR_ARG, "count_batch: mixed predicate kinds");
        if (kind == PCQ_PRED_CLASS) {
            if (cols[i].cls_stride != 1 || (!cols[i].cls && cols[i].n))
                return pcq_fail(PCQ_ERR_ARG, "count_batch: LAST classification blocks only (stride 1)");
            DevClassSegment g;
            memset(&g, 0, sizeof g);
            g.cls = (const uint8_t *)cols[i].cls;
            g.n = cols[i].n;
            g.head = (uint64_t)((16 - ((uintptr_t)g.cls & 15)) & 15);
            if (g.head > g.n) g.head = g.n;
            g.nvec = (g.n - g.head) / 16;
            g.tile_begin = steps;
            g.pat = 0x01010101u * (uint32_t)preds[i].cls;
            memcpy(&table[i], &g, sizeof g);
            steps += g.nvec / (64 * (uint64_t)K2_LOADS);
            continue;
        }
        if (kind != PCQ_PRED_BOUNDS) return pcq_fail(PCQ_ERR_ARG, "count_batch: bad predicate kind %d", kind);
        if (cols[i].xyz_stride != 12) return pcq_fail(PCQ_ERR_ARG, "count_batch: LAST positions blocks only (stride 12)");
        if (((uintptr_t)cols[i].xyz & 15) != 0) return pcq_fail(PCQ_ERR_ARG, "count_batch: positions block %zu not 16-byte aligned", i);
        DevPred dp;
        int rc = pcq_make_dev_pred(&preds[i], &dp);
        if (rc) return rc;
        DevSegment &g = table[i];
        g.xyz = reinterpret_cast<const int4 *>(cols[i].xyz);
        g.n = cols[i].n;
        g.tile_begin = steps;
        for (int a = 0; a < 3; a++) g.lo[a] = dp.lo[a], g.width[a] = dp.width[a];
        g.empty = dp.empty;
        steps += cols[i].n / ((uint64_t)K1_TILES * TILE_POINTS);
    }
    if (ctx->segments_uploaded != nsegments || ctx->segments_kind != kind ||
        memcmp(ctx->h_segments, table.data(), nsegments * sizeof(DevSegment)) != 0) {
        PCQ_HIP(hipStreamSynchronize(s));  // the previous upload from the pinned table must have been consumed
        memcpy(ctx->h_segments, table.data(), nsegments * sizeof(DevSegment));
        PCQ_HIP(hipMemcpyAsync(ctx->d_segments, ctx->h_segments, nsegments * sizeof(DevSegment), hipMemcpyHostToDevice, s));
        ctx->segments_uploaded = nsegments;
        ctx->segments_kind = kind;
    }
    uint64_t g = (uint64_t)ctx->num_cus * (kind == PCQ_PRED_CLASS ? K2_WAVES_PER_CU : K1_WAVES_PER_CU);
    if (g > steps + nsegments) g = steps + nsegments;
    int rc = pcq_ensure_partials(ctx, (size_t)g);
    if (rc) return rc;
    if (kind == PCQ_PRED_CLASS)
        hipLaunchKernelGGL(k_class_count_batch_pipe<K2_LOADS>, dim3((unsigned)g), dim3(64), 0, s, ctx->d_segments, (int)nsegments, steps, ctx->d_partials);
    else
        hipLaunchKernelGGL(k_bounds_count_batch_pipe<K1_TILES>, dim3((unsigned)g), dim3(64), 0, s, ctx->d_segments, (int)nsegments, steps, ctx->d_partials);
    hipLaunchKernelGGL(k_finish_count, dim3(1), dim3(BLOCK), 0, s, ctx->d_partials, (int)g, device_total);
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}
