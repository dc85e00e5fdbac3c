// chunk_index.hip — on-the-fly chunk index for device-resident LAST columns.
//
// The reference's authors list this as their own next step (improvements.md:3-10): "while scanning
// first (without an index) we can create a chunk header for each chunk, but only for the queried
// attribute(s): if we query by bounds, we compute an AABB for each chunk; if we query by object class,
// a class histogram ... upon further scans, we first consult the index to find the matching chunks".
//
// Parts.  An index object holds up to three parts of one type (IndexPart), each a side output of the first scan that needs it
// and kept for as long as its column's pointer and n stay the same (ensure_part):
//   * boxes: the integer AABB of every 4096-point chunk of the positions (24 B per 48 KiB);
//   * histograms: 256 bins per 65536-point chunk of the class bytes;
//   * time records: the minimum and maximum of every 4096-point chunk's non-NaN GPS times and the number of its NaNs (24 B per
//     32 KiB).  A file in acquisition order is close to monotone in time and coherent in space, so most chunks are disjoint
//     from a query.
// Every chunk takes a state from its records (pcq_internal.h: index_box_state, index_class_state, index_time_state, combined by
// index_combined_state): disjoint -> skipped, contained -> counted without reading a byte, straddling -> read.
//
// Plan.  index_plan.h says, per predicate kind and as data, which parts a scan prunes with and what follows from that:
//
//   kind (entry)                    parts          chunks                 building call, count collector        ragged tail advances
//   BOUNDS (_indexed)               boxes          n / 4096               the builder counts on its way         xyz; no cls
//   CLASS (_indexed)                hist           ceil(n / 65536)        built, then bins summed (no partials)  none
//   BOUNDS_CLASS (_combined)        boxes + hist   n / 4096 (class: /16)  built silently, pruned pass always    xyz, cls + 1 per point
//   TIME (_time)                    times          n / 4096               the builder counts on its way         cls + 8 per point, xyz if any
//   BOUNDS_TIME (_bounds_time)      boxes + times  n / 4096               built silently, pruned pass always    xyz, cls + 8 per point
//
// Driver.  The four entries check their arguments and call indexed_scan, which holds the one skeleton: validate; fall through to
// pcq_scan_dev with all-zero statistics where the plan does not cover the layout; build the missing parts; then either hand an
// EmitIndex to the buffer emit of scan_generic.hip (its count pass takes each 2048-point tile's state from the index first:
// k_tile_counts with IDX; the statistics of such a scan are classified when they are asked for, k_index_emit_stats), or run the
// pruned count kernel, the finish, and the plain scan of the ragged tail.  A one-part kind's building count is the builder's own
// (built = 1, scanned = chunks); a class count is a sum of one bin per chunk and reads no class byte at all.
// Results are identical to the unindexed scans (tests/test_gpu_index*.py).  The index never takes part in bench.py: skipping work
// inside the timed region would invalidate the north-star measurement.
#include <new>

#include "pcq_internal.h"
#include "scan_tiles.h"

namespace {

constexpr int WAVES = 4;
constexpr int CHUNK_TILES = 16;                           // 16 wave-tiles = 4096 points = 48 KiB
constexpr uint64_t CHUNK_POINTS = (uint64_t)CHUNK_TILES * TILE_POINTS;
constexpr uint64_t CLASS_CHUNK = 65536;

// (BLOCK, TILE_POINTS, LaneBox, rotate_box, ld_nt and the mask algebra tile_count_regs: scan_tiles.h)

struct ChunkBox {  // integer AABB of one chunk
    int32_t mn[3], mx[3];
};

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// First bounds scan: count + per-chunk AABB in one pass.  One block per chunk iteration; each of the
// four waves takes four of the chunk's sixteen tiles.
__global__ __launch_bounds__(BLOCK) void k_index_build_bounds(const v4i *__restrict__ base, uint64_t nchunks, DevPred pred,
                                                              ChunkBox *__restrict__ boxes, uint64_t *__restrict__ partials) {
    __shared__ int s_mn[WAVES][3], s_mx[WAVES][3];
    __shared__ uint64_t s_cnt[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LaneBox lb = rotate_box(pred.lo, pred.width, lane);
    const int r = lane % 3;
    uint64_t total = 0;
    for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        int mn[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, mx[3] = {INT32_MIN, INT32_MIN, INT32_MIN};  // per ROTATED component
#pragma unroll
        for (int q = 0; q < CHUNK_TILES / WAVES; q++) {
            const v4i *tile = base + (ch * CHUNK_TILES + (uint64_t)wave * (CHUNK_TILES / WAVES) + q) * 192;
            v4i v[3];
            v[0] = ld_nt(tile + lane);
            v[1] = ld_nt(tile + 64 + lane);
            v[2] = ld_nt(tile + 128 + lane);
            if (!pred.empty) total += tile_count_regs(v, lb);
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int t = (k + j) % 3;  // dword (k, lane, j) is component (lane%3 + t) % 3
                    mn[t] = min(mn[t], v[k][j]);
                    mx[t] = max(mx[t], v[k][j]);
                }
        }
        // un-rotate: actual component c lives in rotated slot (c - r + 3) % 3
        int amn[3], amx[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int t = (c - r + 3) % 3;
            amn[c] = t == 0 ? mn[0] : (t == 1 ? mn[1] : mn[2]);
            amx[c] = t == 0 ? mx[0] : (t == 1 ? mx[1] : mx[2]);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int a = wave_min(amn[c]), b = wave_max(amx[c]);
            if (lane == 0) s_mn[wave][c] = a, s_mx[wave][c] = b;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const int c = threadIdx.x;
            int a = s_mn[0][c], b = s_mx[0][c];
            for (int w = 1; w < WAVES; w++) a = min(a, s_mn[w][c]), b = max(b, s_mx[w][c]);
            boxes[ch].mn[c] = a;
            boxes[ch].mx[c] = b;
        }
        __syncthreads();
    }
    if (lane == 0) s_cnt[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// stats[0..2] += the chunks a block skipped / counted whole / scanned (its thread 0, once)
__device__ __forceinline__ void chunk_stats_out(uint32_t n_skip, uint32_t n_full, uint32_t n_scan, unsigned long long *__restrict__ stats) {
    if (n_skip) atomicAdd(&stats[0], (unsigned long long)n_skip);
    if (n_full) atomicAdd(&stats[1], (unsigned long long)n_full);
    if (n_scan) atomicAdd(&stats[2], (unsigned long long)n_scan);
}

// The three pruned counts over positions below (bounds, box AND class, box AND time) are one loop written out three times:
// classify / skip / whole / scan sixteen tiles, with K1's second column or without.  Folded into one device template (state as a
// callable, second column as COL of scan_tiles.h) the compiler schedules two of the three differently, and k_index_count_bounds
// changes as soon as it calls index_box_state instead of its own hoisted copy (profiles/index_driver_asm_compare.log).  These
// kernels were shaped by measurement (profiles/r10_index_count_shape.log), so they stay as they are; only the epilogue is shared.
//
// Later bounds scans: classify each chunk, read only the straddling ones.  stats[0..2] += chunks
// skipped / counted whole / scanned.
__global__ __launch_bounds__(BLOCK) void k_index_count_bounds(const v4i *__restrict__ base, uint64_t nchunks, DevPred pred,
                                                              const ChunkBox *__restrict__ boxes, uint64_t *__restrict__ partials,
                                                              unsigned long long *__restrict__ stats) {
    __shared__ uint64_t s_cnt[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LaneBox lb = rotate_box(pred.lo, pred.width, lane);
    int64_t hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) hi[a] = (int64_t)pred.lo[a] + (int64_t)pred.width[a];
    uint64_t total = 0;
    uint32_t n_skip = 0, n_full = 0, n_scan = 0;
    for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const ChunkBox cb = boxes[ch];  // block-uniform
        bool disjoint = pred.empty != 0, inside = !pred.empty;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            disjoint |= (int64_t)cb.mx[a] < (int64_t)pred.lo[a] || (int64_t)cb.mn[a] > hi[a];
            inside &= (int64_t)cb.mn[a] >= (int64_t)pred.lo[a] && (int64_t)cb.mx[a] <= hi[a];
        }
        if (disjoint) {
            n_skip++;
            continue;
        }
        if (inside) {
            if (threadIdx.x == 0) total += CHUNK_POINTS;
            n_full++;
            continue;
        }
        n_scan++;
#pragma unroll
        for (int q = 0; q < CHUNK_TILES / WAVES; q++) {
            const v4i *tile = base + (ch * CHUNK_TILES + (uint64_t)wave * (CHUNK_TILES / WAVES) + q) * 192;
            v4i v[3];
            v[0] = ld_nt(tile + lane);
            v[1] = ld_nt(tile + 64 + lane);
            v[2] = ld_nt(tile + 128 + lane);
            const uint32_t c = tile_count_regs(v, lb);
            if (lane == 0) total += c;
        }
    }
    // `total` was accumulated on lane 0 of each wave (thread 0 for whole chunks)
    if (lane == 0) s_cnt[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        chunk_stats_out(n_skip, n_full, n_scan, stats);
    }
}

// Box AND class (pcq_scan_dev_indexed_combined): each 4096-point chunk takes its box state together with the state of the
// 65536-point class chunk it lies in (index_combined_state).  Only SCAN chunks are read: their positions and their 4096 class
// bytes, tested tile by tile as K1 does with its second column (scan_tiles.h, COL_U8; the class block at any alignment).
__global__ __launch_bounds__(BLOCK) void k_index_count_bounds_class(const v4i *__restrict__ base, const uint8_t *__restrict__ cls, uint64_t n,
                                                                    uint64_t nchunks, DevPred pred, const ChunkBox *__restrict__ boxes,
                                                                    const uint32_t *__restrict__ hist, uint64_t *__restrict__ partials,
                                                                    unsigned long long *__restrict__ stats) {
    __shared__ uint64_t s_cnt[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LaneBox lb = rotate_box(pred.lo, pred.width, lane);
    const Col2<COL_U8> c2 = col2_setup(cls, pred, lane, IntC<COL_U8>{});
    uint64_t total = 0;
    uint32_t n_skip = 0, n_full = 0, n_scan = 0;
    for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const ChunkBox cb = boxes[ch];  // block-uniform
        const uint64_t cch = ch / (CLASS_CHUNK / CHUNK_POINTS), first = cch * CLASS_CHUNK;
        const int st = index_combined_state(index_box_state(cb.mn, cb.mx, pred),
                                            index_class_state(hist[cch * 256 + (pred.cls & 255u)], n - first < CLASS_CHUNK ? n - first : CLASS_CHUNK));
        if (st == CHUNK_NONE) {
            n_skip++;
            continue;
        }
        if (st == CHUNK_ALL) {
            if (threadIdx.x == 0) total += CHUNK_POINTS;
            n_full++;
            continue;
        }
        n_scan++;
#pragma unroll
        for (int q = 0; q < CHUNK_TILES / WAVES; q++) {
            const uint64_t t = ch * CHUNK_TILES + (uint64_t)wave * (CHUNK_TILES / WAVES) + q;
            const v4i *tile = base + t * 192;
            v4i v[3];
            v[0] = ld_nt(tile + lane);
            v[1] = ld_nt(tile + 64 + lane);
            v[2] = ld_nt(tile + 128 + lane);
            Col2Regs<COL_U8> r;
            col2_load_plain(r, c2, t);
            const uint32_t c = tile_count_regs<COL_U8>(v, lb, c2, verdict_word(r, c2));
            if (lane == 0) total += c;
        }
    }
    if (lane == 0) s_cnt[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        chunk_stats_out(n_skip, n_full, n_scan, stats);
    }
}

// Box AND time (pcq_scan_dev_indexed_bounds_time): each 4096-point chunk takes its box state together with the state of its own
// time record (index_combined_state; both parts have the same chunks).  Only SCAN chunks are read: their 48 KiB of positions and
// their 32 KiB of times, tested tile by tile as K1 does with its second column (scan_tiles.h, COL_F64).  The shape of
// k_index_count_bounds_class: a tile's five loads are issued together and evaluated before the next tile's.
__global__ __launch_bounds__(BLOCK) void k_index_count_bounds_time(const v4i *__restrict__ base, const uint8_t *__restrict__ times, uint64_t nchunks,
                                                                   DevPred pred, const ChunkBox *__restrict__ boxes,
                                                                   const ChunkTime *__restrict__ recs, uint64_t *__restrict__ partials,
                                                                   unsigned long long *__restrict__ stats) {
    __shared__ uint64_t s_cnt[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LaneBox lb = rotate_box(pred.lo, pred.width, lane);
    const Col2<COL_F64> c2 = col2_setup(times, pred, lane, IntC<COL_F64>{});
    uint64_t total = 0;
    uint32_t n_skip = 0, n_full = 0, n_scan = 0;
    for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const ChunkBox cb = boxes[ch];  // block-uniform
        const int st = index_combined_state(index_box_state(cb.mn, cb.mx, pred), index_time_state(recs[ch], c2.t0, c2.t1));
        if (st == CHUNK_NONE) {
            n_skip++;
            continue;
        }
        if (st == CHUNK_ALL) {
            if (threadIdx.x == 0) total += CHUNK_POINTS;
            n_full++;
            continue;
        }
        n_scan++;
#pragma unroll
        for (int q = 0; q < CHUNK_TILES / WAVES; q++) {
            const uint64_t t = ch * CHUNK_TILES + (uint64_t)wave * (CHUNK_TILES / WAVES) + q;
            const v4i *tile = base + t * 192;
            v4i v[3];
            v[0] = ld_nt(tile + lane);
            v[1] = ld_nt(tile + 64 + lane);
            v[2] = ld_nt(tile + 128 + lane);
            Col2Regs<COL_F64> r;
            col2_load_plain(r, c2, t);
            const uint32_t c = tile_count_regs<COL_F64>(v, lb, c2, verdict_word(r, c2));
            if (lane == 0) total += c;
        }
    }
    if (lane == 0) s_cnt[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        chunk_stats_out(n_skip, n_full, n_scan, stats);
    }
}

// First class scan: 256-bin histogram per 65536-point chunk (LDS atomics), one block per chunk.
__global__ __launch_bounds__(BLOCK) void k_index_build_class(const uint8_t *__restrict__ cls, uint64_t n, uint64_t nchunks,
                                                             uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_h[256];
    for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        s_h[threadIdx.x] = 0;
        __syncthreads();
        const uint64_t first = ch * CLASS_CHUNK;
        const uint64_t cnt = n - first < CLASS_CHUNK ? n - first : CLASS_CHUNK;
        for (uint64_t i = threadIdx.x; i < cnt; i += BLOCK) atomicAdd(&s_h[cls[first + i]], 1u);
        __syncthreads();
        hist[ch * 256 + threadIdx.x] = s_h[threadIdx.x];
        __syncthreads();
    }
}

__global__ __launch_bounds__(BLOCK) void k_index_count_class(const uint32_t *__restrict__ hist, uint64_t nchunks, uint32_t cls,
                                                             uint64_t *__restrict__ d_count) {
    __shared__ uint64_t s[BLOCK];
    uint64_t t = 0;
    for (uint64_t ch = threadIdx.x; ch < nchunks; ch += BLOCK) t += hist[ch * 256 + cls];
    s[threadIdx.x] = t;
    __syncthreads();
    for (int off = BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd((unsigned long long *)d_count, (unsigned long long)s[0]);
}

// ---- GPS time (pcq_scan_dev_indexed_time) ----------------------------------------------------------------------------------
// A chunk's 4096 times are 2048 16-byte vectors of two times: eight loads per thread of a 256-thread block.
constexpr int TIME_LOADS = (int)(CHUNK_POINTS / 2 / BLOCK);
static_assert(TIME_LOADS * 2 * BLOCK == (int)CHUNK_POINTS, "a block reads a time chunk in whole loads");

__device__ __forceinline__ void load_time_chunk(v4i (&v)[TIME_LOADS], const v4i *__restrict__ base, uint64_t ch) {
    const v4i *p = base + ch * (CHUNK_POINTS / 2) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < TIME_LOADS; k++) v[k] = ld_nt(p + k * BLOCK);
}
__device__ __forceinline__ uint32_t count_time_chunk(const v4i (&v)[TIME_LOADS], double t0, double t1) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < TIME_LOADS; k++) c += (uint32_t)t_in(v[k][0], v[k][1], t0, t1) + (uint32_t)t_in(v[k][2], v[k][3], t0, t1);
    return c;
}
// per-thread counts -> partials[blockIdx.x]; `whole` (thread 0): points of the chunks counted without being read
__device__ __forceinline__ void block_count_out(uint32_t cnt, uint64_t whole, uint64_t *__restrict__ partials) {
    __shared__ uint64_t s_cnt[WAVES];
    uint64_t t = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor((unsigned long long)t, off, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3] + whole;
}

// First time scan: count + per-chunk {min, max, NaNs} in one pass.  A NaN loses every compare, so it moves neither extreme.
__global__ __launch_bounds__(BLOCK) void k_index_build_time(const v4i *__restrict__ base, uint64_t nchunks, DevPred pred,
                                                            ChunkTime *__restrict__ recs, uint64_t *__restrict__ partials) {
    __shared__ double s_mn[WAVES], s_mx[WAVES];
    __shared__ uint32_t s_nan[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double t0 = pred.wmin[0], t1 = pred.wmax[0];
    uint32_t cnt = 0;
    for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        v4i v[TIME_LOADS];
        load_time_chunk(v, base, ch);
        if (!pred.empty) cnt += count_time_chunk(v, t0, t1);
        double mn = __longlong_as_double(0x7ff0000000000000ll), mx = -mn;  // +inf, -inf
        uint32_t nans = 0;
#pragma unroll
        for (int k = 0; k < TIME_LOADS; k++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const double t = time_of(v[k][2 * h], v[k][2 * h + 1]);
                mn = t < mn ? t : mn;
                mx = t > mx ? t : mx;
                nans += t != t;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
            nans += __shfl_xor(nans, off, 64);
        }
        if (lane == 0) s_mn[wave] = mn, s_mx[wave] = mx, s_nan[wave] = nans;
        __syncthreads();
        if (threadIdx.x == 0) {
            ChunkTime ct;
            ct.mn = s_mn[0], ct.mx = s_mx[0], ct.nans = s_nan[0], ct._pad = 0;
            for (int w = 1; w < WAVES; w++) {
                ct.mn = s_mn[w] < ct.mn ? s_mn[w] : ct.mn;
                ct.mx = s_mx[w] > ct.mx ? s_mx[w] : ct.mx;
                ct.nans += s_nan[w];
            }
            recs[ch] = ct;
        }
        __syncthreads();
    }
    block_count_out(cnt, 0, partials);
}

// Later time scans: classify each chunk (block-uniform), read only the straddling ones.  All 256 threads read a chunk's times
// together, so this is no index_count_xyz: its loop has no tiles.
__global__ __launch_bounds__(BLOCK) void k_index_count_time(const v4i *__restrict__ base, uint64_t nchunks, DevPred pred,
                                                            const ChunkTime *__restrict__ recs, uint64_t *__restrict__ partials,
                                                            unsigned long long *__restrict__ stats) {
    const double t0 = pred.wmin[0], t1 = pred.wmax[0];
    uint32_t cnt = 0;
    uint64_t whole = 0;
    uint32_t n_skip = 0, n_full = 0, n_scan = 0;
    for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int st = index_time_state(recs[ch], t0, t1);  // block-uniform
        if (st == CHUNK_NONE) {
            n_skip++;
            continue;
        }
        if (st == CHUNK_ALL) {
            whole += CHUNK_POINTS;
            n_full++;
            continue;
        }
        n_scan++;
        v4i v[TIME_LOADS];
        load_time_chunk(v, base, ch);
        cnt += count_time_chunk(v, t0, t1);
    }
    block_count_out(cnt, whole, partials);
    if (threadIdx.x == 0) chunk_stats_out(n_skip, n_full, n_scan, stats);
}

// Statistics of an indexed buffer scan in index-chunk units: stats[0..2] += chunks disjoint from the predicate (not read by
// the count pass) / contained (not read by the count pass) / straddling (read) — the classification k_tile_counts<.., IDX> took
// its tile states from.  boxes alone: a bounds scan; hist alone: a class scan (class chunks); both: box AND class (bounds chunks);
// times alone: a time scan (time chunks); boxes and times: box AND time (the chunks of both).  Launched by pcq_index_get_stats when the statistics are asked for, never on the scan path.
__global__ __launch_bounds__(BLOCK) void k_index_emit_stats(const ChunkBox *__restrict__ boxes, const uint32_t *__restrict__ hist,
                                                            const ChunkTime *__restrict__ times, uint64_t nchunks, uint64_t n, DevPred pred,
                                                            unsigned long long *__restrict__ stats) {
    uint32_t k[3] = {0, 0, 0};
    for (uint64_t ch = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; ch < nchunks; ch += (uint64_t)gridDim.x * BLOCK) {
        int st;
        if (boxes) {
            const ChunkBox cb = boxes[ch];
            st = index_box_state(cb.mn, cb.mx, pred);
            if (hist) {  // box AND class, in bounds chunks
                const uint64_t cch = ch / (CLASS_CHUNK / CHUNK_POINTS), first = cch * CLASS_CHUNK;
                st = index_combined_state(st, index_class_state(hist[cch * 256 + (pred.cls & 255u)], n - first < CLASS_CHUNK ? n - first : CLASS_CHUNK));
            } else if (times) {  // box AND time
                st = index_combined_state(st, index_time_state(times[ch], pred.wmin[0], pred.wmax[0]));
            }
        } else if (times) {
            st = index_time_state(times[ch], pred.wmin[0], pred.wmax[0]);
        } else {
            const uint64_t first = ch * CLASS_CHUNK;
            st = index_class_state(hist[ch * 256 + (pred.cls & 255u)], n - first < CLASS_CHUNK ? n - first : CLASS_CHUNK);
        }
        k[0] += st == CHUNK_NONE, k[1] += st == CHUNK_ALL, k[2] += st == CHUNK_SCAN;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        uint32_t v = k[a];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&stats[a], (unsigned long long)v);
    }
}

}  // namespace
static_assert(sizeof(ChunkBox) == 6 * sizeof(int32_t) && CHUNK_POINTS == INDEX_BOUNDS_CHUNK && CLASS_CHUNK == INDEX_CLASS_CHUNK,
              "EmitIndex reads the boxes as {mn[3], mx[3]}");

// One part of an index object: the records of `chunks` chunks of the column at `col`, as built for n points.
struct IndexPart {
    const void *col = nullptr;
    uint64_t n = 0, chunks = 0;
    void *d = nullptr;
};
struct PartRecords {  // the records of the parts a mask names, nullptr for the others
    const ChunkBox *boxes;
    const uint32_t *hist;
    const ChunkTime *times;
};

struct pcq_index {
    pcq_ctx *ctx = nullptr;
    IndexPart part[INDEX_PARTS];  // boxes, histograms, time records (index_part_slot)
    // statistics of the last indexed scan
    unsigned long long *d_stats = nullptr;
    pcq_index_stats last = {};
    hipStream_t stats_stream = nullptr;  // non-null: `last` must be completed from d_stats (fetched lazily)
    int stats_parts = 0;                 // 0: the scan writes d_stats itself (a count) · a PART_* mask: a buffer scan, classified from
    DevPred stats_pred = {};             //    those parts with stats_pred by pcq_index_get_stats (k_index_emit_stats)
};

static PartRecords part_records(const pcq_index *ix, int mask) {
    const void *d[INDEX_PARTS];
    for (int p = 0; p < INDEX_PARTS; p++) d[p] = (mask & INDEX_PART_BITS[p]) ? ix->part[p].d : nullptr;
    return {(const ChunkBox *)d[index_part_slot(PART_BOXES)], (const uint32_t *)d[index_part_slot(PART_HIST)],
            (const ChunkTime *)d[index_part_slot(PART_TIMES)]};
}

extern "C" int pcq_index_new(pcq_ctx *ctx, pcq_index **out) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !out) return pcq_fail(PCQ_ERR_ARG, "pcq_index_new: null argument");
    *out = nullptr;
    pcq_index *ix = new (std::nothrow) pcq_index();
    if (!ix) return pcq_fail(PCQ_ERR_NOMEM, "pcq_index_new: out of memory");
    ix->ctx = ctx;
    hipError_t e = hipMalloc((void **)&ix->d_stats, 4 * sizeof(unsigned long long));
    if (e != hipSuccess) {
        delete ix;
        return pcq_fail(PCQ_ERR_HIP, "pcq_index_new: %s", hipGetErrorString(e));
    }
    *out = ix;
    return PCQ_OK;
}

extern "C" int pcq_index_free(pcq_index *ix) {
    if (!ix) return PCQ_OK;
    PCQ_ON_DEVICE_OF_CTX(ix->ctx);
    (void)hipDeviceSynchronize();
    for (IndexPart &p : ix->part)
        if (p.d) (void)hipFree(p.d);
    if (ix->d_stats) (void)hipFree(ix->d_stats);
    delete ix;
    return PCQ_OK;
}

extern "C" int pcq_index_get_stats(pcq_index *ix, pcq_index_stats *out) {
    if (!ix || !out) return pcq_fail(PCQ_ERR_ARG, "pcq_index_get_stats: null argument");
    PCQ_ON_DEVICE_OF_CTX(ix->ctx);
    if (ix->stats_stream) {  // the counters of the last indexed scan are still on the device
        unsigned long long h[3] = {0, 0, 0};
        if (ix->stats_parts) {  // a buffer scan: classified now, in the chunks the scan reported
            const uint64_t nch = ix->last.chunks, blocks = (nch + BLOCK - 1) / BLOCK;
            const int grid = (int)(blocks < (uint64_t)ix->ctx->num_cus ? blocks : (uint64_t)ix->ctx->num_cus);
            const PartRecords r = part_records(ix, ix->stats_parts);
            PCQ_HIP(hipMemsetAsync(ix->d_stats, 0, 4 * sizeof(unsigned long long), ix->stats_stream));
            if (grid > 0)
                hipLaunchKernelGGL(k_index_emit_stats, dim3(grid), dim3(BLOCK), 0, ix->stats_stream, r.boxes, r.hist, r.times, nch,
                                   ix->part[index_part_slot(PART_HIST)].n, ix->stats_pred, ix->d_stats);
            PCQ_HIP(hipGetLastError());
        }
        PCQ_HIP(hipStreamSynchronize(ix->stats_stream));
        PCQ_HIP(hipMemcpy(h, ix->d_stats, sizeof h, hipMemcpyDeviceToHost));
        ix->last.skipped = h[0];
        ix->last.whole = h[1];
        ix->last.scanned = h[2];
        ix->stats_stream = nullptr;
    }
    *out = ix->last;
    return PCQ_OK;
}

// The records of `which` (a PART_* bit) for the `chunks` chunks of its column, built on `s` unless the index holds them for this
// column and n already (*had).  The builders of boxes and time records count the matches of `build_with` into the context's
// partials on their way: the real predicate when the building call is a count (one launch builds and counts), one with
// empty = 1 otherwise (the records alone).
static int ensure_part(pcq_ctx *ctx, pcq_index *ix, int which, const pcq_columns *cols, uint64_t chunks, int grid, const DevPred &build_with,
                       hipStream_t s, bool *had) {
    IndexPart &p = ix->part[index_part_slot(which)];
    const void *col = index_part_column(which, *cols);
    *had = p.d && p.col == col && p.n == cols->n;
    if (*had) return PCQ_OK;
    if (p.d) PCQ_HIP(hipFree(p.d));
    p.d = nullptr;
    const size_t record = which == PART_BOXES ? sizeof(ChunkBox) : (which == PART_HIST ? 256 * sizeof(uint32_t) : sizeof(ChunkTime));
    PCQ_HIP(hipMalloc(&p.d, chunks * record));
    switch (which) {
    case PART_BOXES:
        hipLaunchKernelGGL(k_index_build_bounds, dim3(grid), dim3(BLOCK), 0, s, reinterpret_cast<const v4i *>(col), chunks, build_with, (ChunkBox *)p.d,
                           ctx->d_partials);
        break;
    case PART_HIST:
        hipLaunchKernelGGL(k_index_build_class, dim3(grid), dim3(BLOCK), 0, s, (const uint8_t *)col, cols->n, chunks, (uint32_t *)p.d);
        break;
    default:
        hipLaunchKernelGGL(k_index_build_time, dim3(grid), dim3(BLOCK), 0, s, reinterpret_cast<const v4i *>(col), chunks, build_with, (ChunkTime *)p.d,
                           ctx->d_partials);
    }
    PCQ_HIP(hipGetLastError());
    p.col = col;
    p.n = cols->n;
    p.chunks = chunks;
    return PCQ_OK;
}

// The skeleton of the four entries below, which have checked their pointers and their predicate kind; `pl` (index_plan.h) holds
// what differs between the kinds.  An empty plan is a kind the entry serves without an index.
static int indexed_scan(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, const IndexPlan &pl, pcq_index *ix, pcq_collector *c,
                        void *stream, const char *entry) {
    if (c->kind == COLL_GRID) return pcq_fail(PCQ_ERR_ARG, "%s: count and buffer collectors only", entry);
    int rc = pcq_validate_scan(cols, pred, c);  // (before the index or the collector is touched: the kernels below trust the columns)
    if (rc) return rc;
    DevPred dp = {};
    if (pl.parts) {
        rc = pcq_make_dev_pred(pred, &dp);
        if (rc) return rc;
    }
    ix->last = pcq_index_stats{};
    ix->stats_stream = nullptr;
    ix->stats_parts = 0;
    // no index of this kind, a layout it does not cover, a predicate that can match nothing (where the plan says so): the plain
    // scan, statistics that claim nothing, the parts left as they are
    if (!index_covers(pl, *cols) || (pl.live_only && (dp.empty || !(dp.wmin[0] < dp.wmax[0])))) return pcq_scan_dev(ctx, cols, pred, c, stream);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    rc = pcq_scratch_stream(ctx, s);
    if (rc) return rc;
    const bool count = c->kind == COLL_COUNT;
    const uint64_t chunks = index_chunks(pl.unit, cols->n), max_blocks = (uint64_t)ctx->num_cus * 8;
    const int grid = (int)(chunks < max_blocks ? chunks : max_blocks);
    if (!pl.from_hist) {
        rc = pcq_ensure_partials(ctx, (size_t)grid);
        if (rc) return rc;
    }
    DevPred build_with = dp;
    if (!(count && pl.counts_on_build)) build_with.empty = 1;  // the records alone: the pruned pass or the emit counts
    bool missing = false;
    for (int part : INDEX_PART_BITS) {
        if (!(pl.parts & part)) continue;
        const uint64_t pchunks = index_chunks(part, cols->n);
        bool had;
        rc = ensure_part(ctx, ix, part, cols, pchunks, (int)(pchunks < max_blocks ? pchunks : max_blocks), build_with, s, &had);
        if (rc) return rc;
        missing |= !had;
    }
    const bool pruned = !(pl.counts_on_build && missing);  // false: the build of the one part read every chunk, and counted
    const PartRecords r = part_records(ix, pl.parts);
    ix->last.chunks = chunks;
    ix->last.built = missing;
    if (!pruned) ix->last.scanned = chunks;
    if (!count) {
        // A buffer collector: the emit's count pass takes each tile's state from the index (scan_generic.hip, k_tile_counts with
        // IDX), then the records are written as by pcq_scan_dev.  Nothing on the scan path for the statistics: they are
        // classified and fetched by pcq_index_get_stats.
        if (pruned) {
            ix->stats_stream = s;
            ix->stats_parts = pl.parts;
            ix->stats_pred = dp;
        }
        const EmitIndex eix = {reinterpret_cast<const int32_t *>(r.boxes), r.hist, r.times, index_covered_tiles(pl, cols->n)};
        return pcq_scan_dev_impl(ctx, cols, pred, c, s, &eix);
    }
    c->last_stream = s;
    if (pl.from_hist) {
        if (pruned) ix->last.whole = chunks;  // answered from the histograms: no classification byte is read
        hipLaunchKernelGGL(k_index_count_class, dim3(1), dim3(BLOCK), 0, s, r.hist, chunks, (uint32_t)pred->cls, c->d_count);
        PCQ_HIP(hipGetLastError());
        return PCQ_OK;
    }
    if (pruned) {  // (the builders wrote the partials; the pruned count writes every one of the `grid` again before they are summed)
        const v4i *xyz = reinterpret_cast<const v4i *>(cols->xyz);
        PCQ_HIP(hipMemsetAsync(ix->d_stats, 0, 4 * sizeof(unsigned long long), s));
        switch (pl.parts) {
        case PART_BOXES:
            hipLaunchKernelGGL(k_index_count_bounds, dim3(grid), dim3(BLOCK), 0, s, xyz, chunks, dp, r.boxes, ctx->d_partials, ix->d_stats);
            break;
        case PART_TIMES:
            hipLaunchKernelGGL(k_index_count_time, dim3(grid), dim3(BLOCK), 0, s, reinterpret_cast<const v4i *>(cols->cls), chunks, dp, r.times,
                               ctx->d_partials, ix->d_stats);
            break;
        case PART_BOXES | PART_HIST:
            hipLaunchKernelGGL(k_index_count_bounds_class, dim3(grid), dim3(BLOCK), 0, s, xyz, (const uint8_t *)cols->cls, cols->n, chunks, dp, r.boxes,
                               r.hist, ctx->d_partials, ix->d_stats);
            break;
        default:
            hipLaunchKernelGGL(k_index_count_bounds_time, dim3(grid), dim3(BLOCK), 0, s, xyz, (const uint8_t *)cols->cls, chunks, dp, r.boxes, r.times,
                               ctx->d_partials, ix->d_stats);
        }
        ix->stats_stream = s;  // fetched lazily by pcq_index_get_stats: no sync on the scan path
    }
    rc = pcq_launch_finish_counts(ctx, 1, grid, c->d_count, s);
    if (rc) return rc;
    const uint64_t rest_first = chunks * CHUNK_POINTS;
    if (pl.tail && rest_first < cols->n) {  // the ragged end (< one chunk) is always scanned
        const pcq_columns tail = index_tail_columns(pl, *cols, rest_first);
        return pcq_scan_dev(ctx, &tail, pred, c, stream);
    }
    return PCQ_OK;
}

// Bounds through the boxes, class through the histograms.  The other kinds have no index HERE (the time part belongs to the
// entries below): an empty plan.
extern "C" int pcq_scan_dev_indexed(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                                    pcq_collector *c, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !cols || !pred || !ix || !c) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed: null argument");
    const bool own = pred->kind == PCQ_PRED_BOUNDS || pred->kind == PCQ_PRED_CLASS;
    return indexed_scan(ctx, cols, pred, own ? index_plan(pred->kind) : IndexPlan{}, ix, c, stream, "pcq_scan_dev_indexed");
}

// Box AND class through the boxes and the histograms.
extern "C" int pcq_scan_dev_indexed_combined(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                                             pcq_collector *c, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !cols || !pred || !ix || !c) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_combined: null argument");
    if (pred->kind != PCQ_PRED_BOUNDS_CLASS)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_combined: predicate kind %d (PCQ_PRED_BOUNDS_CLASS only)", pred->kind);
    return indexed_scan(ctx, cols, pred, index_plan(pred->kind), ix, c, stream, "pcq_scan_dev_indexed_combined");
}

// GPS time in [start, end) through the time records; the boxes and the histograms are neither read nor changed.
extern "C" int pcq_scan_dev_indexed_time(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                                         pcq_collector *c, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !cols || !pred || !ix || !c) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_time: null argument");
    if (pred->kind != PCQ_PRED_TIME) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_time: predicate kind %d (PCQ_PRED_TIME only)", pred->kind);
    return indexed_scan(ctx, cols, pred, index_plan(pred->kind), ix, c, stream, "pcq_scan_dev_indexed_time");
}

// Box AND time through the boxes and the time records of the same index object.
extern "C" int pcq_scan_dev_indexed_bounds_time(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                                                pcq_collector *c, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !cols || !pred || !ix || !c) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_bounds_time: null argument");
    if (pred->kind != PCQ_PRED_BOUNDS_TIME)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_bounds_time: predicate kind %d (PCQ_PRED_BOUNDS_TIME only)", pred->kind);
    return indexed_scan(ctx, cols, pred, index_plan(pred->kind), ix, c, stream, "pcq_scan_dev_indexed_bounds_time");
}
