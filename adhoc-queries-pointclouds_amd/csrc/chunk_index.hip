// chunk_index.hip — on-the-fly chunk index for device-resident LAST columns.
//
// The reference's authors list this as their own next step (improvements.md:3-10): "while scanning
// first (without an index) we can create a chunk header for each chunk, but only for the queried
// attribute(s): if we query by bounds, we compute an AABB for each chunk; if we query by object class,
// a class histogram ... upon further scans, we first consult the index to find the matching chunks".
//
// Here the index is a side output of the count scans of a file that stays resident in HBM:
//   * bounds: the first bounds scan also writes the integer AABB of every 4096-point chunk (24 B per
//     48 KiB of positions).  Later bounds scans classify each chunk against the query box: disjoint ->
//     skipped, contained -> counted without reading a byte, straddling -> scanned with the same
//     mask-algebra tile kernel as K1 (scan_count.hip).
//   * class: the first class scan writes a 256-bin histogram per 65536-point chunk; later class
//     counts are sums of one bin per chunk and read no classification bytes at all.
//   * time (pcq_scan_dev_indexed_time): the first time scan writes the minimum and maximum of every 4096-point chunk's non-NaN
//     GPS times and the number of its NaNs (24 B per 32 KiB of times).  Later time scans classify each chunk against
//     [start, end) (index_time_state): a file in acquisition order is close to monotone in time, so all but a handful of chunks
//     are disjoint.
//   * box AND time (pcq_scan_dev_indexed_bounds_time): the boxes and the time records of the same 4096-point chunks, combined
//     as box AND class combines its parts; a file in acquisition order is coherent in space and in time at once.
//   * buffer collectors (the records of the matches): the index is built the same way (boxes or histograms alone), then the
//     emit of scan_generic.hip runs with its count pass taking each 2048-point tile's state from the index first
//     (k_tile_counts with IDX): disjoint tiles and contained tiles are not read there, disjoint ones not by the emit either.
//     The statistics of such a scan are classified from the index when they are asked for (k_index_emit_stats).
// Results are identical to the unindexed scans (tests/test_gpu_index.py, tests/test_gpu_index_points.py).  The index never takes part
// in bench.py: skipping work inside the timed region would invalidate the north-star measurement.
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
        if (n_skip) atomicAdd(&stats[0], (unsigned long long)n_skip);
        if (n_full) atomicAdd(&stats[1], (unsigned long long)n_full);
        if (n_scan) atomicAdd(&stats[2], (unsigned long long)n_scan);
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
        if (n_skip) atomicAdd(&stats[0], (unsigned long long)n_skip);
        if (n_full) atomicAdd(&stats[1], (unsigned long long)n_full);
        if (n_scan) atomicAdd(&stats[2], (unsigned long long)n_scan);
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

__device__ __forceinline__ double f64_of(int lo, int hi) {
    return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}
__device__ __forceinline__ bool in_range(double t, double t0, double t1) { return (t >= t0) & (t < t1); }  // (scan_time.hip)
__device__ __forceinline__ void load_time_chunk(v4i (&v)[TIME_LOADS], const v4i *__restrict__ base, uint64_t ch) {
    const v4i *p = base + ch * (CHUNK_POINTS / 2) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < TIME_LOADS; k++) v[k] = ld_nt(p + k * BLOCK);
}
__device__ __forceinline__ uint32_t count_time_chunk(const v4i (&v)[TIME_LOADS], double t0, double t1) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < TIME_LOADS; k++) c += (uint32_t)in_range(f64_of(v[k][0], v[k][1]), t0, t1) + (uint32_t)in_range(f64_of(v[k][2], v[k][3]), t0, t1);
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
                const double t = f64_of(v[k][2 * h], v[k][2 * h + 1]);
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

// Later time scans: classify each chunk (block-uniform), read only the straddling ones.  stats[0..2] += chunks skipped /
// counted whole / scanned.
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
    if (threadIdx.x == 0) {
        if (n_skip) atomicAdd(&stats[0], (unsigned long long)n_skip);
        if (n_full) atomicAdd(&stats[1], (unsigned long long)n_full);
        if (n_scan) atomicAdd(&stats[2], (unsigned long long)n_scan);
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
        if (n_skip) atomicAdd(&stats[0], (unsigned long long)n_skip);
        if (n_full) atomicAdd(&stats[1], (unsigned long long)n_full);
        if (n_scan) atomicAdd(&stats[2], (unsigned long long)n_scan);
    }
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

struct pcq_index {
    pcq_ctx *ctx = nullptr;
    // bounds part
    const void *xyz = nullptr;
    uint64_t n_xyz = 0, nchunks = 0;
    ChunkBox *d_boxes = nullptr;
    // class part
    const void *cls = nullptr;
    uint64_t n_cls = 0, ncchunks = 0;
    uint32_t *d_hist = nullptr;
    // time part
    const void *times = nullptr;
    uint64_t n_times = 0, ntchunks = 0;
    ChunkTime *d_times = nullptr;
    // statistics of the last indexed bounds scan
    unsigned long long *d_stats = nullptr;
    pcq_index_stats last = {};
    hipStream_t stats_stream = nullptr;  // non-null: `last` must be completed from d_stats (fetched lazily)
    int stats_kind = 0;                  // 0: the scan writes d_stats itself (a count) · 1 / 2 / 3 / 4 / 5: a bounds / class / box AND
    DevPred stats_pred = {};             //    class / time / box AND time buffer scan, classified from the index with stats_pred by pcq_index_get_stats (k_index_emit_stats)
};

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
    if (ix->d_boxes) (void)hipFree(ix->d_boxes);
    if (ix->d_hist) (void)hipFree(ix->d_hist);
    if (ix->d_times) (void)hipFree(ix->d_times);
    if (ix->d_stats) (void)hipFree(ix->d_stats);
    delete ix;
    return PCQ_OK;
}

extern "C" int pcq_index_get_stats(pcq_index *ix, pcq_index_stats *out) {
    if (!ix || !out) return pcq_fail(PCQ_ERR_ARG, "pcq_index_get_stats: null argument");
    PCQ_ON_DEVICE_OF_CTX(ix->ctx);
    if (ix->stats_stream) {  // the counters of the last indexed bounds scan are still on the device
        unsigned long long h[3] = {0, 0, 0};
        if (ix->stats_kind) {
            const bool time = ix->stats_kind == 4, box_time = ix->stats_kind == 5;
            const uint64_t nch = time ? ix->ntchunks : (ix->stats_kind == 2 ? ix->ncchunks : ix->nchunks);
            const int grid = (int)((nch + BLOCK - 1) / BLOCK < (uint64_t)ix->ctx->num_cus ? (nch + BLOCK - 1) / BLOCK : (uint64_t)ix->ctx->num_cus);
            PCQ_HIP(hipMemsetAsync(ix->d_stats, 0, 4 * sizeof(unsigned long long), ix->stats_stream));
            if (grid > 0)
                hipLaunchKernelGGL(k_index_emit_stats, dim3(grid), dim3(BLOCK), 0, ix->stats_stream,
                                   !time && ix->stats_kind != 2 ? ix->d_boxes : nullptr,
                                   !time && !box_time && ix->stats_kind != 1 ? ix->d_hist : nullptr, time || box_time ? ix->d_times : nullptr, nch, ix->n_cls, ix->stats_pred, ix->d_stats);
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

// What the index covers: packed, 16-byte aligned positions with at least one whole chunk; packed class bytes.
static bool bounds_index_covers(const pcq_columns *cols) {
    return cols->xyz_stride == 12 && ((uintptr_t)cols->xyz & 15) == 0 && cols->n >= CHUNK_POINTS;
}
static bool class_index_covers(const pcq_columns *cols) { return cols->cls && cols->cls_stride == 1 && cols->n > 0; }

// The boxes of the `chunks` whole chunks of cols->xyz, built on `s` unless the index holds them for these columns already
// (*had).  The build counts the matches of `build_with` into the context's partials on its way: the real predicate for a
// count scan (one launch builds and counts), one with empty = 1 for a buffer scan (the boxes alone: the emit counts).
static int ensure_boxes(pcq_ctx *ctx, pcq_index *ix, const pcq_columns *cols, uint64_t chunks, int grid, const DevPred &build_with,
                        hipStream_t s, bool *had) {
    *had = ix->d_boxes && ix->xyz == cols->xyz && ix->n_xyz == cols->n;
    if (*had) return PCQ_OK;
    if (ix->d_boxes) PCQ_HIP(hipFree(ix->d_boxes));
    ix->d_boxes = nullptr;
    PCQ_HIP(hipMalloc((void **)&ix->d_boxes, chunks * sizeof(ChunkBox)));
    hipLaunchKernelGGL(k_index_build_bounds, dim3(grid), dim3(BLOCK), 0, s, reinterpret_cast<const v4i *>(cols->xyz), chunks, build_with,
                       ix->d_boxes, ctx->d_partials);
    PCQ_HIP(hipGetLastError());
    ix->xyz = cols->xyz;
    ix->n_xyz = cols->n;
    ix->nchunks = chunks;
    return PCQ_OK;
}
// The same for the class histograms of cols->cls.
static int ensure_hist(pcq_index *ix, const pcq_columns *cols, uint64_t chunks, int grid, hipStream_t s, bool *had) {
    *had = ix->d_hist && ix->cls == cols->cls && ix->n_cls == cols->n;
    if (*had) return PCQ_OK;
    if (ix->d_hist) PCQ_HIP(hipFree(ix->d_hist));
    ix->d_hist = nullptr;
    PCQ_HIP(hipMalloc((void **)&ix->d_hist, chunks * 256 * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_index_build_class, dim3(grid), dim3(BLOCK), 0, s, (const uint8_t *)cols->cls, cols->n, chunks, ix->d_hist);
    PCQ_HIP(hipGetLastError());
    ix->cls = cols->cls;
    ix->n_cls = cols->n;
    ix->ncchunks = chunks;
    return PCQ_OK;
}

extern "C" int pcq_scan_dev_indexed(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                                    pcq_collector *c, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !cols || !pred || !ix || !c) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed: null argument");
    if (c->kind == COLL_GRID) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed: count and buffer collectors only");
    int rc = pcq_validate_scan(cols, pred, c);  // (before the index or the collector is touched: the kernels below trust the columns)
    if (rc) return rc;
    const bool bounds = pred->kind == PCQ_PRED_BOUNDS;
    // no index of the other kinds (nor of a world-space box): the plain scan, statistics that claim nothing
    if (!bounds && pred->kind != PCQ_PRED_CLASS) {
        ix->last = pcq_index_stats{};
        ix->stats_stream = nullptr;
        ix->stats_kind = 0;
        return pcq_scan_dev(ctx, cols, pred, c, stream);
    }
    if (!(bounds ? bounds_index_covers(cols) : class_index_covers(cols))) return pcq_scan_dev(ctx, cols, pred, c, stream);  // layout the index does not cover: plain scan
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    DevPred dp;
    rc = pcq_make_dev_pred(pred, &dp);
    if (rc) return rc;
    rc = pcq_scratch_stream(ctx, s);
    if (rc) return rc;
    const bool count = c->kind == COLL_COUNT;
    const uint64_t chunks = bounds ? cols->n / CHUNK_POINTS : (cols->n + CLASS_CHUNK - 1) / CLASS_CHUNK;
    const int max_blocks = ctx->num_cus * 8;
    const int grid = (int)(chunks < (uint64_t)max_blocks ? chunks : (uint64_t)max_blocks);
    bool had;
    if (bounds) {
        rc = pcq_ensure_partials(ctx, (size_t)grid);
        if (rc) return rc;
        DevPred build_with = dp;
        if (!count) build_with.empty = 1;
        rc = ensure_boxes(ctx, ix, cols, chunks, grid, build_with, s, &had);
    } else {
        rc = ensure_hist(ix, cols, chunks, grid, s, &had);
    }
    if (rc) return rc;
    ix->last = pcq_index_stats{};
    ix->last.chunks = chunks;
    ix->stats_stream = nullptr;
    ix->stats_kind = 0;
    if (!had) {  // the build read every chunk
        ix->last.built = 1;
        ix->last.scanned = chunks;
    }
    if (!count) {
        // A buffer collector: the emit's count pass takes each tile's state from the index (scan_generic.hip, k_tile_counts with
        // IDX), then the records are written as by pcq_scan_dev.
        if (had) {
            ix->stats_stream = s;  // classified and fetched by pcq_index_get_stats: nothing on the scan path
            ix->stats_kind = bounds ? 1 : 2;
            ix->stats_pred = dp;
        }
        EmitIndex eix = {};
        if (bounds) {
            eix.boxes = reinterpret_cast<const int32_t *>(ix->d_boxes);
            eix.covered_tiles = chunks * (CHUNK_POINTS / EMIT_TILE_POINTS);
        } else {
            eix.hist = ix->d_hist;
            eix.covered_tiles = cols->n / EMIT_TILE_POINTS;  // whole tiles
        }
        return pcq_scan_dev_impl(ctx, cols, pred, c, s, &eix);
    }
    c->last_stream = s;
    if (!bounds) {
        if (had) ix->last.whole = chunks;  // answered from the histograms: no classification byte is read
        hipLaunchKernelGGL(k_index_count_class, dim3(1), dim3(BLOCK), 0, s, ix->d_hist, chunks, (uint32_t)pred->cls, c->d_count);
        PCQ_HIP(hipGetLastError());
        return PCQ_OK;
    }
    if (had) {
        PCQ_HIP(hipMemsetAsync(ix->d_stats, 0, 4 * sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_index_count_bounds, dim3(grid), dim3(BLOCK), 0, s, reinterpret_cast<const v4i *>(cols->xyz), chunks, dp,
                           ix->d_boxes, ctx->d_partials, ix->d_stats);
        ix->stats_stream = s;  // fetched lazily by pcq_index_get_stats: no sync on the scan path
    }
    rc = pcq_launch_finish_counts(ctx, 1, grid, c->d_count, s);
    if (rc) return rc;
    const uint64_t rest_first = chunks * CHUNK_POINTS;
    if (rest_first < cols->n) {  // the ragged end (< one chunk) is always scanned
        pcq_columns tail = *cols;
        tail.xyz = (const uint8_t *)cols->xyz + 12 * rest_first;
        tail.cls = nullptr;
        tail.rgb = nullptr;
        tail.n = cols->n - rest_first;
        return pcq_scan_dev(ctx, &tail, pred, c, stream);
    }
    return PCQ_OK;
}

// Box AND class through both parts of the index.  Parts missing for these columns are built first (the boxes without a count:
// k_index_build_bounds knows boxes only), then the pruned pass always runs.
extern "C" int pcq_scan_dev_indexed_combined(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                                             pcq_collector *c, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !cols || !pred || !ix || !c) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_combined: null argument");
    if (pred->kind != PCQ_PRED_BOUNDS_CLASS)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_combined: predicate kind %d (PCQ_PRED_BOUNDS_CLASS only)", pred->kind);
    if (c->kind == COLL_GRID) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_combined: count and buffer collectors only");
    int rc = pcq_validate_scan(cols, pred, c);  // (before the index or the collector is touched: the kernels below trust the columns)
    if (rc) return rc;
    if (!(bounds_index_covers(cols) && class_index_covers(cols))) {  // layout the index does not cover: plain scan, statistics that claim nothing
        ix->last = pcq_index_stats{};
        ix->stats_stream = nullptr;
        ix->stats_kind = 0;
        return pcq_scan_dev(ctx, cols, pred, c, stream);
    }
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    DevPred dp;
    rc = pcq_make_dev_pred(pred, &dp);
    if (rc) return rc;
    rc = pcq_scratch_stream(ctx, s);
    if (rc) return rc;
    const uint64_t chunks = cols->n / CHUNK_POINTS, cchunks = (cols->n + CLASS_CHUNK - 1) / CLASS_CHUNK;
    const int max_blocks = ctx->num_cus * 8;
    const int grid = (int)(chunks < (uint64_t)max_blocks ? chunks : (uint64_t)max_blocks);
    const int cgrid = (int)(cchunks < (uint64_t)max_blocks ? cchunks : (uint64_t)max_blocks);
    rc = pcq_ensure_partials(ctx, (size_t)grid);
    if (rc) return rc;
    bool had_boxes, had_hist;
    DevPred boxes_only = dp;
    boxes_only.empty = 1;
    rc = ensure_boxes(ctx, ix, cols, chunks, grid, boxes_only, s, &had_boxes);
    if (!rc) rc = ensure_hist(ix, cols, cchunks, cgrid, s, &had_hist);
    if (rc) return rc;
    ix->last = pcq_index_stats{};
    ix->last.chunks = chunks;
    ix->last.built = !had_boxes || !had_hist;
    ix->stats_stream = s;  // completed by pcq_index_get_stats: no sync on the scan path
    if (c->kind != COLL_COUNT) {
        ix->stats_kind = 3;  // classified from the index when asked for
        ix->stats_pred = dp;
        EmitIndex eix = {};
        eix.boxes = reinterpret_cast<const int32_t *>(ix->d_boxes);
        eix.hist = ix->d_hist;
        eix.covered_tiles = chunks * (CHUNK_POINTS / EMIT_TILE_POINTS);
        return pcq_scan_dev_impl(ctx, cols, pred, c, s, &eix);
    }
    ix->stats_kind = 0;
    c->last_stream = s;
    PCQ_HIP(hipMemsetAsync(ix->d_stats, 0, 4 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_index_count_bounds_class, dim3(grid), dim3(BLOCK), 0, s, reinterpret_cast<const v4i *>(cols->xyz), (const uint8_t *)cols->cls,
                       cols->n, chunks, dp, ix->d_boxes, ix->d_hist, ctx->d_partials, ix->d_stats);
    rc = pcq_launch_finish_counts(ctx, 1, grid, c->d_count, s);
    if (rc) return rc;
    const uint64_t rest_first = chunks * CHUNK_POINTS;
    if (rest_first < cols->n) {  // the ragged end (< one chunk) is always scanned, with ITS class bytes
        pcq_columns tail = *cols;
        tail.xyz = (const uint8_t *)cols->xyz + 12 * rest_first;
        tail.cls = (const uint8_t *)cols->cls + rest_first;
        tail.cls_stride = 1;
        tail.rgb = nullptr;
        tail.n = cols->n - rest_first;
        return pcq_scan_dev(ctx, &tail, pred, c, stream);
    }
    return PCQ_OK;
}

// The time part: packed f64 times, 16-byte aligned (two times per load), with at least one whole chunk.
static bool time_index_covers(const pcq_columns *cols) {
    return cols->cls && cols->cls_stride == 8 && ((uintptr_t)cols->cls & 15) == 0 && cols->n >= CHUNK_POINTS;
}
// The records of the `chunks` whole chunks of the time column cols->cls, as ensure_boxes builds the boxes.
static int ensure_times(pcq_ctx *ctx, pcq_index *ix, const pcq_columns *cols, uint64_t chunks, int grid, const DevPred &build_with,
                        hipStream_t s, bool *had) {
    *had = ix->d_times && ix->times == cols->cls && ix->n_times == cols->n;
    if (*had) return PCQ_OK;
    if (ix->d_times) PCQ_HIP(hipFree(ix->d_times));
    ix->d_times = nullptr;
    PCQ_HIP(hipMalloc((void **)&ix->d_times, chunks * sizeof(ChunkTime)));
    hipLaunchKernelGGL(k_index_build_time, dim3(grid), dim3(BLOCK), 0, s, reinterpret_cast<const v4i *>(cols->cls), chunks, build_with,
                       ix->d_times, ctx->d_partials);
    PCQ_HIP(hipGetLastError());
    ix->times = cols->cls;
    ix->n_times = cols->n;
    ix->ntchunks = chunks;
    return PCQ_OK;
}

// GPS time in [start, end) through the time part of the index; the bounds and class parts are neither read nor changed.
extern "C" int pcq_scan_dev_indexed_time(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                                         pcq_collector *c, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !cols || !pred || !ix || !c) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_time: null argument");
    if (pred->kind != PCQ_PRED_TIME) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_time: predicate kind %d (PCQ_PRED_TIME only)", pred->kind);
    if (c->kind == COLL_GRID) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_time: count and buffer collectors only");
    int rc = pcq_validate_scan(cols, pred, c);  // (before the index or the collector is touched: the kernels below trust the columns)
    if (rc) return rc;
    if (!time_index_covers(cols)) {  // layout the index does not cover: plain scan, statistics that claim nothing
        ix->last = pcq_index_stats{};
        ix->stats_stream = nullptr;
        ix->stats_kind = 0;
        return pcq_scan_dev(ctx, cols, pred, c, stream);
    }
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    DevPred dp;
    rc = pcq_make_dev_pred(pred, &dp);
    if (rc) return rc;
    rc = pcq_scratch_stream(ctx, s);
    if (rc) return rc;
    const bool count = c->kind == COLL_COUNT;
    const uint64_t chunks = cols->n / CHUNK_POINTS;
    const int max_blocks = ctx->num_cus * 8;
    const int grid = (int)(chunks < (uint64_t)max_blocks ? chunks : (uint64_t)max_blocks);
    rc = pcq_ensure_partials(ctx, (size_t)grid);
    if (rc) return rc;
    DevPred build_with = dp;
    if (!count) build_with.empty = 1;  // the records alone: the emit counts
    bool had;
    rc = ensure_times(ctx, ix, cols, chunks, grid, build_with, s, &had);
    if (rc) return rc;
    ix->last = pcq_index_stats{};
    ix->last.chunks = chunks;
    ix->stats_stream = nullptr;
    ix->stats_kind = 0;
    if (!had) {  // the build read every chunk
        ix->last.built = 1;
        ix->last.scanned = chunks;
    }
    if (!count) {
        if (had) {
            ix->stats_stream = s;  // classified and fetched by pcq_index_get_stats: nothing on the scan path
            ix->stats_kind = 4;
            ix->stats_pred = dp;
        }
        EmitIndex eix = {};
        eix.times = ix->d_times;
        eix.covered_tiles = chunks * (CHUNK_POINTS / EMIT_TILE_POINTS);
        return pcq_scan_dev_impl(ctx, cols, pred, c, s, &eix);
    }
    c->last_stream = s;
    if (had) {
        PCQ_HIP(hipMemsetAsync(ix->d_stats, 0, 4 * sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_index_count_time, dim3(grid), dim3(BLOCK), 0, s, reinterpret_cast<const v4i *>(cols->cls), chunks, dp, ix->d_times,
                           ctx->d_partials, ix->d_stats);
        ix->stats_stream = s;  // fetched lazily by pcq_index_get_stats: no sync on the scan path
    }
    rc = pcq_launch_finish_counts(ctx, 1, grid, c->d_count, s);
    if (rc) return rc;
    const uint64_t rest_first = chunks * CHUNK_POINTS;
    if (rest_first < cols->n) {  // the ragged end (< one chunk) is always scanned, with ITS times (and positions, when present)
        pcq_columns tail = *cols;
        tail.cls = (const uint8_t *)cols->cls + 8 * rest_first;
        tail.xyz = cols->xyz ? (const uint8_t *)cols->xyz + 12 * rest_first : nullptr;
        tail.rgb = nullptr;
        tail.n = cols->n - rest_first;
        return pcq_scan_dev(ctx, &tail, pred, c, stream);
    }
    return PCQ_OK;
}

// Box AND time through the boxes and the time records of the same index object.  Parts missing for these columns are built first
// (without a count: each builder knows its own column only), then the pruned pass always runs.
extern "C" int pcq_scan_dev_indexed_bounds_time(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                                                pcq_collector *c, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !cols || !pred || !ix || !c) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_bounds_time: null argument");
    if (pred->kind != PCQ_PRED_BOUNDS_TIME)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_bounds_time: predicate kind %d (PCQ_PRED_BOUNDS_TIME only)", pred->kind);
    if (c->kind == COLL_GRID) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_indexed_bounds_time: count and buffer collectors only");
    int rc = pcq_validate_scan(cols, pred, c);  // (before the index or the collector is touched: the kernels below trust the columns)
    if (rc) return rc;
    DevPred dp;
    rc = pcq_make_dev_pred(pred, &dp);
    if (rc) return rc;
    // a layout the index does not cover, or a predicate that can match nothing (a box outside the i32 range, an empty or NaN
    // range): the plain scan, statistics that claim nothing
    if (!(bounds_index_covers(cols) && time_index_covers(cols)) || dp.empty || !(dp.wmin[0] < dp.wmax[0])) {
        ix->last = pcq_index_stats{};
        ix->stats_stream = nullptr;
        ix->stats_kind = 0;
        return pcq_scan_dev(ctx, cols, pred, c, stream);
    }
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    rc = pcq_scratch_stream(ctx, s);
    if (rc) return rc;
    const uint64_t chunks = cols->n / CHUNK_POINTS;  // of both parts
    const int max_blocks = ctx->num_cus * 8;
    const int grid = (int)(chunks < (uint64_t)max_blocks ? chunks : (uint64_t)max_blocks);
    rc = pcq_ensure_partials(ctx, (size_t)grid);
    if (rc) return rc;
    bool had_boxes, had_times;
    DevPred build_only = dp;
    build_only.empty = 1;
    rc = ensure_boxes(ctx, ix, cols, chunks, grid, build_only, s, &had_boxes);
    if (!rc) rc = ensure_times(ctx, ix, cols, chunks, grid, build_only, s, &had_times);
    if (rc) return rc;
    ix->last = pcq_index_stats{};
    ix->last.chunks = chunks;
    ix->last.built = !had_boxes || !had_times;
    ix->stats_stream = s;  // completed by pcq_index_get_stats: no sync on the scan path
    if (c->kind != COLL_COUNT) {
        ix->stats_kind = 5;  // classified from the index when asked for
        ix->stats_pred = dp;
        EmitIndex eix = {};
        eix.boxes = reinterpret_cast<const int32_t *>(ix->d_boxes);
        eix.times = ix->d_times;
        eix.covered_tiles = chunks * (CHUNK_POINTS / EMIT_TILE_POINTS);
        return pcq_scan_dev_impl(ctx, cols, pred, c, s, &eix);
    }
    ix->stats_kind = 0;
    c->last_stream = s;
    PCQ_HIP(hipMemsetAsync(ix->d_stats, 0, 4 * sizeof(unsigned long long), s));
    // (both builders wrote the partials; the pruned count writes every one of the `grid` again before they are summed)
    hipLaunchKernelGGL(k_index_count_bounds_time, dim3(grid), dim3(BLOCK), 0, s, reinterpret_cast<const v4i *>(cols->xyz), (const uint8_t *)cols->cls,
                       chunks, dp, ix->d_boxes, ix->d_times, ctx->d_partials, ix->d_stats);
    rc = pcq_launch_finish_counts(ctx, 1, grid, c->d_count, s);
    if (rc) return rc;
    const uint64_t rest_first = chunks * CHUNK_POINTS;
    if (rest_first < cols->n) {  // the ragged end (< one chunk) is always scanned, with ITS positions and ITS times
        pcq_columns tail = *cols;
        tail.xyz = (const uint8_t *)cols->xyz + 12 * rest_first;
        tail.cls = (const uint8_t *)cols->cls + 8 * rest_first;
        tail.rgb = nullptr;
        tail.n = cols->n - rest_first;
        return pcq_scan_dev(ctx, &tail, pred, c, stream);
    }
    return PCQ_OK;
}
