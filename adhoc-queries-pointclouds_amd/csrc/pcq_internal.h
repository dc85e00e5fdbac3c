// pcq_internal.h — shared declarations of libpcq.so (not part of the public ABI; see include/pcq.h).
#pragma once

#include <sched.h>
#include <atomic>
#include <thread>
#include "copy_pool.h"
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcq.h"
#include "stage_plan.h"  // the predicate-kind helpers (pred_has_box, ...), the collector kinds, what a scan reads
#include "index_plan.h"  // the chunk sizes of the index (INDEX_BOUNDS_CHUNK, ...), what an indexed scan of each kind prunes with

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
int pcq_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define PCQ_HIP(expr)                                                                           \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return pcq_fail(PCQ_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                            __FILE__, __LINE__);                                                \
    } while (0)

// Every entry point that takes a context or a collector runs on the context's device, whatever device the calling
// thread used before (a driver thread draining the collectors of several GPUs sits on device 0 by default: memory
// allocated and kernels launched from there would land on the wrong GPU).  The caller's device is restored on return.
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int device) {
        if (device < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) changed = hipSetDevice(device) == hipSuccess && prev >= 0;
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define PCQ_ON_DEVICE_OF_CTX(ctx) DeviceGuard _device_guard((ctx) ? (ctx)->device : -1)
#define PCQ_ON_DEVICE_OF_COLLECTOR(c) DeviceGuard _device_guard((c) && (c)->ctx ? (c)->ctx->device : -1)

// ---------------------------------------------------------------------------------------------
// device-side views
// ---------------------------------------------------------------------------------------------

// Predicate in device form.  The i64 box of the reference (last.rs:98-109) is clamped to the i32
// value range of the stored coordinates; `(uint32)(v - lo) <= width` is then exactly
// `lo <= v && v <= hi` on sign-extended values (last.rs:122-135).
struct DevPred {
    int32_t kind;      // pcq_predicate_kind
    int32_t empty;     // 1: no i32 coordinate can match (box entirely outside the i32 range)
    int32_t lo[3];
    uint32_t width[3];
    uint32_t cls;
    uint32_t _pad;
    double wmin[3], wmax[3];  // PCQ_PRED_BOUNDS_F64; PCQ_PRED_TIME, PCQ_PRED_BOUNDS_TIME: [wmin[0], wmax[0])
};

struct DevCols {
    const uint8_t *xyz;
    const uint8_t *cls;
    const uint8_t *rgb;
    uint64_t xyz_stride, cls_stride, rgb_stride;
    uint64_t n;
    uint64_t first_index;
    double scale[3];
    double offset[3];
};

// One segment of a batched count launch.
struct DevSegment {
    const int4 *xyz;       // 16-byte aligned positions block
    uint64_t n;            // points
    uint64_t tile_begin;   // first global wave-tile index of this segment
    int32_t lo[3];
    uint32_t width[3];
    int32_t empty;
    int32_t _pad;
};

// One segment of a batched class-count launch: a LAST classification block of any alignment.
struct DevClassSegment {
    const uint8_t *cls;
    uint64_t n;            // bytes (= points)
    uint64_t head;         // bytes in front of the first 16-byte aligned byte
    uint64_t nvec;         // 16-byte vectors in the aligned body
    uint64_t tile_begin;   // first global wave-tile (256 vectors = 4 KiB) of this segment
    uint32_t pat;          // class byte replicated x4
    uint32_t _pad;
};

// One segment of a batched box AND class count launch (scan_count_batch.hip): DevSegment with the class block beside it.
// Tables of these live in the same d_segments / h_segments buffers at their own pitch.
struct DevCombinedSegment {
    const int4 *xyz;       // 16-byte aligned positions block
    const uint8_t *cls;    // classification block of the same points, any alignment
    uint64_t n;            // points
    uint64_t tile_begin;   // first global step of this segment
    int32_t lo[3];
    uint32_t width[3];
    int32_t empty;
    uint32_t pat;          // class byte replicated x4
};

// One segment of a batched box AND time count launch (scan_count_batch.hip): DevCombinedSegment with the time block in
// place of the class block, and the range.  At its own pitch in the same buffers.
struct DevBoundsTimeSegment {
    const int4 *xyz;       // 16-byte aligned positions block
    const uint8_t *times;  // packed f64 GPS times of the same points, 8-byte aligned
    uint64_t n;            // points
    uint64_t tile_begin;   // first global step of this segment
    int32_t lo[3];
    uint32_t width[3];
    int32_t empty;
    uint32_t _pad;
    double t0, t1;         // [t0, t1)
};

// One segment of a multi-box batched count launch (scan_count_multi.hip): up to PCQ_MULTI_BOX_MAX boxes are asked of the
// segment while its tiles are in registers.  One pitch whatever the number of boxes of the launch; slots that are not live
// hold zeros.  Its tables travel under PCQ_SEGMENTS_MULTI, a kind of the segment table outside pcq_predicate_kind.
struct DevMultiSegment {
    const int4 *xyz;       // 16-byte aligned positions block
    uint64_t n;            // points
    uint64_t tile_begin;   // first global step of this segment
    uint32_t live;         // bit q: box q is asked of this segment and is not empty
    uint32_t _pad;
    int32_t lo[PCQ_MULTI_BOX_MAX][3];
    uint32_t width[PCQ_MULTI_BOX_MAX][3];
};
static_assert(PCQ_MULTI_BOX_MAX == 8 && sizeof(DevMultiSegment) == 224, "DevMultiSegment: eight boxes at one pitch");
constexpr int PCQ_SEGMENTS_MULTI = 0x4d42;  // ("MB") no pcq_predicate_kind: the key of a multi-box table equals no other table's

// The class histogram of a box (scan_class_hist.hip) reads tables of DevCombinedSegment (`pat` unused) under a kind of its own:
// the same bytes under PCQ_PRED_BOUNDS_CLASS are another batch entry's table.
constexpr int PCQ_SEGMENTS_CLASS_HIST = 0x4348;  // ("CH") no pcq_predicate_kind
// The time histogram of a box (scan_time_hist.hip) reads tables of DevBoundsTimeSegment (t0, t1 unused) with the launch's bin
// count and edges behind them, under a kind of its own: the same segments under PCQ_PRED_BOUNDS_TIME are another entry's table.
constexpr int PCQ_SEGMENTS_TIME_HIST = 0x5448;  // ("TH") no pcq_predicate_kind

// One segment of a density raster launch (scan_raster.hip) or a height, mean-height or height-spread raster launch (scan_zrange.hip, scan_zsum.hip, scan_zmoments.hip: the
// same table under the same kind, since the kernels read every field alike): DevSegment with the segment's cell widths in lattice units and the
// magics of the division by them (raster_div.h).  At its own pitch in the same buffers, under a kind of its own: the widths are
// part of the bytes the upload compares.
struct DevRasterSegment {
    const int4 *xyz;       // 16-byte aligned positions block
    uint64_t n;            // points
    uint64_t tile_begin;   // first global step of this segment
    int32_t lo[3];         // (lo[0], lo[1]: the raster's origin)
    uint32_t width[3];
    int32_t empty;
    int32_t _pad;
    uint32_t cw[2];        // cell widths along x and y
    uint32_t magic[2];     // raster_div_magic of them
};
static_assert(sizeof(DevRasterSegment) == 72, "DevRasterSegment: DevSegment and four words");
constexpr int PCQ_SEGMENTS_RASTER = 0x5253;  // ("RS") no pcq_predicate_kind

// One segment of a class-filtered mean-height raster launch (scan_zsum_classes.hip): DevRasterSegment with the class block of the
// same points beside it.  At its own pitch in the same buffers, under a kind of its own: the cached table of a raster launch is
// never taken for this entry's, nor this one's for theirs.  The class SET of a launch is no part of the table (it travels as
// kernel arguments), so two calls that differ in the set alone share one table.
struct DevRasterClassSegment : DevRasterSegment {  // (so raster_segment_fill of raster_cells.h fills it, with every refusal)
    const uint8_t *cls;    // classification block of the same points, any alignment
};
static_assert(sizeof(DevRasterClassSegment) == 80, "DevRasterClassSegment: DevRasterSegment and the class pointer");
constexpr int PCQ_SEGMENTS_RASTER_CLASSES = 0x5243;  // ("RC") no pcq_predicate_kind

// One segment of a box AND polygon count launch (scan_polygon.hip): DevSegment with the place of the segment's edges in the
// trailer behind the table.  An edge is a DevPolygonEdge: the outline's edge with its lower end first; horizontal edges, which never
// cross a point, do not travel.  At its own pitch in the same buffers, under a kind of its own; the edges are part of the bytes the
// upload compares.
struct DevPolygonSegment {
    const int4 *xyz;       // 16-byte aligned positions block
    uint64_t n;            // points
    uint64_t tile_begin;   // first global step of this segment
    int32_t lo[3];
    uint32_t width[3];
    int32_t empty;
    int32_t _pad;
    uint32_t edge_begin;   // first edge of the segment, counted in edges from the start of the trailer
    uint32_t nedges;       // its edges (0 .. PCQ_POLYGON_VERTS_MAX)
};
static_assert(sizeof(DevPolygonSegment) == 64, "DevPolygonSegment: DevSegment and two words; the trailer behind a table stays 16-byte aligned");
struct DevPolygonEdge {
    int32_t ax, ay;        // the end with the smaller y
    int32_t bx, by;        // the other end: by > ay
};
static_assert(sizeof(DevPolygonEdge) == 16, "DevPolygonEdge: one 16-byte scalar load");
constexpr int PCQ_SEGMENTS_POLYGON = 0x5047;  // ("PG") no pcq_predicate_kind

// SparseGrid parameters (grid_sampling.rs:9-47) in device form.
struct DevGrid {
    double bmin[3], bmax[3];
    double cell_size;
    double dims_f[3];     // dims as f64 (`self.dimensions.x as f64`, grid_sampling.rs:51)
    double inv_extent[3]; // 1 / (bmax - bmin): only to find the cell WITHOUT the division when that is provably safe (grid_common.h cell_of)
    double qk[3];         // RN(dims / (bmax - bmin)), and the range / boundary guard of the short cell computation (grid_common.h cell_fast)
    double qmax[3], guard[3];
    uint64_t mask[3];     // (1 << bits) - 1
    uint32_t shift[3];    // 0, bits_x, bits_x + bits_y  (already & 63)
    uint32_t keys_wide;   // 1: a key can have more than 32 bits (grid_common.h cell_hash)
};

// The chunk index (chunk_index.hip) as the buffer emit's count pass sees it: the state of the index chunk a tile of 2048
// points lies in.  Bounds and time chunks hold 4096 points (tiles 2c, 2c + 1), class chunks 65536 (tiles 32c .. 32c + 31); all
// start at point 0.  Tiles from `covered_tiles` on (the ragged tail) are always counted.
struct ChunkTime {  // GPS times of one 4096-point chunk: extremes over its non-NaN times (+inf / -inf when it has none)
    double mn, mx;
    uint32_t nans;  // times that are NaN
    uint32_t _pad;
};
struct EmitIndex {
    const int32_t *boxes;    // bounds: {mn[3], mx[3]} per chunk (integer AABB), or nullptr
    const uint32_t *hist;    // class: 256 bins per chunk, or nullptr   (box AND class: both)
    const ChunkTime *times;  // time: one record per chunk, or nullptr (alone; box AND time: with the boxes)
    uint64_t covered_tiles;
};
enum { CHUNK_SCAN = 0, CHUNK_NONE = 1, CHUNK_ALL = 2 };  // straddling: read it · disjoint: no match · contained: every point matches
// A chunk's integer AABB against the predicate's inclusive i64 box [lo, lo + width] (pred.empty: nothing matches).
__device__ __forceinline__ int index_box_state(const int32_t (&mn)[3], const int32_t (&mx)[3], const DevPred &pr) {
    bool disjoint = pr.empty != 0, inside = !pr.empty;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int64_t hi = (int64_t)pr.lo[a] + (int64_t)pr.width[a];
        disjoint |= (int64_t)mx[a] < (int64_t)pr.lo[a] || (int64_t)mn[a] > hi;
        inside &= (int64_t)mn[a] >= (int64_t)pr.lo[a] && (int64_t)mx[a] <= hi;
    }
    return disjoint ? CHUNK_NONE : (inside ? CHUNK_ALL : CHUNK_SCAN);
}
// A class chunk of `points` points whose histogram bin for the predicate's class is `bin`.
__device__ __forceinline__ int index_class_state(uint32_t bin, uint64_t points) {
    return bin == 0 ? CHUNK_NONE : ((uint64_t)bin == points ? CHUNK_ALL : CHUNK_SCAN);
}
// A time chunk against [t0, t1): Range<f64>::contains (pcq.h, PCQ_PRED_TIME) restated on the chunk's extremes, in IEEE f64
// compares only.  An empty range (t0 >= t1, or a NaN bound) and a chunk of NaNs match nothing; a chunk is contained only when
// none of its times is NaN.
__device__ __forceinline__ int index_time_state(const ChunkTime &ct, double t0, double t1) {
    if (!(t0 < t1) || ct.nans == (uint32_t)INDEX_BOUNDS_CHUNK || ct.mx < t0 || ct.mn >= t1) return CHUNK_NONE;
    return ct.nans == 0 && ct.mn >= t0 && ct.mx < t1 ? CHUNK_ALL : CHUNK_SCAN;
}
// Box AND class: a bounds chunk's box state with the state of the class chunk it lies in.  Nothing matches where either
// part has no match, every point matches only where both say so, and everything else is read.
__device__ __forceinline__ int index_combined_state(int box_state, int class_state) {
    if (box_state == CHUNK_NONE || class_state == CHUNK_NONE) return CHUNK_NONE;
    return box_state == CHUNK_ALL && class_state == CHUNK_ALL ? CHUNK_ALL : CHUNK_SCAN;
}

constexpr uint64_t PCQ_EMPTY_KEY = ~0ull;
constexpr uint64_t PCQ_NO_INDEX = ~0ull;

// ---------------------------------------------------------------------------------------------
// host-side objects
// ---------------------------------------------------------------------------------------------
struct GridState;
struct PoolBlock {
    void *p = nullptr;
    size_t bytes = 0;
    bool used = false;
};
// The staging ring of the host / file scans (host_stream.hip): two pinned host buffers with their device twins, the events
// that order their reuse, the copy helpers that fill them and the two warm-up threads.  Nothing else names its state; what
// the operations below keep true:
//   * a pair is present only when BOTH its pinned and its device buffer exist — an allocation that fails halfway frees the
//     half, so that the next call allocates again and reports the failure (pcq.h: pcq_prepare_host_scans);
//   * whatever frees, resizes or re-creates the pairs or the copy pool joins the prepare thread first, and whatever uses
//     the copy stream joins the copy-path warm-up first;
//   * pair b is "busy" from mark_busy(b) until its event has been waited for or the streams have been drained.
class StageRing {
public:
    int init(pcq_ctx *ctx);                  // (the events; pcq_init)
    void destroy();                          // joins, drains and frees everything (pcq_shutdown)
    int ensure(size_t bytes, int upto = 2);  // pairs 0 .. upto-1 present, each of at least `bytes`
    void drop();                             // no pairs (drained first), no copy pool: the next scan re-creates them (option "numa_local")
    void prepare();                          // pcq_prepare_host_scans: both pairs and the copy pool, on a thread of its own
    void join_prepare();                     // ... which reads chunk_points, copy_threads and numa_local: join it before they change
    bool copy_path_ready();                  // false: the process's first large copy has not been made — now under way on a thread
    void wait_copy_path();                   // in front of the caller's own use of the copy stream
    uint8_t *host(int b) const { return h_[b]; }
    uint8_t *dev(int b) const { return d_[b]; }
    int fetch(int fd, uint8_t *dst, const uint8_t *src, size_t bytes);  // caller memory or file -> pinned memory, over the copy helpers
    int copy_out(int b, void *d_dst, size_t bytes);  // pinned buffer b -> device memory on the copy stream; marks "copied"
    int wait_copied(int b, hipStream_t s);   // `s` waits for that copy
    int host_wait_copied(int b);             // the host does
    int wait_free(int b);                    // until the kernels that read pair b last are done with it
    int mark_busy(int b, hipStream_t s);     // pair b is read by what has been enqueued on s so far
    bool busy() const { return busy_[0] || busy_[1]; }
    void set_idle() { busy_[0] = busy_[1] = false; }  // (the caller has drained the compute stream)
    int drain();                             // both streams drained, no pair busy

private:
    int ensure_now(size_t bytes, int upto);
    void ensure_pool_now();
    void free_pairs();
    pcq_ctx *ctx_ = nullptr;
    uint8_t *h_[2] = {nullptr, nullptr}, *d_[2] = {nullptr, nullptr};
    size_t bytes_ = 0;                       // the size the pairs have, or will be allocated with
    bool busy_[2] = {false, false};          // kernels not yet known to be done with staging pair b (event consumed_[b])
    hipEvent_t copied_[2] = {nullptr, nullptr}, consumed_[2] = {nullptr, nullptr};
    CopyPool *pool_ = nullptr;               // created on first use by pcq_scan_host / pcq_scan_fd
    std::thread prepare_;                    // pcq_prepare_host_scans: joined by whoever touches the pairs or the copy pool next
    std::thread copy_warm_;                  // sets the copy path up: one pinned megabyte through hipMemcpyAsync, beside the first file's scan
    std::atomic<int> copy_warm_state_{0};    // 0 not started, 1 under way, 2 done
    void *copy_warm_h_ = nullptr, *copy_warm_d_ = nullptr;
};

struct pcq_ctx {
    int device = 0;
    hipStream_t stream = nullptr;       // compute stream
    hipStream_t copy_stream = nullptr;  // H2D stream
    hipStream_t scratch_stream = nullptr;  // the stream whose kernels may still be using the context's scratch (pcq_scratch_stream)
    int num_cus = 0;
    hipDeviceProp_t prop;
    // scratch: per-block partial counts / block offsets
    uint64_t *d_partials = nullptr;
    size_t partials_cap = 0;
    uint64_t *d_scalars = nullptr;      // a few device u64 scratch words
    uint64_t *h_scalars = nullptr;      // pinned mirror
    StageRing ring;                     // staging for pcq_scan_host / pcq_scan_fd (host_stream.hip)
    // segment table for batched launches
    DevSegment *d_segments = nullptr;
    DevSegment *h_segments = nullptr;
    size_t segments_cap = 0;            // BYTES of each of the two buffers (the tables of the batched kernels differ in pitch)
    size_t segments_uploaded = 0;       // number of segments of the table currently in d_segments (0 = none)
    int segments_kind = -1;             // predicate kind of the uploaded table
    // device-memory pool (pcq_pool_alloc / pcq_pool_free): the grid collector's tuple runs, partition buffers and
    // winner arrays are gigabytes per file, and a device allocation of that size costs from tens of milliseconds to
    // over a second (profiles/r01_grid_timeline.txt) — per-file grids (main.rs:156) reuse the blocks of the file before
    std::vector<PoolBlock> pool;
    uint64_t pool_limit = 96ull << 30;  // free bytes the pool may keep
    // diagnostics of the grid collector (pcq_get_option): folds run, folds that needed a second partition level,
    // folds repeated because a partition overflowed its LDS table, the last fold's second-level fan-out
    int64_t grid_folds = 0, grid_level2 = 0, grid_refolds = 0, grid_last_f2 = 0;
    int64_t grid_compactions = 0;       // folds whose bins were copied together first (short fragments)
    int64_t grid_level2_exact = 0;      // second levels repeated in the exact (counting) form: a sub-partition had outgrown its region
    int64_t grid_pending_budget = 0;    // option: tuples a grid collector may hold before it folds (0 = default)
    int allreduce_single_rank = 0;      // option: pcq_allreduce_sum_u64 with ONE rank still goes through RCCL (communicator of one
                                        // device, ncclAllReduce) — exercises the run-time binding on a single-GPU box
    int allreduce_fail = 0;             // option (tests): pcq_allreduce_sum_u64 fails — 1: before anything is touched, 2: after the reduction has run, 3: inside the group
    int grid_f2 = 0;                    // option (tests): second-level fan-out a fold starts from (0 = from the measured estimate)
    int grid_agg = 0;                   // option: pass 0 folds a tile's duplicate cells before they travel — 0 = while it pays (per workgroup),
                                        // 1 = every tile, 2 = never; the results are the same, the tuples moved are not
    int grid_stream = 1;                // option (tests): 0 = a coarse grid's bins are folded by k_fold<BIG> (the fallback of the streaming fold) only
    int64_t grid_deferred = 0;          // diagnostics: bins the streaming fold left to k_fold<BIG> (survivor list outgrown)
    int64_t grid_dense_deferred = 0;    // diagnostics: partitions k_fold_dense left to k_fold<SMALL> (more tuples than its chunk of 1536)
    int host_in_place = 2;              // option: count and grid scans of host / file data read the pinned staging ring IN PLACE (over PCIe) instead of
                                        // copying it to a device twin first: 0 never, 1 always, 2 while the process's copy path is being set up
                                        // (host_stream.hip scan_host_impl)
    int emit_park_max = 256;            // option: a tile with at most this many matches leaves them as 16-byte words for the emit (0 = never; <= 256)
    int emit_sparse_max = 64;           // option: a tile of 2048 points with at most this many matches is written by k_emit_sparse (0 = never)
    bool scanned_before = false;        // (PCQ_TIMING: the first host / file scan of a context prints where its time goes)
    int grid_block_pad = 0;             // option: 16-byte units between the end of a tile's block of tuples and the next block
    int grid_p0_blocks = 0;             // option (tests): > 0 = pass 0 runs on at most this many workgroups (never more than one per CU); 0 = one per CU
    int grid_tuple16 = 1;               // option (tests): 0 = every scan writes 24-byte tuples (the form a 16-byte tuple falls back to), 2 = 16-byte tuples without the second level's selector
    int64_t grid_last_tuples = 0;       // diagnostics: tuples the last fold found pending (after pass 0's own fold)
    int64_t grid_last_tuple_bytes = 0;  // diagnostics: bytes per tuple (16 or 24) of the last grid scan's run
    int64_t scratch_cap_words = 0;      // option (tests): > 0 = pcq_ensure_partials fails (PCQ_ERR_NOMEM) on a request above this many words
    int64_t emit_park_fallbacks = 0;    // diagnostics: buffer scans whose emit found no room for the parked matches (park_max dropped to 0)
    // options
    int grid_blocks_per_cu = 2;   // persistent blocks per CU of the generic (strided) count kernels and the chunk index
#ifdef PCQ_LAB                    // libpcq_lab.so only: the kernel shapes of csrc/lab/scan_count_lab.hip
    int k1_variant = 12;          // per-file K1: 12 = one wave per workgroup, two adjacent 3 KiB tiles per step, software-pipelined (= the product's)
    int k1_waves_per_cu = 3;
    int batch_blocks_per_cu = 3;
    int k1_grid = 0;              // absolute number of workgroups for the one-wave per-file kernels (0 = num_cus x k1_waves_per_cu)
    int batch_variant = 3;        // batched K1: 0 = 256-thread blocks · 1 / 2 = one wave per workgroup, 2 / 3 tiles per step · 3 = pipelined (= the product's)
    int batch_waves_per_cu = 3;
    int class_batch_loads = 4;
    int class_batch_waves_per_cu = 4;
    int class_batch_pipe = 1;
    int multi_waves_per_cu = 0;   // multi-box K1 (scan_count_multi.hip): workgroups per CU (0 = the product's: MULTI_WAVES_PER_CU)
    int class_hist_waves_per_cu = 0;  // class histogram (scan_class_hist.hip): workgroups per CU (0 = the product's: CLASS_HIST_WAVES_PER_CU)
    int time_hist_waves_per_cu = 0;  // time histogram (scan_time_hist.hip): workgroups per CU (0 = the product's: TIME_HIST_WAVES_PER_CU)
    int class_hist_copies = 0;    // ... and copies of the LDS histogram per wave, 1 / 2 / 4 / 8 / 16 (0 = the product's: CLASS_HIST_COPIES)
    int raster_waves_per_cu = 0;  // density raster (scan_raster.hip): workgroups per CU before the LDS limit (0 = the product's: RASTER_WAVES_PER_CU)
    int zrange_waves_per_cu = 0;  // height raster (scan_zrange.hip): workgroups per CU before the LDS limit (0 = the product's: ZRANGE_WAVES_PER_CU)
    int zsum_waves_per_cu = 0;    // mean-height raster (scan_zsum.hip): workgroups per CU before the LDS limit (0 = the product's: ZSUM_WAVES_PER_CU)
    int zsum_classes_waves_per_cu = 0;  // class-filtered mean-height raster (scan_zsum_classes.hip): the same (0 = the product's: ZSUM_CLASSES_WAVES_PER_CU)
    int zmoments_waves_per_cu = 0;  // height-spread raster (scan_zmoments.hip): the same (0 = the product's: ZMOMENTS_WAVES_PER_CU)
    int zrange_classes_waves_per_cu = 0;  // canopy-height raster (scan_zrange_classes.hip): the same (0 = the product's: ZRANGE_CLASSES_WAVES_PER_CU)
    int polygon_waves_per_cu = 0; // box AND polygon count (scan_polygon.hip): workgroups per CU (0 = the product's: POLYGON_WAVES_PER_CU)
    int raster_add = 0;           // ... and the form of its LDS add: 1 = per lane, 2 = the wave-level shortcut (0 = the product's: RASTER_WAVE_ADD)
#endif
    int numa_node = -1;               // NUMA node the GPU hangs off (sysfs), -1 if unknown
    cpu_set_t node_cpus;              // its CPUs (empty if unknown)
    int numa_local = 1;               // option "numa_local": staging buffers and copy helpers on that node
    int copy_threads = 16;        // threads filling a staging buffer (caller + helpers): 2-4 reach the PCIe rate from memory next to the
                                  // GPU, page-cache pages on the other socket need 8 (profiles/r01_cli_probe_timing.log); a stream of
                                  // files read with pread: 8 -> 5.5, 12 -> 5.0, 16 -> 4.9 ms per 240 MB (profiles/r04_cli_threads.log).
                                  // pcq_init caps it at the host's hardware threads per GPU.
    uint64_t chunk_points = 1ull << 20;    // 12 MB of positions per staging chunk: the steady rate of 24 MB (profiles/r01_host_path_rate.json: 1-8 Mi equal)
                                           // at half the pinning in front of a process's first file (profiles/r04_cli_chunks.log: 25 -> 20 ms)
};

// host_stream.hip: [offset, offset+bytes) of fd -> device memory through the pinned staging buffers
int pcq_stream_fd_to_device(pcq_ctx *ctx, int fd, uint64_t offset, uint64_t bytes, uint8_t *d_dst);

struct pcq_collector {
    int kind = COLL_COUNT;
    pcq_ctx *ctx = nullptr;
    // count
    uint64_t *d_count = nullptr;
    bool owns_count = false;
    // buffer: packed 31-byte points in HBM.  The number of points lives on the device (d_count): every scan reads it as
    // its base and moves it on, so scans need no round trip.  The host only knows an upper bound (one match per
    // scanned point) and asks the device for the truth when that bound outgrows the buffer.
    uint8_t *d_points = nullptr;
    uint64_t n_upper = 0, cap_points = 0;
    int count_slot = 0;                 // which of the two words of d_count holds the current count (a scan reads one, writes the other)
    // grid
    double bmin[3], bmax[3], cell_size = 0;
    uint64_t dims[3], bits[3];
    DevGrid grid;
    GridState *gs = nullptr;            // pending tuple runs + folded winners (grid_host.hip)
    uint64_t next_index = 0;            // file-order index the next scan starts at
    hipStream_t last_stream = nullptr;  // stream of the most recent scan: accessors wait on it
};

// ---------------------------------------------------------------------------------------------
// internal entry points (defined across the .hip files)
// ---------------------------------------------------------------------------------------------
int pcq_make_dev_pred(const pcq_predicate *p, DevPred *out);
int pcq_scratch_stream(pcq_ctx *ctx, hipStream_t s);
// collectors.hip: scans enqueued on a caller's stream may still be reading and moving the collector's state — waits for the
// stream of the collector's last scan unless that is `s` (whose order the caller's next operation keeps anyway)
int pcq_collector_wait_last(const pcq_collector *c, hipStream_t s);
int pcq_ensure_partials(pcq_ctx *ctx, size_t n);
// pcq_api.hip: d_segments / h_segments hold at least `bytes` each (a table that grows forgets the uploaded one)
int pcq_ensure_segment_table(pcq_ctx *ctx, size_t bytes);
// pcq_api.hip: the table (nsegments segments of `kind`, `bytes` long) is in d_segments once the work enqueued on s so far is
// done; uploaded only when it differs from the one already there
int pcq_upload_segment_table(pcq_ctx *ctx, int kind, size_t nsegments, const void *table, size_t bytes, hipStream_t s);

// scan_count.hip
int pcq_launch_bounds_count_xyz12(pcq_ctx *ctx, const void *d_xyz, uint64_t n, const DevPred &pred,
                                  uint64_t *d_count, hipStream_t s);
// K1 with a second column (PCQ_PRED_BOUNDS_CLASS: class bytes at any alignment; PCQ_PRED_BOUNDS_TIME: 8-byte aligned f64
// times), both for the same n points; positions 16-byte aligned (+= into *d_count)
int pcq_launch_bounds_count_xyz12_col(pcq_ctx *ctx, const void *d_xyz, const void *d_col, uint64_t n, const DevPred &pred, uint64_t *d_count,
                                      hipStream_t s);
int pcq_launch_class_count_u8(pcq_ctx *ctx, const void *d_cls, uint64_t n, uint8_t cls,
                              uint64_t *d_count, hipStream_t s);
// scan_count_multi.hip: the finish reduction of every count kernel, k_finish_counts on s — block q folds slice q (nblocks words) of
// the context's partials, += into d_counts[q]; nslices = 1 for the one-count kernels
int pcq_launch_finish_counts(pcq_ctx *ctx, int nslices, int nblocks, uint64_t *d_counts, hipStream_t s);
// scan_count_multi.hip: the finish of the height raster, k_finish_zrange on s — block c folds slice c (nblocks words: max z high, min z
// low) of the context's partials with a signed min / max into d_zmin[c] / d_zmax[c]
int pcq_launch_finish_zrange(pcq_ctx *ctx, int ncells, int nblocks, int32_t *d_zmin, int32_t *d_zmax, hipStream_t s);
// scan_count_multi.hip: the finish of the mean-height raster, k_finish_counts on s twice — slice c (nblocks words) of the context's
// partials += into d_count[c], slice ncells + c += into d_zsum[c], both modulo 2^64
int pcq_launch_finish_zsum(pcq_ctx *ctx, int ncells, int nblocks, uint64_t *d_count, int64_t *d_zsum, hipStream_t s);
// scan_count_multi.hip: the finish of the height-spread raster, k_finish_counts on s four times — slices a * ncells + c (a = 0 .. 3) of
// the context's partials += into d_count[c], d_zsum[c], d_zsq_lo[c], d_zsq_hi[c], all modulo 2^64
int pcq_launch_finish_zmoments(pcq_ctx *ctx, int ncells, int nblocks, uint64_t *d_count, int64_t *d_zsum, uint64_t *d_zsq_lo, uint64_t *d_zsq_hi,
                               hipStream_t s);
// scan_time.hip: K3 over a packed, 8-byte aligned f64 time column (+= into *d_count)
int pcq_launch_time_count_f64(pcq_ctx *ctx, const void *d_t, uint64_t n, const DevPred &pred, uint64_t *d_count, hipStream_t s);
// scan_generic.hip
int pcq_launch_generic_count(pcq_ctx *ctx, const DevCols &cols, const DevPred &pred,
                             uint64_t *d_count, hipStream_t s);
// ix (optional): the count pass takes each tile's state from the chunk index first (bounds, class, time, box AND class or box AND time predicates)
int pcq_launch_emit_points(pcq_ctx *ctx, const DevCols &cols, const DevPred &pred, uint8_t *d_out31, const uint64_t *d_npoints_in,
                           uint64_t *d_npoints_out, hipStream_t s, const EmitIndex *ix = nullptr);
// collectors.hip: pcq_scan_dev on stream s; ix (optional) is handed to the buffer collector's emit
int pcq_validate_scan(const pcq_columns *cols, const pcq_predicate *pred, const pcq_collector *c);
int pcq_scan_dev_impl(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c, hipStream_t s,
                      const EmitIndex *ix = nullptr);
// grid_host.hip (kernels: grid_pass0.hip, grid_dir.hip, grid_level2.hip, grid_fold.hip, grid_finish.hip; shared: grid_common.h)
int pcq_grid_scan(pcq_ctx *ctx, pcq_collector *c, const DevCols &cols, const DevPred &pred, hipStream_t s);
void pcq_grid_release(pcq_collector *c);
int pcq_grid_drain(pcq_collector *c, pcq_point *out, uint64_t *keys_out, uint64_t cap, uint64_t *out_n);
int pcq_grid_flush(pcq_collector *c);  // folds what is pending now
// alias_sort.hip: sorted[i] = the i-th of n records (u64 key at +0, u64 order at +8) by (key, order)
int pcq_sort_by_key_then_order(pcq_ctx *ctx, const void *items, size_t stride, uint64_t n, void *sorted, hipStream_t s);
// pcq_api.hip: device-memory pool of the context.  A block may be freed only when the work that used it has completed.
int pcq_pool_alloc(pcq_ctx *ctx, size_t bytes, void **out);
void pcq_pool_free(pcq_ctx *ctx, void *p);
void pcq_pool_clear(pcq_ctx *ctx);
