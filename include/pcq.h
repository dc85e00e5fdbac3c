/*
 * pcq.h — C ABI of the MI355X-native point-cloud predicate path ("libpcq.so").
 *
 * This is the drop-in boundary for the reference's `--optimized` predicate-evaluation hot path.
 * The reference (Rust) has no FFI for this path: the seam is the body of the four free functions
 *
 *     search_last_file_by_bounds_optimized           query/src/search/last.rs:46-166
 *     search_last_file_by_classification_optimized   query/src/search/last.rs:213-293
 *     search_las_file_by_bounds_optimized            query/src/search/las.rs:52-148
 *     search_las_file_by_classification_optimized    query/src/search/las.rs:192-261
 *
 * after they have mmapped the file and parsed the LAS header: a per-point loop that evaluates a
 * predicate over column data and pushes every match into a `&mut dyn ResultCollector`
 * (query/src/collect_points.rs:7-12).  The entry points below replace exactly that loop plus the
 * collector it feeds; file IO and header parsing stay on the host side of the boundary (in the
 * reference: readers/src + las crate; here: adhoc-queries-pointclouds_amd/host/).
 *
 * Plain pointers and sizes only.  `stream` arguments are hipStream_t passed as void*; NULL = the
 * context's own stream.  All functions return 0 (PCQ_OK) or a negative pcq_status; the message of
 * the last failure on the calling thread is available from pcq_last_error().
 * No function falls back to a CPU implementation: without a usable HIP device pcq_init fails.
 *
 * INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add to bind these.
 */
#ifndef PCQ_H
#define PCQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCQ_ABI_VERSION 6

typedef enum pcq_status {
    PCQ_OK = 0,
    PCQ_ERR_IO = -1,          /* reserved for the host layer: File::open / mmap     (last.rs:27-34)  */
    PCQ_ERR_HEADER = -2,      /* reserved for the host layer: LAS header parse      (last.rs:53-54)  */
    PCQ_ERR_FORMAT = -3,      /* reserved for the host layer: "Invalid LAS format"  (last.rs:72-78)  */
    PCQ_ERR_EXTENSION = -4,   /* reserved for the host layer: unsupported extension (searcher.rs:84) */
    PCQ_ERR_EOF = -5,         /* column block extends past the mapped file                           */
    PCQ_ERR_GRID = -6,        /* SparseGrid::new: too many cells                (grid_sampling.rs:32)*/
    PCQ_ERR_PANIC = -7,       /* AABB::from_min_max min > max                       (last.rs:98)     */
    PCQ_ERR_ARG = -8,         /* invalid argument                                                    */
    PCQ_ERR_HIP = -9,         /* a HIP runtime call failed / no device                               */
    PCQ_ERR_CAPACITY = -10,   /* caller buffer too small; required size reported through out param   */
    PCQ_ERR_UNSUPPORTED = -11,/* valid in the reference but not representable here   */
    PCQ_ERR_NOMEM = -12
} pcq_status;

/* readers/src/lib.rs:10-19 — `#[repr(C, packed)] struct Point`, 31 bytes. */
#pragma pack(push, 1)
typedef struct pcq_point {
    double x, y, z;             /* position        @0  */
    uint16_t r, g, b;           /* color           @24 */
    uint8_t classification;     /* classification  @30 */
} pcq_point;
#pragma pack(pop)

typedef struct pcq_ctx pcq_ctx;
typedef struct pcq_collector pcq_collector;

/* ---------------------------------------------------------------------------------------------
 * Context: one per (thread, GPU).  Owns a HIP stream, pinned staging buffers and device scratch.
 * Mirrors the reference's threading model: search_file is called concurrently from rayon workers
 * (main.rs:153-161) — each worker uses its own context; a context is not thread-safe.
 * ------------------------------------------------------------------------------------------- */
int pcq_init(int device, pcq_ctx **out_ctx);
int pcq_shutdown(pcq_ctx *ctx);
const char *pcq_last_error(void);
int pcq_abi_version(void);

typedef struct pcq_device_info {
    char name[128];
    char gcn_arch[64];
    int compute_units;
    int wavefront_size;
    uint64_t hbm_bytes;
    uint64_t lds_bytes_per_block;
    int clock_khz;
} pcq_device_info;
int pcq_get_device_info(pcq_ctx *ctx, pcq_device_info *out);
/* The context's stream (hipStream_t as void*). */
void *pcq_ctx_stream(pcq_ctx *ctx);
int pcq_ctx_synchronize(pcq_ctx *ctx);

/* ---------------------------------------------------------------------------------------------
 * Column view of one file's point data (or of a chunk of it).
 * LAST (readers/src/last_reader.rs:83-144): xyz_stride 12, cls_stride 1, rgb_stride 6.
 * LAS  (las.rs:102-135): all three strides = point_data_record_length, pointers offset into the
 * record (xyz +0, cls +15/+16, rgb +20/+28).
 * scale/offset are the header's (last.rs:156-160); `first_index` is the file-order index of the
 * first point of this view (used to keep "first seen wins" across chunks and files).
 * For PCQ_PRED_TIME, `cls` / `cls_stride` name the PREDICATE'S column instead: n little-endian f64 GPS times at any
 * byte alignment, stride >= 8 — LAST: the time block at offset_to_point_data + n*20 (formats 1, 3-5) or + n*22
 * (6-10), stride 8; LAS: the record + 20 / + 22, stride = record length.  A time record carries no class byte.  The time
 * column is always required; the positions only for buffer and grid collectors.  PCQ_PRED_BOUNDS_TIME passes the time
 * column the same way, next to the positions; PCQ_PRED_BOUNDS_CLASS passes class bytes as PCQ_PRED_CLASS does.
 * ------------------------------------------------------------------------------------------- */
typedef struct pcq_columns {
    const void *xyz;            /* n records of {i32 x, i32 y, i32 z}, little endian            */
    const void *cls;            /* n classification bytes; may be NULL for count-only bounds scan
                                   (PCQ_PRED_TIME: n f64 GPS times)                                */
    const void *rgb;            /* n records of {u16 r, u16 g, u16 b}; NULL = no colour (0,0,0)  */
    uint64_t xyz_stride;
    uint64_t cls_stride;
    uint64_t rgb_stride;
    uint64_t n;
    uint64_t first_index;
    double scale[3];
    double offset[3];
} pcq_columns;

typedef enum pcq_predicate_kind {
    PCQ_PRED_BOUNDS = 0,
    PCQ_PRED_CLASS = 1,
    PCQ_PRED_BOUNDS_F64 = 2,
    PCQ_PRED_TIME = 3,
    PCQ_PRED_BOUNDS_CLASS = 4,
    PCQ_PRED_BOUNDS_TIME = 5
} pcq_predicate_kind;

/* The predicate.
 * BOUNDS:     in the file's local integer space: lmin <= (x,y,z) <= lmax, inclusive, compared as i64
 *             (last.rs:122-135).  lmin/lmax are what pcq_box_to_local produced; values outside the i32
 *             range are legal.
 * CLASS:      classification byte == cls, whole byte (last.rs:259-262).
 * BOUNDS_F64: in world space, the reference's non-integer form used by the LAZER scan
 *             (query/src/search/lazer.rs:65-69 on positions rebuilt as offset + scale * x,
 *             readers/src/lazer_reader.rs:600-607): wmin <= world <= wmax per axis, inclusive
 *             (pasture AABB::contains).
 * TIME:       GPS time in [wmin[0], wmax[0]), half-open, IEEE compares on f64 (Range<f64>::contains of
 *             query/src/search/las.rs:297-358): a NaN time or bound matches nothing, wmin[0] >= wmax[0] is an empty
 *             range (no error), -0.0 == 0.0.  The other fields are ignored.  The time column is passed in
 *             pcq_columns.cls (see there); a match's record is the position with class 0 and colour (0,0,0)
 *             (`..Default::default()`, las.rs:345-355), so `rgb` is ignored.
 * BOUNDS_CLASS: the BOUNDS rule on lmin/lmax AND the CLASS rule on cls (not in the reference, whose CLI rejects the
 *             pair).  `xyz` and `cls` (class bytes, any stride >= 1) are both always read, even for a count; a match's
 *             record is the CLASS search's: position, the class byte of `cls`, colour from `rgb`.
 * BOUNDS_TIME: the BOUNDS rule on lmin/lmax AND the TIME rule on [wmin[0], wmax[0]).  `xyz` and `cls` (the f64 time
 *             column, stride >= 8, any alignment) are both always read; a match's record is the TIME search's:
 *             position, class 0, colour (0,0,0) — `rgb` is ignored.
 *             For both: an empty integer box (lmin > lmax on an axis, or outside the i32 range) matches nothing and
 *             launches no kernel. */
typedef struct pcq_predicate {
    int32_t kind;               /* pcq_predicate_kind */
    uint8_t cls;
    uint8_t _pad[3];
    int64_t lmin[3];
    int64_t lmax[3];
    double wmin[3];
    double wmax[3];
} pcq_predicate;

/* last.rs:98-109 / las.rs:88-99 — f64 query box -> local integer box, bug-for-bug (all three min
 * components divide by scale[0]; `as i64` truncation/saturation).  PCQ_ERR_PANIC if min > max. */
int pcq_box_to_local(const double bmin[3], const double bmax[3], const double scale[3],
                     const double offset[3], int64_t lmin[3], int64_t lmax[3]);

/* ---------------------------------------------------------------------------------------------
 * Collectors — device-resident counterparts of query/src/collect_points.rs.
 *   count  : CountCollector        (:72-98)   a u64 counter in HBM
 *   buffer : BufferCollector       (:14-44)   matches appended in file order (stable compaction)
 *   grid   : GridSampledCollector  (:100-127) SparseGrid (grid_sampling.rs:9-114): per cell the point closest to
 *            the cell centre, first seen wins ties.  No hash table in HBM: a scan leaves its matches as 16-byte tuples
 *            sorted by a hash bin of their cell, and a fold — when a result is asked for, or pcq_collector_flush —
 *            resolves every bin in an LDS table (csrc/grid_*.hip).
 * A collector may be fed by several scans (sequential mode feeds all files into one collector,
 * main.rs:129-133); scans into one collector must be issued in file order.
 * ------------------------------------------------------------------------------------------- */
int pcq_collector_new_count(pcq_ctx *ctx, pcq_collector **out);
/* Count collector whose counter lives in caller-owned device memory (8 bytes, zeroed by the
 * caller) — so that the caller can all-reduce it with RCCL (main.rs:164-180); pcq_allreduce_sum_u64 does that OUT OF
 * PLACE (the per-GPU counts stay what they were, whatever happens to the collective). */
int pcq_collector_new_count_at(pcq_ctx *ctx, uint64_t *device_counter, pcq_collector **out);
int pcq_collector_new_buffer(pcq_ctx *ctx, pcq_collector **out);
int pcq_collector_new_grid(pcq_ctx *ctx, const double bmin[3], const double bmax[3],
                           double cell_size, pcq_collector **out);
int pcq_collector_free(pcq_collector *c);
/* ResultCollector::point_count (synchronises the collector's stream). */
int pcq_collector_point_count(pcq_collector *c, uint64_t *out);
/* 1 when points()/points_ref() is Some (buffer, grid), 0 for the count collector. */
int pcq_collector_has_points(const pcq_collector *c);
/* ResultCollector::points: copies up to cap points to host memory, *out_n = number available
 * (PCQ_ERR_CAPACITY when cap is too small; call with out=NULL, cap=0 to size).
 * buffer: file order.  grid: hash-table slot order (the reference's HashMap order is unspecified);
 * pcq_collector_grid_cells returns the cell keys in the same order. */
int pcq_collector_points(pcq_collector *c, pcq_point *out, uint64_t cap, uint64_t *out_n);
int pcq_collector_grid_cells(pcq_collector *c, uint64_t *out, uint64_t cap, uint64_t *out_n);
/* SparseGrid::new results (grid_sampling.rs:24-44). */
int pcq_collector_grid_params(const pcq_collector *c, uint64_t dims[3], uint64_t bits[3]);
/* Resets the collector to its freshly constructed state (keeps allocations).  Waits for the collector's scans, and for
 * the zeroing of its counters: the next scan may be enqueued on any stream. */
int pcq_collector_reset(pcq_collector *c);
/* Brings a collector that is kept for later into its compact form NOW and waits for it: a grid collector folds its
 * pending matches into per-cell winners (the reference's HashMap never holds more than the winners,
 * grid_sampling.rs:72-103; the device keeps a tuple per scanned point until it folds) and returns their memory to the
 * context; count and buffer collectors only wait for their scans.  run_search_parallel calls it when a file is done
 * (main.rs:153-161 keeps one collector per file until all files are searched).  Results are unchanged. */
int pcq_collector_flush(pcq_collector *c);

/* ---------------------------------------------------------------------------------------------
 * The scan: evaluates `pred` over `cols` and pushes every match into `c`
 * (the loop at last.rs:117-164 / :253-291 / las.rs:101-146 / :221-259).
 *   pcq_scan_dev : column pointers are DEVICE memory; kernels are enqueued on `stream`
 *                  (asynchronous: results are complete after the stream is synchronised or a
 *                  collector accessor is called).
 *   pcq_scan_host: column pointers are HOST memory (e.g. the mmapped file); the library streams
 *                  them through pinned double buffers with hipMemcpyAsync overlapped with the
 *                  kernels, in chunks; returns when the scan is complete.
 * ------------------------------------------------------------------------------------------- */
int pcq_scan_dev(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c,
                 void *stream);
int pcq_scan_host(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred,
                  pcq_collector *c);
/* Same as pcq_scan_host, but the column "pointers" of `cols` are BYTE OFFSETS into the open file
 * `fd` (e.g. offset_to_point_data for xyz): chunks are pread() straight into the pinned staging
 * buffers, which avoids the page-table work of reading through a fresh mmap (last.rs:27-34). */
int pcq_scan_fd(pcq_ctx *ctx, int fd, const pcq_columns *cols, const pcq_predicate *pred,
                pcq_collector *c);
/* pcq_scan_host that returns as soon as the caller's memory has been read (copied into the staging buffers):
 * the caller may overwrite its columns at once and issue the next scan, whose staging copy then overlaps this
 * scan's transfer and kernels.  Results are complete after pcq_ctx_synchronize or any collector accessor. */
int pcq_scan_host_nowait(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c);
/* The same for pcq_scan_fd: returns when the file's last chunk has been read and its kernels are enqueued — the descriptor may
 * be closed at once, and the next file's first chunk is read while this one's last transfer and kernels run (a per-file
 * synchronisation drained the pipeline for about a chunk's read + transfer at every file boundary of main.rs:153-161). */
int pcq_scan_fd_nowait(pcq_ctx *ctx, int fd, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c);
/* Optional, for a caller that is going to scan from host memory or files: starts — on a thread of its own, and returns at
 * once — what the first such scan of a context otherwise does before it can move a byte: pinning the two staging buffers
 * (4 ms each) and starting the copy helpers.  Called right behind pcq_init this runs while the caller opens its first file
 * and creates its collector; the first scan (or pcq_shutdown) waits for whatever is left of it.  A failure here is not
 * reported here: the first scan repeats the allocation and reports it. */
int pcq_prepare_host_scans(pcq_ctx *ctx);

/* Count-only scan of many device-resident LAST files in ONE launch (files = independent units,
 * main.rs:153-161): segment i is scanned with preds[i] (all bounds, over 16-byte aligned positions
 * blocks — or all class, over classification blocks of any alignment); the total is ADDED to
 * *device_total.  PCQ_PRED_TIME, PCQ_PRED_BOUNDS_CLASS and PCQ_PRED_BOUNDS_TIME are refused (PCQ_ERR_ARG). */
int pcq_scan_dev_count_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds,
                             size_t nsegments, uint64_t *device_total, void *stream);
/* The same for box AND class: every predicate is PCQ_PRED_BOUNDS_CLASS, and segment i — packed positions (xyz_stride 12,
 * 16-byte aligned) beside the packed class bytes of the same points (cls_stride 1, any alignment, non-null when n > 0) — is
 * counted with the box and the class byte of preds[i]; the total is ADDED to *device_total.  nsegments == 0 is PCQ_OK.  Any
 * other predicate kind or layout is refused (PCQ_ERR_ARG) before anything is launched. */
int pcq_scan_dev_count_batch_combined(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds,
                                      size_t nsegments, uint64_t *device_total, void *stream);
/* The same for box AND time: every predicate is PCQ_PRED_BOUNDS_TIME, and segment i — packed positions (xyz_stride 12, 16-byte
 * aligned) beside the packed f64 GPS times of the same points in cols[i].cls (cls_stride 8, 8-byte aligned: 0 or 8 modulo 16,
 * non-null when n > 0) — is counted with the box and the range [wmin[0], wmax[0]) of preds[i] (an empty or NaN range matches
 * nothing); the total is ADDED to *device_total.  nsegments == 0 is PCQ_OK.  Any other predicate kind or layout is refused
 * (PCQ_ERR_ARG) before anything is launched or uploaded. */
int pcq_scan_dev_count_batch_bounds_time(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds,
                                         size_t nsegments, uint64_t *device_total, void *stream);
/* Many boxes in ONE pass: nqueries (1 .. PCQ_MULTI_BOX_MAX) boxes are asked of every segment while its positions are in
 * registers, so the data is read once instead of nqueries times.  preds is row-major [nsegments][nqueries], every entry
 * PCQ_PRED_BOUNDS; the count of segment i under preds[i * nqueries + q] is ADDED to device_totals[q] (nqueries device words).
 * A predicate that is empty (lmin > lmax on an axis, or a box outside the i32 value range) says "box q is not asked of
 * segment i": it contributes 0 and costs no evaluation.  The layout is that of pcq_scan_dev_count_batch: xyz_stride 12,
 * 16-byte aligned, non-null when n > 0.  nqueries == 1 is pcq_scan_dev_count_batch.  nsegments == 0 is PCQ_OK.  nqueries == 0
 * or above PCQ_MULTI_BOX_MAX, any other predicate kind and any other layout are refused (PCQ_ERR_ARG) before anything is
 * uploaded or launched. */
#define PCQ_MULTI_BOX_MAX 8
int pcq_scan_dev_count_batch_multi(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments,
                                   size_t nqueries, uint64_t *device_totals, void *stream);
/* The class histogram of a box in ONE pass: "what is in this box, by class?".  Every predicate is PCQ_PRED_BOUNDS, and segment
 * i has the layout of pcq_scan_dev_count_batch_combined — packed positions (xyz_stride 12, 16-byte aligned) beside the packed
 * class bytes of the same points (cls_stride 1, any alignment), both non-null when n > 0.  For every point of segment i inside
 * the box of preds[i], device_hist[its class byte] is incremented: the counts are ADDED to PCQ_CLASS_BINS device words, so
 * that device_hist[c] grows by what pcq_scan_dev_count_batch_combined counts for class c on the same segments and boxes, for
 * every c at once and from one read of the data.  A predicate that is empty (lmin > lmax on an axis, or a box outside the i32
 * value range) matches nothing and its segment is not evaluated.  nsegments == 0 is PCQ_OK.  A null argument, any other
 * predicate kind (PCQ_PRED_BOUNDS_CLASS included) and any other layout are refused (PCQ_ERR_ARG) before anything is uploaded
 * or launched: device_hist is untouched. */
#define PCQ_CLASS_BINS 256
int pcq_scan_dev_class_hist_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments,
                                  uint64_t *device_hist, void *stream);
/* The time histogram of a box in ONE pass: "when was this box scanned?".  Every predicate is PCQ_PRED_BOUNDS, and segment i has
 * the layout of pcq_scan_dev_count_batch_bounds_time — packed positions (xyz_stride 12, 16-byte aligned) beside the packed f64
 * GPS times of the same points in cols[i].cls (cls_stride 8, 8-byte aligned), both non-null when n > 0.  `edges` is a HOST
 * pointer to nbins + 1 doubles e[0] <= e[1] <= ... <= e[nbins]: non-decreasing, none NaN; infinities, -0.0 and equal neighbours
 * are allowed.  Bin b is the half-open range [e[b], e[b+1]) under IEEE compares, the range test of PCQ_PRED_BOUNDS_TIME.  A
 * point of segment i inside the box of preds[i] with time t adds 1 to bin b = #{i : e[i] <= t} - 1 when 0 <= b < nbins and to
 * nothing otherwise, so that device_hist[b] grows by what pcq_scan_dev_count_batch_bounds_time counts for [e[b], e[b+1]) on the
 * same segments and boxes, for every b at once and from one read of the data: a NaN time lands in no bin, a time equal to an
 * edge belongs to the bin that starts there, a bin with equal edges stays empty, -0.0 and 0.0 are one value, and +inf is in no
 * bin.  Only compares decide a bin, no arithmetic.  The counts are ADDED to device_hist[0 .. nbins); no word beyond is touched.
 * A predicate that is empty matches nothing and its segment is not evaluated.  nsegments == 0 is PCQ_OK after the argument
 * checks.  A null argument, nbins == 0 or above PCQ_TIME_BINS_MAX, a NaN edge, e[i] > e[i+1], any other predicate kind
 * (PCQ_PRED_BOUNDS_TIME included) and any other layout are refused (PCQ_ERR_ARG) before anything is uploaded or launched:
 * device_hist is untouched. */
#define PCQ_TIME_BINS_MAX 1024
int pcq_scan_dev_time_hist_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments,
                                 const double *edges, size_t nbins, uint64_t *device_hist, void *stream);
/* The density raster of a box in ONE pass: "where in this box are the points?".  Every predicate is PCQ_PRED_BOUNDS and the layout
 * is that of pcq_scan_dev_count_batch: xyz_stride 12, 16-byte aligned, non-null when n > 0; cls is not read.  `cell_xy` is a HOST
 * pointer to [nsegments][2] cell widths in the segment's lattice units (x, y), 1 .. 2^32 - 1.  All in the segment's integer
 * lattice: a point (X, Y, Z) of segment i inside the box of preds[i] adds 1 to device_raster[cy * nx + cx] with cx = (X - lmin[0])
 * / cell_xy[2i] and cy = (Y - lmin[1]) / cell_xy[2i + 1], exact integer floor divisions, so that word (cx, cy) grows by what
 * pcq_scan_dev_count_batch counts for the box intersected with that cell's integer sub-box, for every cell at once and from one
 * read of the data.  Only integer arithmetic decides a cell.  The counts are ADDED to device_raster[0 .. nx * ny), row-major with
 * y the slow axis; no word beyond is touched.  A predicate that is empty (lmin > lmax on an axis, or a box outside the i32 value
 * range) matches nothing and its segment is not evaluated.  nsegments == 0 is PCQ_OK after the argument checks.  A null argument,
 * nx == 0, ny == 0 or nx * ny above PCQ_RASTER_CELLS_MAX, any other predicate kind, any other layout, a cell width of 0 in a
 * segment with points, a non-empty predicate whose lmin[0] or lmin[1] lies outside the i32 range, and a non-empty predicate whose
 * box reaches beyond the raster — (min(lmax[a], INT32_MAX) - lmin[a]) / cell >= n for a = 0 or 1 — are refused (PCQ_ERR_ARG)
 * before anything is uploaded or launched: device_raster is untouched.  lmax and lmin[2] may be anywhere. */
#define PCQ_RASTER_CELLS_MAX 8192
int pcq_scan_dev_raster_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                              size_t nsegments, uint32_t nx, uint32_t ny, uint64_t *device_raster, void *stream);
/* The height raster of a box in ONE pass: "how high is this box, cell by cell?".  Layout, predicate kind, `cell_xy`, the cell rule
 * and the refusals are those of pcq_scan_dev_raster_batch, word for word; only the limit on nx * ny differs: PCQ_ZRANGE_CELLS_MAX.
 * A point (X, Y, Z) of segment i inside the box of preds[i] lies in cell c = cy * nx + cx with cx = (X - lmin[0]) / cell_xy[2i] and
 * cy = (Y - lmin[1]) / cell_xy[2i + 1], exact integer floor divisions.  The call is a FOLD, the counterpart of "the counts are
 * ADDED": after it device_zmin[c] = min(device_zmin[c] before, the Z of every such point) and device_zmax[c] = max(device_zmax[c]
 * before, the Z of every such point), signed compares of i32 words, for every cell at once and from one read of the data.  The
 * caller presets the words: INT32_MAX in device_zmin and INT32_MIN in device_zmax say "nothing yet", and a cell no point reaches
 * keeps both words.  Z is in the segment's OWN integer lattice: the values of segments whose z scale or z offset differ are NOT
 * comparable, so a caller batches segments of one z lattice per call (pcq_query_resident_bounds_zrange_raster does).  No word at
 * or beyond nx * ny of either array is touched.  A predicate that is empty matches nothing and its segment is not evaluated; a
 * point that fails only the z test of its box contributes nothing.  nsegments == 0 is PCQ_OK after the argument checks.  A null
 * argument (device_zmin and device_zmax among them), nx == 0, ny == 0 or nx * ny above PCQ_ZRANGE_CELLS_MAX, any other predicate
 * kind, any other layout, a cell width of 0 in a segment with points, a non-empty predicate whose lmin[0] or lmin[1] lies outside
 * the i32 range, and a non-empty predicate whose box reaches beyond the raster — (min(lmax[a], INT32_MAX) - lmin[a]) / cell >= n for
 * a = 0 or 1 — are refused (PCQ_ERR_ARG) before anything is uploaded or launched: both arrays are untouched.  lmax and lmin[2] may
 * be anywhere. */
#define PCQ_ZRANGE_CELLS_MAX 4096
int pcq_scan_dev_zrange_raster_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                                     size_t nsegments, uint32_t nx, uint32_t ny, int32_t *device_zmin, int32_t *device_zmax, void *stream);
/* The mean-height raster of a box in ONE pass: "how high is this box on average, cell by cell?" — the count and the z sum a mean
 * rests on.  Layout, predicate kind, `cell_xy`, the cell rule and the refusals are those of pcq_scan_dev_raster_batch, word for
 * word; only the limit on nx * ny differs: PCQ_ZSUM_CELLS_MAX.  A point (X, Y, Z) of segment i inside the box of preds[i] lies in
 * cell c = cy * nx + cx with cx = (X - lmin[0]) / cell_xy[2i] and cy = (Y - lmin[1]) / cell_xy[2i + 1], exact integer floor
 * divisions.  The call ADDS: for every such point device_count[c] += 1 and device_zsum[c] += (int64_t)Z, Z the stored i32
 * sign-extended, for every cell at once and from one read of the data.  Both are 64-bit adds MODULO 2^64 (two's complement for the
 * sum): what the words hold afterwards is the sum of what they held and of every contribution, reduced modulo 2^64, in whatever
 * order the adds happen.  The sums are exact outright while the true values fit i64, which fewer than 2^32 points into zeroed
 * words guarantees (|Z| <= 2^31, so |sum| < 2^63).  device_count after a call from zeroed words is exactly what
 * pcq_scan_dev_raster_batch gives.  Z is in the segment's OWN integer lattice: the sums of segments whose z scale or z offset
 * differ do not add up, so a caller batches segments of one z lattice per call (pcq_query_resident_bounds_zmean_raster does).  No
 * word at or beyond nx * ny of either array is touched.  A predicate that is empty matches nothing and its segment is not
 * evaluated; a point that fails only the z test of its box contributes nothing.  nsegments == 0 is PCQ_OK after the argument
 * checks.  A null argument (device_count and device_zsum among them), nx == 0, ny == 0 or nx * ny above PCQ_ZSUM_CELLS_MAX, any
 * other predicate kind, any other layout, a cell width of 0 in a segment with points, a non-empty predicate whose lmin[0] or
 * lmin[1] lies outside the i32 range, and a non-empty predicate whose box reaches beyond the raster — (min(lmax[a], INT32_MAX) -
 * lmin[a]) / cell >= n for a = 0 or 1 — are refused (PCQ_ERR_ARG) before anything is uploaded or launched: both arrays are
 * untouched.  lmax and lmin[2] may be anywhere. */
#define PCQ_ZSUM_CELLS_MAX 2048
int pcq_scan_dev_zsum_raster_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                                   size_t nsegments, uint32_t nx, uint32_t ny, uint64_t *device_count, int64_t *device_zsum, void *stream);
/* The mean-height raster of the points of a SET of classes in ONE pass: "how high is the ground of this box, cell by cell?".
 * pcq_scan_dev_zsum_raster_batch restricted to the points whose class byte is in the set: the same cells, the same two adds modulo
 * 2^64 for every point inside the box of its segment AND of a class in the set, at most PCQ_ZSUM_CELLS_MAX cells, PCQ_PRED_BOUNDS
 * predicates only, every refusal of that entry.  `class_set` is a HOST pointer to eight words: class c is in the set when bit
 * (c & 31) of class_set[c >> 5] is set: the whole class byte, as the LAST class search compares it.  Segments are laid out as for
 * pcq_scan_dev_count_batch_combined: beside the positions, cols[i].cls is the classification block of the same points (cls_stride
 * 1, any alignment).  device_count after a call from zeroed words is the class-filtered density raster; with all 256 bits set both
 * arrays receive exactly what pcq_scan_dev_zsum_raster_batch adds.  Refused besides (PCQ_ERR_ARG, both arrays untouched): a null
 * class_set, a segment with points whose cls is null, a segment with points whose cls_stride is not 1.  An empty set (eight zero
 * words) is PCQ_OK after every check: nothing is uploaded or launched and the words stay as they were. */
int pcq_scan_dev_zsum_raster_batch_classes(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                                           size_t nsegments, uint32_t nx, uint32_t ny, const uint32_t class_set[8],
                                           uint64_t *device_count, int64_t *device_zsum, void *stream);
/* The height-spread raster of a box in ONE pass: "how rough is this box, cell by cell?" — the count, the z sum and the sum of z
 * squared that a mean and a standard deviation rest on.  The cells, the boxes, `cell_xy`, the refusals and their order are those of
 * pcq_scan_dev_zsum_raster_batch, word for word; only the limit on nx * ny differs: PCQ_ZMOMENTS_CELLS_MAX.  The call ADDS, every
 * add a 64-bit add MODULO 2^64: for every point (X, Y, Z) of segment i inside the box of preds[i], in cell c,
 *
 *     device_count[c]  += 1;
 *     device_zsum[c]   += Z;                        (the stored i32 sign-extended, two's complement)
 *     device_zsq_lo[c] += (Z * Z) & 0xffffffff;     (Z * Z formed in 64 bits: at most 2^62, Z = INT32_MIN)
 *     device_zsq_hi[c] += (Z * Z) >> 32;
 *
 * device_count and device_zsum receive exactly what pcq_scan_dev_zsum_raster_batch adds.  The square is split so that no word needs
 * more than 64 bits: while a call reads fewer than 2^32 points into words that were 0, neither half can wrap and the sum of Z * Z
 * over the cell is device_zsq_hi[c] * 2^32 + device_zsq_lo[c] exactly (below 2^94); no carry is moved from the low word into the
 * high one.  Z is in the segment's OWN integer lattice, as there: a caller batches segments of one z lattice per call
 * (pcq_query_resident_bounds_zstd_raster does).  No word at or beyond nx * ny of any of the four arrays is touched.  nsegments == 0
 * is PCQ_OK after the argument checks, with nothing written.  A null argument (any of the four arrays among them: "null argument"),
 * nx == 0, ny == 0 or nx * ny above PCQ_ZMOMENTS_CELLS_MAX, and every refusal of pcq_scan_dev_zsum_raster_batch are PCQ_ERR_ARG
 * before anything is uploaded or launched: the four arrays are untouched. */
#define PCQ_ZMOMENTS_CELLS_MAX 1024
int pcq_scan_dev_zmoments_raster_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                                       size_t nsegments, uint32_t nx, uint32_t ny, uint64_t *device_count, int64_t *device_zsum,
                                       uint64_t *device_zsq_lo, uint64_t *device_zsq_hi, void *stream);
/* The canopy-height raster of a box in ONE pass: "how high above the ground is this box, cell by cell?" — the lowest z of the
 * points of a LOW set of classes and the highest z of the points of a HIGH set, per cell, from one read of positions and class
 * bytes.  Layout, predicate kind, `cell_xy`, the cell rule and every refusal are those of pcq_scan_dev_zsum_raster_batch_classes:
 * PCQ_PRED_BOUNDS only, cols[i].cls the classification block of the same points (cls_stride 1, not null, any byte alignment), and a
 * null set is a null argument; the limit on nx * ny is PCQ_ZRANGE_CLASSES_CELLS_MAX.  `low_set` and `high_set` are HOST pointers to
 * eight words each: class c is in a set when bit (c & 31) of its word c >> 5 is set.  The call is a FOLD, as
 * pcq_scan_dev_zrange_raster_batch is.  After it, for every cell c,
 *
 *     device_zmin[c] = min(before, Z of every point inside the box of its segment whose class byte is in low_set);
 *     device_zmax[c] = max(before, Z of every point inside the box of its segment whose class byte is in high_set);
 *
 * signed i32 compares; a point in both sets counts for both, a point in neither for nothing, and a point that fails only the z
 * test of its box contributes nothing.  A caller presets INT32_MAX / INT32_MIN and reads those values back as "no such point".  Z is
 * in the segment's OWN integer lattice: a caller batches segments of one z lattice per call.  No word at or beyond nx * ny of either
 * array is touched.  On any refusal (PCQ_ERR_ARG) both arrays are untouched.  Consequences:
 *   (a) both sets with all 256 bits give, word for word, what pcq_scan_dev_zrange_raster_batch gives from the same presets;
 *   (b) with low_set == high_set == S, on words preset to INT32_MAX / INT32_MIN and data without a stored Z of INT32_MAX,
 *       device_zmin[c] != INT32_MAX exactly where pcq_scan_dev_zsum_raster_batch_classes counts a point of S in c; the same holds
 *       for INT32_MIN, device_zmax and its sentinel;
 *   (c) an empty low set leaves device_zmin as it was while device_zmax is still folded, and the reverse;
 *   (d) with BOTH sets empty every check of the table is made, then nothing is uploaded or launched: PCQ_OK, the words as they were.
 * The segment table travels under the kind of pcq_scan_dev_zsum_raster_batch_classes (the sets are kernel arguments, never part
 * of it), so a table uploaded by either entry serves the other. */
#define PCQ_ZRANGE_CLASSES_CELLS_MAX 4096 /* 256 + 32 KiB of LDS per wave: four workgroups per CU at the limit */
int pcq_scan_dev_zrange_raster_batch_classes(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                                             size_t nsegments, uint32_t nx, uint32_t ny, const uint32_t low_set[8],
                                             const uint32_t high_set[8], int32_t *device_zmin, int32_t *device_zmax, void *stream);
/* Box AND polygon in ONE pass: "how many points of this box lie inside this outline?".  Every predicate is PCQ_PRED_BOUNDS and the
 * layout is that of pcq_scan_dev_count_batch_multi: xyz_stride 12, 16-byte aligned, non-null when n > 0; cls is not read.
 * `verts_xy` is a HOST pointer to [nsegments][nverts][2] i32, in each segment's own lattice.  The rule, all in a segment's integer
 * lattice:
 *
 * A polygon is `m` vertices `V_0 .. V_{m-1}` with `3 <= m <= PCQ_POLYGON_VERTS_MAX`. Each vertex is a pair of i32. The edges are
 * `(V_i, V_{(i+1) mod m})`.
 *
 * For a stored point `(X, Y, Z)` and an edge `A -> B`, let
 *
 *     d = (B.x - A.x) * (Y - A.y) - (X - A.x) * (B.y - A.y)        (exact, in integers)
 *
 * The edge *crosses* the point iff `(A.y <= Y < B.y and d > 0)` or `(B.y <= Y < A.y and d < 0)`. A horizontal edge never crosses.
 *
 * The point is inside iff an odd number of edges cross it (even-odd rule). This means:
 *
 * - Orientation does not matter.
 * - Self-intersecting outlines are legal.
 * - There is no validity check beyond `m`.
 *
 * A point is **counted** iff it passes the `PCQ_PRED_BOUNDS` rule of its segment's predicate (x, y and z, as everywhere) AND is
 * inside the polygon.
 *
 * So a rectangle (x0,y0),(x1,y0),(x1,y1),(x0,y1) contains exactly x0 <= X < x1, y0 <= Y < y1, half-open like the raster's cells,
 * and two polygons that share an edge never both claim or both drop a point on it.  Exactness bound: for a non-empty predicate,
 * take the hull of the box's x range clamped to i32 and the vertices' x range, and likewise on y; each hull must span at most
 * 2^31 - 1.  Then every difference fits 32 signed bits, every product is below 2^62 and d fits an i64.  The count is ADDED to
 * *device_total.  A predicate that is empty (lmin > lmax on an axis, or a box outside the i32 value range) matches nothing, its
 * segment is not evaluated and its vertices are not examined.  nsegments == 0 is PCQ_OK after the argument checks.  A null argument,
 * nverts < 3 or above PCQ_POLYGON_VERTS_MAX, any other predicate kind, any other layout and a non-empty predicate that breaks the
 * exactness bound are refused (PCQ_ERR_ARG) before anything is uploaded or launched: device_total is untouched. */
#define PCQ_POLYGON_VERTS_MAX 256
int pcq_scan_dev_count_batch_polygon(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds,
                                     const int32_t *verts_xy, size_t nsegments, size_t nverts,
                                     uint64_t *device_total, void *stream);

/* ---------------------------------------------------------------------------------------------
 * On-the-fly chunk index for device-resident LAST columns — the reference authors' own next step
 * (improvements.md:3-10), SURVEY.md §8f-3.  The first bounds (class) scan of a file through
 * pcq_scan_dev_indexed also records the integer AABB of every 4096-point chunk (a 256-bin class
 * histogram per 65536-point chunk); later scans of the SAME columns (same pointer and n) consult it:
 * chunks disjoint from the box are skipped, chunks inside it are counted without being read, only
 * straddling chunks are scanned (class counts are answered from the histograms alone).
 * Count and buffer collectors; grid collectors are refused (PCQ_ERR_ARG).  A buffer collector gets
 * exactly the records pcq_scan_dev appends, in the same order, after those it already holds: the
 * emit's count pass reads neither the positions nor the class bytes of a disjoint or contained
 * chunk (a disjoint one is then skipped by the emit as well; a contained one is read once, for its
 * records), and the ragged tail behind the last whole bounds chunk is always read.  Results are
 * identical to pcq_scan_dev; layouts the index does not cover fall through to pcq_scan_dev with all-zero
 * statistics and leave the index untouched: strided / LAS columns, positions not 16-byte aligned or fewer
 * than 4096 points (bounds), cls_stride != 1 (class).  PCQ_PRED_TIME,
 * PCQ_PRED_BOUNDS_CLASS, PCQ_PRED_BOUNDS_TIME and PCQ_PRED_BOUNDS_F64 have no index: they are served by pcq_scan_dev, the
 * statistics of such a scan are all zero, and the index is neither built nor changed by it.
 * Statistics of the last scan, in index chunks: for a count scan what it read; for a buffer scan the
 * chunks its count pass skipped (disjoint), took whole (contained) and read (straddling); after a
 * build, every chunk was read.  They are collected on the device and fetched (one wait) when asked.
 * ------------------------------------------------------------------------------------------- */
typedef struct pcq_index pcq_index;
typedef struct pcq_index_stats {
    uint64_t chunks;   /* chunks covered by the last indexed scan                       */
    uint64_t skipped;  /* ... disjoint from the query box: not read                     */
    uint64_t whole;    /* ... inside the box / answered from the histogram: not read    */
    uint64_t scanned;  /* ... read                                                      */
    uint64_t built;    /* 1 when the last scan built the index (it read everything)     */
} pcq_index_stats;
int pcq_index_new(pcq_ctx *ctx, pcq_index **out);
int pcq_index_free(pcq_index *ix);
int pcq_index_get_stats(pcq_index *ix, pcq_index_stats *out);
int pcq_scan_dev_indexed(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                         pcq_collector *c, void *stream);
/* PCQ_PRED_BOUNDS_CLASS (only; other kinds PCQ_ERR_ARG) through BOTH parts of the same index object, count and buffer
 * collectors (grid: PCQ_ERR_ARG).  Parts an earlier pcq_scan_dev_indexed built for these columns are used as they are, a
 * missing part is built first and serves later pcq_scan_dev_indexed bounds / class scans; then the pruned pass runs, on the
 * building call too.  A 4096-point bounds chunk takes its box state together with the state of the 65536-point class chunk
 * it lies in: no match in either -> skipped, nothing read; both contained -> counted whole, nothing read; everything else ->
 * its positions and its 4096 class bytes are read.  Results and records are pcq_scan_dev's for PCQ_PRED_BOUNDS_CLASS, byte
 * for byte and in order; the ragged tail behind the last whole bounds chunk is always read.  Covered: packed positions,
 * 16-byte aligned, at least 4096 points, with packed non-null class bytes; any other layout falls through to pcq_scan_dev with
 * all-zero statistics and leaves the index untouched.  Statistics in bounds chunks: chunks = n / 4096 = skipped + whole +
 * scanned, built = 1 when this call built either part. */
int pcq_scan_dev_indexed_combined(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                                  pcq_collector *c, void *stream);
/* PCQ_PRED_TIME (only; other kinds PCQ_ERR_ARG) through a third part of the same index object, count and buffer collectors
 * (grid: PCQ_ERR_ARG): per 4096-point chunk of the time column (pcq_columns.cls, the chunk of the bounds part) the minimum and
 * the maximum of its non-NaN times and the number of its NaNs.  The first call for a column (pointer and n) builds the part
 * while it scans (built = 1, scanned = chunks); later calls take each chunk's state against [wmin[0], wmax[0]) from it, in
 * IEEE f64 compares only: an empty range (start >= end, or a NaN bound), a chunk of NaNs, max < start or min >= end -> skipped,
 * nothing read; no NaN and start <= min and max < end -> counted whole, nothing read; everything else -> its 32 KiB of times
 * are read.  A file in acquisition order is close to monotone in time: a range then reads a handful of chunks.  Results and
 * records are pcq_scan_dev's for PCQ_PRED_TIME, byte for byte and in order (position, class 0, colour (0,0,0)), behind what the
 * collector holds; the ragged tail behind the last whole chunk is always read.  Covered: a packed time column (cls_stride 8),
 * 16-byte aligned, at least 4096 points — `xyz` may be NULL for a count collector, as for pcq_scan_dev; any other layout (LAS
 * records, a column aligned to 8 bytes only, fewer points) falls through to pcq_scan_dev with all-zero statistics and leaves
 * the index untouched.  Statistics in time chunks: chunks = n / 4096 = skipped + whole + scanned.  This entry neither reads nor
 * changes the bounds and class parts, and pcq_scan_dev_indexed / _combined neither read nor change the time part. */
int pcq_scan_dev_indexed_time(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                              pcq_collector *c, void *stream);
/* PCQ_PRED_BOUNDS_TIME (only; other kinds PCQ_ERR_ARG) through the bounds part AND the time part of the same index object, count
 * and buffer collectors (grid: PCQ_ERR_ARG).  The parts are those of pcq_scan_dev_indexed / _combined (keyed on the positions
 * pointer and n) and of pcq_scan_dev_indexed_time (keyed on the time pointer and n): a part an earlier scan built is used as it
 * is, a missing part is built first and serves those entries later; then the pruned pass runs, on the building call too.  Both
 * parts have the same 4096-point chunks; a chunk takes its box state together with its time state: no match in either ->
 * skipped, nothing read; both contained -> counted whole, nothing read; everything else -> its 48 KiB of positions and its 32 KiB
 * of times are read.  Results and records are pcq_scan_dev's for PCQ_PRED_BOUNDS_TIME, byte for byte and in order (position,
 * class 0, colour (0,0,0)), behind what the collector holds; the ragged tail behind the last whole chunk is always read, with its
 * own positions and times.  Covered: packed positions and a packed time column (pcq_columns.cls, cls_stride 8), each 16-byte
 * aligned, at least 4096 points; any other layout, and a predicate that can match nothing (a box outside the i32 range, an
 * empty or NaN range), falls through to pcq_scan_dev with all-zero statistics and leaves the index untouched.  Statistics in
 * 4096-point chunks: chunks = n / 4096 = skipped + whole + scanned, built = 1 when this call built either part. */
int pcq_scan_dev_indexed_bounds_time(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_index *ix,
                                     pcq_collector *c, void *stream);

/* The one collective of the path (main.rs:164-180) for callers that drive n GPUs from ONE process:
 * recv[i][0] = the sum over i of send[i][0] (8 bytes each in ctxs[i]'s HBM, e.g. the counter of
 * pcq_collector_new_count_at) — a single RCCL all-reduce(sum, u64, count = 1) over an intra-node communicator (xGMI).
 * Synchronous.  recv[i] may be send[i]; callers that want to fall back to summing the per-GPU values themselves when the
 * collective fails pass a different word, so that send[] is never touched.  One rank per GPU (two entries on one device
 * are refused).  n == 1 copies send to recv without RCCL unless option "allreduce_single_rank" is set on ctxs[0] (then
 * the one-rank communicator and the all-reduce really run).  RCCL is bound at run time; failure to find it is an error.
 * pcq_allreduce_prepare(devices, n) builds the communicator for that device list NOW (synchronous, thread-safe: loading RCCL
 * takes a fresh process 1-5 s, ncclCommInitAll 0.6 s), so that the all-reduce finds it ready; a caller that wants that beside
 * its scans calls it from a thread of its own and joins it before the all-reduce.  The library starts no thread. */
int pcq_allreduce_prepare(const int *devices, int n);
int pcq_allreduce_sum_u64(pcq_ctx *const *ctxs, const uint64_t *const *send, uint64_t *const *recv, int n);

/* Device memory helpers for callers that keep column blocks resident in HBM. */
int pcq_device_alloc(pcq_ctx *ctx, uint64_t bytes, void **out);
int pcq_device_free(pcq_ctx *ctx, void *p);
int pcq_copy_to_device(pcq_ctx *ctx, void *dst_device, const void *src_host, uint64_t bytes);
int pcq_copy_to_host(pcq_ctx *ctx, void *dst_host, const void *src_device, uint64_t bytes);
int pcq_device_memset(pcq_ctx *ctx, void *dst_device, int value, uint64_t bytes, void *stream);

/* Reads [file_offset, file_offset + bytes) of an open file into device memory at the rate of the host block path (pinned
 * double buffering, parallel pread) — for callers that keep column blocks resident in HBM.  Synchronous. */
int pcq_read_fd_to_device(pcq_ctx *ctx, int fd, uint64_t file_offset, uint64_t bytes, void *d_dst);

/* Restricts the CALLING thread to the CPUs of the NUMA node the context's GPU is attached to (no-op when the
 * node is unknown or option "numa_local" is 0).  For caller threads that produce the bytes a scan will read —
 * memory they touch first then sits next to the GPU's staging buffers. */
int pcq_bind_thread_near_device(pcq_ctx *ctx);

/* Options: "blocks_per_cu" (persistent blocks per CU of the strided count kernels), "chunk_points" (points per staging
 * chunk of the host paths), "copy_threads" (threads filling a staging chunk, default 16), "numa_local",
 * "allreduce_single_rank", "allreduce_fail" (tests: 1 = pcq_allreduce_sum_u64 fails before it touches anything, 2 = after the
 * reduction ran, 3 = inside the RCCL group, behind rank 0), "grid_pending_budget" (points a grid collector may hold unfolded; 0 = default), "grid_agg" (pass 0 folds a
 * tile's duplicate cells before they travel: 0 = while it pays, 1 = every tile, 2 = never; same results in every mode),
 * "grid_f2" (tests: the second-level fan-out a fold starts from; 0 = from the measured estimate), "host_in_place" (host / file
 * scans with a count or grid collector read the pinned staging ring in place over PCIe: 0 never, 1 always, 2 = while the
 * process's copy path is being set up — the default), "emit_park_max" / "emit_sparse_max" (buffer collector: a 2048-point tile with at
 * most that many matches leaves them as 16-byte words in the count pass — default 256, bounds queries —
 * or is written by one wave from the count pass's match bits — default 64; 0 = never), "grid_tuple16" / "grid_stream" (tests: force
 * the grid collector's tuple size — 1 = 16 bytes with the selector, 2 = without, 0 = 24 bytes — and the coarse fold's form —
 * 1 = k_fold_stream, 0 = k_fold<BIG>; same results in every combination), "grid_block_pad" (tests: 0 .. 65536 units of 16
 * bytes left between a tile's block of tuples and the next one — moves every block's address and phase; same results for
 * every value; default 0), "grid_p0_blocks" (tests: k > 0 = pass 0 of a grid scan runs on min(k, one per CU) workgroups, so that
 * each takes more tiles in turn; it only lowers the count; same results for every value; 0 = one per CU, the default), "scratch_cap_words" (tests: while > 0, growing the
 * context's device scratch beyond that many 8-byte words fails with PCQ_ERR_NOMEM without an allocation — a buffer scan then
 * emits without parking its matches; 0 = no cap, the default).  pcq_get_option also
 * reads "numa_node" and the grid diagnostics "grid_folds", "grid_level2" (folds that needed a second partition level),
 * "grid_refolds" (folds repeated with more partitions), "grid_level2_exact" (second levels repeated in the counting form),
 * "grid_compactions" (folds that copied short fragments together first), "grid_deferred" (bins the streaming fold left to
 * k_fold<BIG>: their survivors outgrew the list), "grid_dense_deferred" (second-level partitions k_fold_dense left to
 * k_fold<SMALL>: more than its chunk of 1536 tuples; both also count in an attempt that is repeated with more partitions),
 * "grid_last_f2", "grid_last_tuples" (tuples the last fold found pending: what is left of the matches after pass 0's own
 * fold), "grid_last_tuple_bytes" (16 or 24: the tuple size the last grid scan packed its matches in) and "emit_park_fallbacks" (buffer scans that found no room for the parked matches
 * and read their thin tiles a second time instead).  (The kernel-shape experiments of round 1 —
 * "k1_variant", "batch_variant", ... — are options of libpcq_lab.so only: include/pcq_lab.h.) */
int pcq_set_option(pcq_ctx *ctx, const char *key, int64_t value);
int pcq_get_option(pcq_ctx *ctx, const char *key, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* PCQ_H */
