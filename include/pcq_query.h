/*
 * pcq_query.h — C view of the C++ host layer (libpcq_query.so), so that tests and other languages
 * can call the file-level operators of the reference by name:
 *
 *   Searcher::search_file for BoundsSearcher / ClassSearcher     query/src/search/searcher.rs:24-152
 *   ... and TimeSearcher (GPS time range)                         query/src/search/las.rs:297-358
 *   ... and the combined BoundsClassSearcher / BoundsTimeSearcher  (not in the reference)
 *   CountCollector / BufferCollector / GridSampledCollector      query/src/collect_points.rs:14-127
 *   parse_aabb, get_all_input_files, is_valid_file, get_total_bounds   query/src/main.rs:29-120, 185-189
 *
 * libpcq_query.so contains NO scan code: every function below that touches point data calls the
 * HIP library through include/pcq.h (pcq_scan_host).  Functions return 0 or a negative pcq_status;
 * pcq_query_last_error() returns the message of the last failure on the calling thread and
 * pcq_query_last_was_panic() tells whether the reference would have panicked (exit code 101).
 */
#ifndef PCQ_QUERY_H
#define PCQ_QUERY_H

#include "pcq.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pcq_host_collector pcq_host_collector;

const char *pcq_query_last_error(void);
int pcq_query_last_was_panic(void);

/* raw::Header::read_from + Header::from_raw on a memory image (no GPU needed). */
typedef struct pcq_las_header_info {
    uint8_t version_major, version_minor;
    uint8_t point_data_record_format;
    uint8_t _pad;
    uint16_t header_size;
    uint16_t point_data_record_length;
    uint32_t offset_to_point_data;
    uint32_t _pad2;
    uint64_t number_of_points;
    double scale[3], offset[3], min[3], max[3];
} pcq_las_header_info;
int pcq_query_parse_las_header(const uint8_t *data, size_t len, int mask_format, pcq_las_header_info *out);

/* main.rs:59-92 (PCQ_ERR_PANIC when min > max), :185-189, :94-120 — no GPU needed. */
int pcq_query_parse_aabb(const char *s, double bmin[3], double bmax[3]);
int pcq_query_is_valid_file(const char *path);
int pcq_query_get_total_bounds(const char *const *files, size_t nfiles, double bmin[3], double bmax[3]);

/* The LZ4 Frame reader the LAZER searches inflate column blobs with (stand-in for lz4::Decoder,
 * readers/src/lazer_reader.rs:176-265): the first `need` bytes of the frame at src -> out (cap >= need),
 * as read_exact calls of `unit` bytes each would get them (4 = read_i32 ..., 0 = a single call).
 * Host-only, no GPU needed.  PCQ_ERR_EOF = read_exact's UnexpectedEof, PCQ_ERR_HEADER = an LZ4 error. */
int pcq_query_lz4_frame_decode(const uint8_t *src, size_t n, uint64_t need, uint64_t unit, uint8_t *out, uint64_t cap);

/* Collectors on the calling thread's context for `device`. */
int pcq_query_collector_new_count(int device, pcq_host_collector **out);
int pcq_query_collector_new_buffer(int device, pcq_host_collector **out);
int pcq_query_collector_new_grid(int device, const double bmin[3], const double bmax[3], double cell_size,
                                 pcq_host_collector **out);
int pcq_query_collector_free(pcq_host_collector *c);
int pcq_query_collector_point_count(pcq_host_collector *c, uint64_t *out);
/* 0: points() is None; 1: Some.  Copies up to cap points (buffer: file order). */
int pcq_query_collector_has_points(pcq_host_collector *c);
int pcq_query_collector_points(pcq_host_collector *c, pcq_point *out, uint64_t cap, uint64_t *out_n);
int pcq_query_collector_grid_cells(pcq_host_collector *c, uint64_t *out, uint64_t cap, uint64_t *out_n);

/* BoundsSearcher::search_file / ClassSearcher::search_file with SearchImplementation
 * (0 = Regular, 1 = Optimized).  *las_record_size receives the value the reference prints with
 * `Point record size: {}` (las.rs:73) or is left at -1. */
int pcq_query_search_file_bounds(const char *path, const double bmin[3], const double bmax[3], int optimized,
                                 pcq_host_collector *c, int *las_record_size);
int pcq_query_search_file_class(const char *path, uint8_t cls, int optimized, pcq_host_collector *c);
/* TimeSearcher::search_file: GPS time in [start, end) (query/src/search/las.rs:297-358; not wired into the reference's
 * searcher.rs).  .las / .last with optimized = 1; matches are recorded with class 0 and colour (0,0,0).  A file of format 0
 * or 2, or above 10, is PCQ_ERR_FORMAT; .laz / .lazer and the Regular implementation are PCQ_ERR_UNSUPPORTED. */
int pcq_query_search_file_time(const char *path, double start, double end, int optimized, pcq_host_collector *c);
/* The combined searches (--combine; not in the reference, whose CLI rejects the pair): a point matches when the bounds
 * search and the class / time search would both match it.  The plan is the attribute search's (its errors, its columns and
 * its records: class byte and colour for BOUNDS_CLASS, class 0 and colour (0,0,0) for BOUNDS_TIME), then the bounds search's
 * header early-out (a disjoint file is 0 matches, no GPU) and pcq_box_to_local.  .las / .last with optimized = 1; .laz and
 * .lazer and the Regular implementation are PCQ_ERR_UNSUPPORTED. */
int pcq_query_search_file_bounds_class(const char *path, const double bmin[3], const double bmax[3], uint8_t cls, int optimized,
                                       pcq_host_collector *c);
int pcq_query_search_file_bounds_time(const char *path, const double bmin[3], const double bmax[3], double start, double end, int optimized,
                                      pcq_host_collector *c);

/* A dataset resident in HBM (host/resident.cpp; not in the reference, which re-reads the files for every query): the
 * positions and classification blocks of LAST files are loaded into `device`'s HBM once; every count query over them
 * is the reference's per-file host prologue (early-out last.rs:92-94, box conversion :98-109) + ONE batched launch
 * (pcq_scan_dev_count_batch).  Same counts as `query --bounds|--class ... --optimized --parallel` on those files. */
typedef struct pcq_host_resident pcq_host_resident;
int pcq_query_resident_load(int device, const char *const *files, size_t nfiles, pcq_host_resident **out);
int pcq_query_resident_free(pcq_host_resident *r);
int pcq_query_resident_count_bounds(pcq_host_resident *r, const double bmin[3], const double bmax[3], uint64_t *matches,
                                    uint64_t *points_scanned);
int pcq_query_resident_count_class(pcq_host_resident *r, uint8_t cls, uint64_t *matches, uint64_t *points_scanned);
/* Box AND class, count only (`--combine --bounds ... --class`): the per-file prologue of the bounds count (header early-out,
 * box conversion; PCQ_ERR_PANIC for min > max) + ONE batched launch over the positions and classification blocks of the
 * surviving files (pcq_scan_dev_count_batch_combined).  points_scanned: the points of the files whose headers meet the box. */
int pcq_query_resident_count_bounds_class(pcq_host_resident *r, const double bmin[3], const double bmax[3], uint8_t cls,
                                          uint64_t *matches, uint64_t *points_scanned);
/* Many boxes in one pass (`--bounds`, count only, nboxes times): bmin and bmax are [nboxes][3]; matches[q] and
 * points_scanned[q] (NULL: not wanted) are what pcq_query_resident_count_bounds(r, bmin + 3q, bmax + 3q, ...) returns, for every
 * q.  Per file and box the prologue of that entry (header early-out, box conversion); a file whose header misses box q is not
 * asked box q, a file no box of a group meets is not read.  The boxes are taken in their order in groups of
 * PCQ_MULTI_BOX_MAX (pcq.h), ONE launch per group (pcq_scan_dev_count_batch_multi): the positions of the files a group meets
 * are read once, not once per box.  points_read (NULL: not wanted): the points of the segments of every launch, summed — what
 * HBM served.  nboxes == 0 is PCQ_OK with nothing written.  A null r, bmin, bmax or matches is PCQ_ERR_ARG before any device
 * is touched.  If some box's own call would fail (PCQ_ERR_PANIC: min > max) the status of the lowest such box is returned,
 * nothing is launched and nothing is written. */
int pcq_query_resident_count_bounds_many(pcq_host_resident *r, size_t nboxes, const double *bmin, const double *bmax, uint64_t *matches,
                                         uint64_t *points_scanned, uint64_t *points_read);
/* What is in this box, by class (`--combine --bounds ... --class c`, count only, for every c at once): hist[c] is what
 * pcq_query_resident_count_bounds_class(r, bmin, bmax, c, ...) returns as matches, for every c in 0 .. 255, zeros included, and
 * points_scanned (NULL: not wanted) is what that entry reports.  The per-file prologue of the bounds count (header early-out,
 * box conversion; PCQ_ERR_PANIC for min > max) + ONE launch over the positions and classification blocks of the surviving
 * files (pcq_scan_dev_class_hist_batch): the data is read once, not once per class, and the caller need not know which classes
 * occur.  Works on a dataset from any of the loaders.  A null r, bmin, bmax or hist is PCQ_ERR_ARG before any device is
 * touched; on any failure hist is left as it was. */
int pcq_query_resident_count_bounds_by_class(pcq_host_resident *r, const double bmin[3], const double bmax[3], uint64_t hist[256],
                                             uint64_t *points_scanned);
/* Point and density queries over a resident dataset: the per-file searches over every loaded file, in load order, into ONE
 * collector.  Count and buffer collectors go through each file's chunk index (pcq_scan_dev_indexed: the first query of a
 * kind builds it, later ones read only the chunks that straddle the box); grid collectors through pcq_scan_dev, unpruned.
 * A dataset from pcq_query_resident_load (no colour blocks) refuses buffer and grid collectors, and a collector of another
 * device than the dataset's is refused (PCQ_ERR_ARG).
 * Like pcq_query_resident_load, and also the colour blocks (formats with colour): what point queries need. */
int pcq_query_resident_load_points(int device, const char *const *files, size_t nfiles, pcq_host_resident **out);
/* == pcq_query_search_file_bounds(path, bmin, bmax, optimized=1, c) for every loaded file, in load order, into ONE collector:
 * the same count, records in the same order, grid cells and winners — the header early-out (last.rs:92-94) included, which
 * leaves the collector's file-order index where it was; PCQ_ERR_PANIC for min > max. */
int pcq_query_resident_search_bounds(pcq_host_resident *r, const double bmin[3], const double bmax[3], pcq_host_collector *c);
/* == pcq_query_search_file_class(path, cls, optimized=1, c) for every loaded file, in load order. */
int pcq_query_resident_search_class(pcq_host_resident *r, uint8_t cls, pcq_host_collector *c);
/* == pcq_query_search_file_bounds_class(path, bmin, bmax, cls, optimized=1, c) for every loaded file, in load order, the
 * header early-out included.  Count and buffer collectors go through both parts of each file's chunk index
 * (pcq_scan_dev_indexed_combined: the parts are those of search_bounds and search_class, built by whichever comes first);
 * grid collectors through pcq_scan_dev. */
int pcq_query_resident_search_bounds_class(pcq_host_resident *r, const double bmin[3], const double bmax[3], uint8_t cls,
                                           pcq_host_collector *c);
/* The loader with the blocks named: `blocks` is a set of the bits below.  0 = pcq_query_resident_load, PCQ_RESIDENT_COLOUR =
 * pcq_query_resident_load_points; PCQ_RESIDENT_TIME adds every file's GPS time block, found as the LAST time search finds it
 * (pcq_query_search_file_time): at offset_to_point_data + n*20 (formats 1, 3-5) or + n*22 (6-10).  With that bit a file of
 * format 0 or 2 ("File {path} does not contain GPS times!") or above 10 is PCQ_ERR_FORMAT and a block reaching past the file
 * PCQ_ERR_EOF; the load fails as a whole on the first such file.  Any other bit is PCQ_ERR_ARG. */
#define PCQ_RESIDENT_COLOUR 1u
#define PCQ_RESIDENT_TIME 2u
int pcq_query_resident_load_with(int device, const char *const *files, size_t nfiles, unsigned blocks, pcq_host_resident **out);
/* == pcq_query_search_file_time(path, start, end, optimized=1, c) for every loaded file, in load order, into ONE collector (no
 * file-level early-out: a header has no time bounds).  Count and buffer collectors go through the time part of each file's
 * chunk index (pcq_scan_dev_indexed_time), grid collectors through pcq_scan_dev.  Needs a dataset loaded with
 * PCQ_RESIDENT_TIME (else PCQ_ERR_ARG) and no colour blocks, whatever the collector: a time record's colour is (0,0,0). */
int pcq_query_resident_search_time(pcq_host_resident *r, double start, double end, pcq_host_collector *c);
/* Box AND time, count only (`--combine --bounds ... --time`): the per-file prologue of pcq_query_resident_count_bounds_class
 * (header early-out, box conversion; PCQ_ERR_PANIC for min > max) + ONE batched launch over the positions and time blocks of
 * the surviving files (pcq_scan_dev_count_batch_bounds_time).  points_scanned: the points of the files whose headers meet the
 * box.  Needs a dataset loaded with PCQ_RESIDENT_TIME (else PCQ_ERR_ARG). */
int pcq_query_resident_count_bounds_time(pcq_host_resident *r, const double bmin[3], const double bmax[3], double start, double end,
                                         uint64_t *matches, uint64_t *points_scanned);
/* When was this box scanned (`--combine --bounds ... --time e[b] e[b+1]`, count only, for every b at once): edges is nbins + 1
 * f64 values e[0] <= e[1] <= ... <= e[nbins], none NaN (infinities, -0.0 and equal neighbours are allowed); hist[b] is what
 * pcq_query_resident_count_bounds_time(r, bmin, bmax, edges[b], edges[b+1], ...) returns as matches, for every b in 0 .. nbins-1,
 * and points_scanned (NULL: not wanted) is what that entry reports.  The per-file prologue of that entry + one launch over the
 * positions and time blocks of the surviving files per group of PCQ_TIME_BINS_MAX bins (pcq.h, pcq_scan_dev_time_hist_batch):
 * the data is read once per group, not once per bin.  The checks in their order: a null r, bmin, bmax, edges or hist is
 * PCQ_ERR_ARG; nbins == 0 is PCQ_OK with nothing written; a NaN or decreasing edge is PCQ_ERR_ARG — these three touch neither
 * r nor a device; a dataset loaded without PCQ_RESIDENT_TIME is PCQ_ERR_ARG; last the box's own error (PCQ_ERR_PANIC for
 * min > max).  On any failure hist and points_scanned are left as they were. */
int pcq_query_resident_count_bounds_by_time(pcq_host_resident *r, const double bmin[3], const double bmax[3], const double *edges,
                                            size_t nbins, uint64_t *hist, uint64_t *points_scanned);
/* Where in this box are the points (`--bounds`, count only, for every cell of a 2-D raster at once): the raster is nx x ny cells
 * of cell_size world units from the origin (bmin[0], bmin[1]), row-major with y upward (raster[cy * nx + cx]), and counts the
 * points with z in [bmin[2], zmax].  The checks in their order, before the dataset or a device is touched: a null r, bmin or
 * raster is PCQ_ERR_ARG; nx * ny == 0 is PCQ_OK with nothing written; nx * ny above PCQ_QUERY_RASTER_CELLS_MAX is PCQ_ERR_ARG; a
 * cell_size that is not finite or not above 0 is PCQ_ERR_ARG.  Then per file the prologue of pcq_query_resident_count_bounds with
 * the world box bmin .. (bmin[0] + nx cell_size, bmin[1] + ny cell_size, zmax): the header early-out, pcq_box_to_local bug for
 * bug, PCQ_ERR_PANIC for bmin[2] > zmax.  A cell is a whole number of a file's lattice steps: k = nearbyint(cell_size / scale[a])
 * must lie in 1 .. 2^32 - 1 with |cell_size / scale[a] - k| <= 1e-9 k, and the file's lmin[0] and lmin[1] inside the i32 range,
 * else PCQ_ERR_UNSUPPORTED naming the file.  The file's box becomes lmin[a] .. lmin[a] + n_a k - 1 on x and y (the cells are full
 * and half-open in the lattice; z stays as converted), so raster[cy * nx + cx] is the number of stored points (X, Y, Z), over the
 * surviving files, with (X - lmin[0]) / k_x == cx, (Y - lmin[1]) / k_y == cy and Z inside.  ONE launch over the positions of the
 * surviving files while nx * ny <= PCQ_RASTER_CELLS_MAX (pcq.h, pcq_scan_dev_raster_batch); a larger raster is cut into blocks of
 * at most that many cells, one launch per block into its own counter words, each reading every surviving file.  points_scanned
 * (NULL: not wanted): what pcq_query_resident_count_bounds reports for the world box.  On any failure raster and points_scanned
 * are left as they were. */
#define PCQ_QUERY_RASTER_CELLS_MAX (1u << 20)
int pcq_query_resident_count_bounds_raster(pcq_host_resident *r, const double bmin[3], double zmax, double cell_size, uint64_t nx,
                                           uint64_t ny, uint64_t *raster, uint64_t *points_scanned);
/* How high is this box, cell by cell: over the raster of pcq_query_resident_count_bounds_raster — nx x ny cells of cell_size world
 * units from (bmin[0], bmin[1]), row-major with y upward, the points with z in [bmin[2], zmax] — zlo[cy * nx + cx] is the lowest
 * and zhi[cy * nx + cx] the highest world z of the points that entry counts in cell (cx, cy); a cell it counts no point in is NaN
 * in both.  The highest z per cell is a surface model, the lowest a first ground model, their difference a height above ground.
 * The checks are that entry's, in its order and before the dataset or a device is touched: a null r, bmin, zlo or zhi is
 * PCQ_ERR_ARG; nx * ny == 0 is PCQ_OK with nothing written; nx * ny above PCQ_QUERY_RASTER_CELLS_MAX is PCQ_ERR_ARG; a cell_size
 * that is not finite or not above 0 is PCQ_ERR_ARG.  The per-file prologue is that entry's too — the header early-out,
 * pcq_box_to_local bug for bug, PCQ_ERR_PANIC for bmin[2] > zmax, PCQ_ERR_UNSUPPORTED naming the file for a cell that is no whole
 * number of its lattice steps — and one rule more: a surviving file whose scale[2] is not finite or not above 0 is
 * PCQ_ERR_UNSUPPORTED naming the file.  World z is (Z as f64 * scale[2]) + offset[2] of the stored integer Z, the value a record
 * of pcq_query_resident_search_bounds carries; it does not decrease with Z, so the results are those of a min / max over these
 * records' z, bit for bit.  The surviving files are scanned in groups of one z lattice (bitwise-equal scale[2] and offset[2]):
 * per group and per block of at most PCQ_ZRANGE_CELLS_MAX cells (pcq.h) ONE pcq_scan_dev_zrange_raster_batch over the positions of
 * the group's files; the groups are merged on the host.  points_scanned (NULL: not wanted): what
 * pcq_query_resident_count_bounds_raster reports.  On any failure zlo, zhi and points_scanned are left as they were. */
int pcq_query_resident_bounds_zrange_raster(pcq_host_resident *r, const double bmin[3], double zmax, double cell_size, uint64_t nx,
                                            uint64_t ny, double *zlo, double *zhi, uint64_t *points_scanned);
/* How many points lie inside this outline (count only): the outline is nverts world vertices xy[nverts][2], closed from the last to
 * the first, and counts the points with z in [zmin, zmax]; even-odd over the edges, so orientation does not matter and a
 * self-intersecting outline is legal (pcq.h, pcq_scan_dev_count_batch_polygon, has the rule, which is exact in each file's integer
 * lattice).  The checks in their order, before the dataset or a device is touched: a null r, xy or matches is PCQ_ERR_ARG; nverts < 3
 * or above PCQ_POLYGON_VERTS_MAX is PCQ_ERR_ARG; a vertex coordinate that is not finite is PCQ_ERR_ARG.  Then per file, in load
 * order, the prologue of pcq_query_resident_count_bounds with the world box (min x, min y, zmin) .. (max x, max y, zmax) of the
 * outline: the header early-out, pcq_box_to_local bug for bug, PCQ_ERR_PANIC for zmin > zmax.  lmin[2] and lmax[2] of that
 * conversion are the z range.  A vertex becomes V.x = nearbyint((x - offset[0]) / scale[0]), V.y = nearbyint((y - offset[1]) /
 * scale[1]): two f64 operations in this order under the default rounding (ties to even).  A surviving file whose scale[0] or
 * scale[1] is not finite or not above 0, a vertex that lands outside the i32 range and an outline that spans more than 2^31 - 1
 * lattice steps on an axis are PCQ_ERR_UNSUPPORTED naming the file.  The file's x and y range is the lattice bounding box of the
 * ROUNDED vertices, not the converted world box (whose truncation and x-scale quirk would cut vertices off).  Then ONE
 * pcq_scan_dev_count_batch_polygon over the positions of the surviving files.  points_scanned (NULL: not wanted): what
 * pcq_query_resident_count_bounds reports for the world box.  On any failure matches and points_scanned are left as they were.
 * Works on a dataset from any of the loaders. */
int pcq_query_resident_count_polygon(pcq_host_resident *r, size_t nverts, const double *xy /* [nverts][2], world */,
                                     double zmin, double zmax, uint64_t *matches, uint64_t *points_scanned);
/* == pcq_query_search_file_bounds_time(path, bmin, bmax, start, end, optimized=1, c) for every loaded file, in load order, into
 * ONE collector: the same count, the same records byte for byte and in order (class 0, colour (0,0,0), whether or not colour
 * blocks are loaded), the same grid cells and winners; the header early-out leaves the collector's file-order index where it
 * was.  Count and buffer collectors go through the bounds and time parts of each file's chunk index
 * (pcq_scan_dev_indexed_bounds_time: the parts are those of search_bounds and search_time, built by whichever comes first);
 * grid collectors through pcq_scan_dev.  Needs a dataset loaded with PCQ_RESIDENT_TIME (else PCQ_ERR_ARG). */
int pcq_query_resident_search_bounds_time(pcq_host_resident *r, const double bmin[3], const double bmax[3], double start, double end,
                                          pcq_host_collector *c);
/* Index statistics of the last resident search, summed over its files (those it scanned through an index; none for a grid
 * collector).  Waits for the search's scans. */
int pcq_query_resident_last_stats(pcq_host_resident *r, pcq_index_stats *out);

/* The whole CLI in-process (main.rs:191-319); returns the exit code. */
int pcq_query_main(int argc, const char *const *argv);

/* Test entries (the `query` binary cannot reach them).
 * pcq_query_main_with_hooks: the CLI with the parallel driver's test hooks — device_slots: a "0,0"-style device list, repeats
 * allowed (two device SLOTS on one GPU run the N > 1 paths of main.rs:146-183's merge), or NULL; allreduce_fail: 0, or make the
 * count merge's collective fail through the real RCCL calls, 1 = before anything is touched, 2 = after the reduction ran.
 * pcq_query_simulate_schedule: the file -> device-slot schedule of the parallel driver (every slot starts with its own
 * longest-processing-time share; a slot that runs dry takes from the fullest) when slot k's context is ready at ready_ms[k]
 * and a file costs ms_per_unit x cost[i]; home_slot (may be NULL) = the share a file started in.  No GPU involved. */
int pcq_query_main_with_hooks(int argc, const char *const *argv, const char *device_slots, int allreduce_fail);
int pcq_query_simulate_schedule(const uint64_t *cost, size_t nfiles, const double *ready_ms, int nslots, double ms_per_unit,
                                int *slot_of_file, int *home_slot, double *makespan_ms);
/* Test entry: the host-only plan of a time search (TimeSearcher, optimized) of a .las / .last file — what search_file decides
 * before any GPU work.  Returns the plan's status; *needs_gpu = 1 when a scan would follow, with its columns (the pointers are
 * BYTE OFFSETS into the file) and predicate.  Wakes no GPU. */
int pcq_query_test_plan_time(const char *path, double start, double end, pcq_columns *cols, pcq_predicate *pred, int *needs_gpu);
/* Test entry: the same for a combined search — cls 0..255: BOUNDS AND CLASS; cls < 0: BOUNDS AND TIME over [start, end). */
int pcq_query_test_plan_combined(const char *path, const double bmin[3], const double bmax[3], int cls, double start, double end,
                                 pcq_columns *cols, pcq_predicate *pred, int *needs_gpu);
/* Test entry: the two halves of a LAST bounds search with something in between — the file's plan is made (header, offsets,
 * box: the host prologue of run_search_parallel), then, if `replacement` is not NULL, that file is renamed over `path`, then the
 * plan is executed.  A plan must not be executed on another file under the same name. */
int pcq_query_test_plan_replace_execute(const char *path, const char *replacement, const double bmin[3], const double bmax[3],
                                        pcq_host_collector *c);

#ifdef __cplusplus
}
#endif
#endif
