/*
 * pcq_query_stats.h — the per-cell STATISTICS of a box on a resident dataset, beside the entries of pcq_query.h (libpcq_query.so).
 *
 * Why a header of its own: tests/test_query_binding.py holds pcq_query.h and query_binding.sig to exactly the declarations they
 * had when the mean-height raster was added, and a change that adds an entry leaves existing tests as they are.  So the new entry
 * is declared here, with a signature table of its own (query_binding.stats_sig).  A later change that is free to touch that test
 * may fold this header back into pcq_query.h, behind pcq_query_resident_bounds_zrange_raster.
 */
#ifndef PCQ_QUERY_STATS_H
#define PCQ_QUERY_STATS_H

#include "pcq_query.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The mean-height raster of a box: "how high is this box on average, cell by cell?".  The cells, the box and the arguments'
 * checks are those of pcq_query_resident_bounds_zrange_raster: nx x ny cells of cell_size from (bmin[0], bmin[1]), z in [bmin[2],
 * zmax].  count[cy * nx + cx] is what pcq_query_resident_count_bounds_raster counts in cell (cx, cy), zmean[cy * nx + cx] the mean
 * world z of those points, NaN exactly where the count is 0; *points_scanned (may be null) is what that entry reports.
 *
 * The surviving files are grouped by bitwise-equal z scale and z offset, groups in the order of their first file; within a group
 * the files, in load order, are cut into batches of fewer than 2^32 points.  Per batch and per block of at most PCQ_ZSUM_CELLS_MAX
 * cells (pcq.h) ONE pcq_scan_dev_zsum_raster_batch gives, per cell, the u64 count `cnt` and the i64 sum `sum` of the stored z, both
 * exact.  The result is DEFINED as, per cell, over the batches in that order, in f64 under the default rounding with every product
 * rounded before the add (no fused multiply-add), W and N starting at 0:
 *
 *     W += offset * (double)cnt + scale * (double)(int64_t)sum;   N += cnt;
 *     count[c] = N;   zmean[c] = N ? W / (double)N : NaN
 *
 * with scale and offset the batch's z scale and z offset.
 *
 * Checked in this order before the dataset or a device is touched: a null r, bmin, count or zmean (PCQ_ERR_ARG "null argument");
 * nx * ny == 0 (PCQ_OK, nothing written); more than PCQ_QUERY_RASTER_CELLS_MAX cells (PCQ_ERR_ARG "... cells ..."); a cell_size
 * that is not finite or not above 0 (PCQ_ERR_ARG "... cell_size ...").  Then: bmin[2] > zmax is PCQ_ERR_PANIC; a cell_size that is
 * no whole number of a scanned file's lattice steps, a scanned file whose z scale is not finite or not above 0, and a scanned file
 * of 2^32 points or more are PCQ_ERR_UNSUPPORTED.  On any failure count, zmean and *points_scanned are left as they were. */
int pcq_query_resident_bounds_zmean_raster(pcq_host_resident *r, const double bmin[3], double zmax, double cell_size, uint64_t nx,
                                           uint64_t ny, uint64_t *count, double *zmean, uint64_t *points_scanned);

#ifdef __cplusplus
}
#endif
#endif
