/*
 * pcq_query_classes.h — the per-cell statistics of the points of a SET OF CLASSES of a box on a resident dataset, beside the entries
 * of pcq_query.h and pcq_query_stats.h (libpcq_query.so).
 *
 * Why a header of its own: tests hold pcq_query.h (46 declarations, query_binding.sig) and pcq_query_stats.h (one declaration,
 * query_binding.stats_sig) to exactly what they declared when this entry was added, and a change that adds an entry leaves existing
 * tests as they are.  So the new entry is declared here, with a signature table of its own (query_binding.classes_sig).  A later
 * change that is free to touch those tests may fold this header back, behind pcq_query_resident_bounds_zmean_raster.
 */
#ifndef PCQ_QUERY_CLASSES_H
#define PCQ_QUERY_CLASSES_H

#include "pcq_query_stats.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The mean-height raster of the ground of a box: "how high are the points of these classes in this box on average, cell by cell?".
 * A terrain model is the set {2}, or {2, 9}; a surface model every class but noise.  class_set is eight words: class c is in the set
 * when bit (c & 31) of class_set[c >> 5] is set — the whole class byte, as the LAST class search compares it.
 *
 * The cells, the box and the arguments' checks are those of pcq_query_resident_bounds_zmean_raster (pcq_query_stats.h), in its
 * order: nx x ny cells of cell_size from (bmin[0], bmin[1]), z in [bmin[2], zmax].  count[cy * nx + cx] is the number of points of
 * cell (cx, cy) whose class byte is in the set — the class-filtered density raster — and zmean[cy * nx + cx] the mean world z of
 * those points, NaN exactly where the count is 0; *points_scanned (may be null) is what the unfiltered entry reports: the points of
 * the files the box reaches, whatever their class.
 *
 * The result is DEFINED by the formula of pcq_query_resident_bounds_zmean_raster over the same batches — the surviving files grouped
 * by bitwise-equal z scale and z offset, groups in the order of their first file, within a group the files in load order cut into
 * batches of fewer than 2^32 points (counted over all their points, whatever their class), per batch and block of at most
 * PCQ_ZSUM_CELLS_MAX cells ONE pcq_scan_dev_zsum_raster_batch_classes (pcq.h) — with `cnt` and `sum` taken over the points whose class
 * byte is in the set: per cell, over the batches in that order, in f64 under the default rounding with every product rounded before
 * the add (no fused multiply-add), W and N starting at 0:
 *
 *     W += offset * (double)cnt + scale * (double)(int64_t)sum;   N += cnt;
 *     count[c] = N;   zmean[c] = N ? W / (double)N : NaN
 *
 * Two consequences.  With all 256 bits set, count and zmean are bit for bit those of pcq_query_resident_bounds_zmean_raster.  With an
 * empty set (eight zero words) every count is 0 and every mean is NaN, and nothing is launched; every refusal below is still made.
 *
 * Checked in this order before the dataset or a device is touched: a null r, bmin, class_set, count or zmean (PCQ_ERR_ARG "null
 * argument"); nx * ny == 0 (PCQ_OK, nothing written); more than PCQ_QUERY_RASTER_CELLS_MAX cells (PCQ_ERR_ARG "... cells ..."); a
 * cell_size that is not finite or not above 0 (PCQ_ERR_ARG "... cell_size ...").  Then: bmin[2] > zmax is PCQ_ERR_PANIC; a cell_size
 * that is no whole number of a scanned file's lattice steps, a scanned file whose z scale is not finite or not above 0, and a scanned
 * file of 2^32 points or more are PCQ_ERR_UNSUPPORTED.  On any failure count, zmean and *points_scanned are left as they were. */
int pcq_query_resident_bounds_zmean_raster_classes(pcq_host_resident *r, const double bmin[3], double zmax, double cell_size,
                                                   uint64_t nx, uint64_t ny, const uint32_t class_set[8], uint64_t *count, double *zmean,
                                                   uint64_t *points_scanned);

#ifdef __cplusplus
}
#endif
#endif
