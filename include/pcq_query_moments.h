/*
 * pcq_query_moments.h — the per-cell second moment of the heights of a box on a resident dataset, beside the entries of pcq_query.h,
 * pcq_query_stats.h and pcq_query_classes.h (libpcq_query.so).
 *
 * Why a header of its own: tests hold pcq_query.h (46 declarations, query_binding.sig), pcq_query_stats.h and pcq_query_classes.h
 * (one declaration each, query_binding.stats_sig and .classes_sig) to exactly what they declared when this entry was added, and a
 * change that adds an entry leaves existing tests as they are.  So the new entry is declared here, with a signature table of its own
 * (query_binding.moments_sig).  A later change that is free to touch those tests may fold this header back.
 */
#ifndef PCQ_QUERY_MOMENTS_H
#define PCQ_QUERY_MOMENTS_H

#include "pcq_query_stats.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The height-spread raster of a box: "how rough is this box, cell by cell?" — roughness, canopy spread, the noise check of a tile.
 *
 * The cells, the box and the arguments' checks are those of pcq_query_resident_bounds_zmean_raster (pcq_query_stats.h), in its
 * order: nx x ny cells of cell_size from (bmin[0], bmin[1]), z in [bmin[2], zmax].  count[cy * nx + cx] and zmean[cy * nx + cx] are
 * bit for bit what that entry returns; zstd[cy * nx + cx] is the POPULATION standard deviation (divisor N, not N - 1) of the world z
 * of the cell's points, NaN exactly where the count is 0 and exactly 0.0 where all heights of the cell are one stored value of one
 * file.  *points_scanned (may be null) is what that entry reports.
 *
 * The result is DEFINED over the same batches — the surviving files grouped by bitwise-equal z scale and z offset, groups in the
 * order of their first file, within a group the files in load order cut into batches of fewer than 2^32 points.  Per batch and block
 * of at most PCQ_ZMOMENTS_CELLS_MAX cells ONE pcq_scan_dev_zmoments_raster_batch (pcq.h) gives per cell four exact integers: the
 * u64 count cnt, the i64 sum of the stored z, and the two u64 halves lo and hi of the sum of their squares.  Per cell, over the
 * batches in that order, in f64 under the default rounding, every product and quotient rounded on its own (no fused multiply-add),
 * W, M and N starting at 0 and a batch with cnt == 0 skipped (host/zmoments_merge.h is the code):
 *
 *     Q  = hi * 2^32 + lo                              (unsigned 128-bit, exact)
 *     D  = cnt * Q - (int128)sum * sum                 (exact, >= 0, < 2^127)
 *     d  = (double)(uint64_t)(D >> 64) * 0x1p64 + (double)(uint64_t)D
 *     wb = offset * (double)cnt + scale * (double)(int64_t)sum
 *     m2 = (scale * scale) * (d / (double)cnt)
 *     if (N) { delta = wb / (double)cnt - W / (double)N;
 *              M += (delta * delta) * ((double)N * (double)cnt / (double)(N + cnt)); }
 *     M += m2;  W += wb;  N += cnt;
 *     count[c] = N;  zmean[c] = N ? W / (double)N : NaN;  zstd[c] = N ? sqrt(M / (double)N) : NaN
 *
 * The subtraction that would cancel in floats, n sum z^2 - (sum z)^2, is made in integers; against exact rational arithmetic the
 * formula was within 2.2 * 2^-53 * (|mean| + std) over lattices of scale 0.001 to 1 and offsets up to 3e6.
 *
 * Checked in this order before the dataset or a device is touched: a null r, bmin, count, zmean or zstd (PCQ_ERR_ARG "null
 * argument"); nx * ny == 0 (PCQ_OK, nothing written); more than PCQ_QUERY_RASTER_CELLS_MAX cells (PCQ_ERR_ARG "... cells ..."); a
 * cell_size that is not finite or not above 0 (PCQ_ERR_ARG "... cell_size ...").  Then: bmin[2] > zmax is PCQ_ERR_PANIC; a cell_size
 * that is no whole number of a scanned file's lattice steps, a scanned file whose z scale is not finite or not above 0, and a scanned
 * file of 2^32 points or more are PCQ_ERR_UNSUPPORTED.  On any failure count, zmean, zstd and *points_scanned are left as they were. */
int pcq_query_resident_bounds_zstd_raster(pcq_host_resident *r, const double bmin[3], double zmax, double cell_size, uint64_t nx,
                                          uint64_t ny, uint64_t *count, double *zmean, double *zstd, uint64_t *points_scanned);

#ifdef __cplusplus
}
#endif
#endif
