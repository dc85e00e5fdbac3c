/*
 * pcq_query_canopy.h — the canopy-height raster of a box on a resident dataset: the lowest ground, the highest surface and their
 * difference, cell by cell, beside the entries of pcq_query.h, pcq_query_stats.h, pcq_query_classes.h and pcq_query_moments.h
 * (libpcq_query.so).
 *
 * Why a header of its own: tests hold each of those four headers to exactly the declarations it had when this entry was added, and
 * a change that adds an entry leaves existing tests as they are.  So the new entry is declared here, with a signature table of its
 * own (query_binding.canopy_sig).  A later change that is free to touch those tests may fold this header back, behind
 * pcq_query_resident_bounds_zrange_raster.
 */
#ifndef PCQ_QUERY_CANOPY_H
#define PCQ_QUERY_CANOPY_H

#include "pcq_query.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How high above the ground is this box, cell by cell: the canopy-height (or building-height) model.  ground_set and surface_set
 * are eight words each: class c is in a set when bit (c & 31) of its word c >> 5 is set — the whole class byte, as the LAST class
 * search compares it.  A usual pair is ground {2} and surface "every class but 7 and 18" (low and high noise).
 *
 * The raster, the box, the per-file prologue and the order of the argument checks are those of
 * pcq_query_resident_bounds_zrange_raster (pcq_query.h): nx x ny cells of cell_size world units from (bmin[0], bmin[1]), row-major
 * with y upward, the points with z in [bmin[2], zmax]; a stored point (X, Y, Z) lies in the cell c = cy * nx + cx that entry
 * assigns it to.
 *
 * The result is DEFINED as follows.  The surviving files are scanned in groups of one z lattice (bitwise-equal scale[2] and
 * offset[2], in the order of their first file).  Per group, two i32 words per cell start at INT32_MAX and INT32_MIN; per block of
 * at most PCQ_ZRANGE_CLASSES_CELLS_MAX cells (pcq.h) ONE pcq_scan_dev_zrange_raster_batch_classes over the positions and class blocks
 * of the group's files folds into them the minimum of Z over the cell's points whose class byte is in ground_set and the maximum
 * of Z over the cell's points whose class byte is in surface_set (signed i32).  A word that left its sentinel becomes the world
 * value ((double)Z * scale[2]) + offset[2]; the groups are merged with < on the minima and > on the maxima.  Then
 *
 *     zground[c]  is the merged image of the minima: NaN exactly where every group's word stayed INT32_MAX;
 *     zsurface[c] is the merged image of the maxima: NaN exactly where every group's word stayed INT32_MIN;
 *     height[c]   = zsurface[c] - zground[c] in f64: NaN where either is NaN.  (height may be null: not wanted.)
 *
 * The sentinel rule, deliberate: the two arrays are independent here, so "no point" cannot be told from the pair as the unfiltered
 * entry tells it (minimum above maximum).  A ground point stored at exactly Z = INT32_MAX therefore reads as no point, and so does
 * a surface point stored at exactly Z = INT32_MIN.  With both sets full (all 256 bits) zground and zsurface equal zlo and zhi of
 * pcq_query_resident_bounds_zrange_raster bit for bit on any dataset without those two stored values.  With both sets empty every
 * output is NaN and nothing is launched; every refusal below is still made.  With one set empty its array is NaN, and so is height.
 * *points_scanned (may be null) is what the unfiltered entry reports: the points of the files the box reaches, whatever their class.
 *
 * Checked in this order before the dataset or a device is touched: a null r, bmin, ground_set, surface_set, zground or zsurface
 * (PCQ_ERR_ARG "null argument"); nx * ny == 0 (PCQ_OK, nothing written); more than PCQ_QUERY_RASTER_CELLS_MAX cells (PCQ_ERR_ARG
 * "... cells ..."); a cell_size that is not finite or not above 0 (PCQ_ERR_ARG "... cell_size ...").  Then: bmin[2] > zmax is
 * PCQ_ERR_PANIC; a cell_size that is no whole number of a scanned file's lattice steps and a scanned file whose z scale is not
 * finite or not above 0 are PCQ_ERR_UNSUPPORTED.  On any failure zground, zsurface, height and *points_scanned are left as they
 * were. */
int pcq_query_resident_bounds_canopy_raster(pcq_host_resident *r, const double bmin[3], double zmax, double cell_size, uint64_t nx,
                                            uint64_t ny, const uint32_t ground_set[8], const uint32_t surface_set[8], double *zground,
                                            double *zsurface, double *height, uint64_t *points_scanned);

#ifdef __cplusplus
}
#endif
#endif
