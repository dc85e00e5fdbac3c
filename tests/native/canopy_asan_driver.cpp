// Memory-safety driver for the host entry of the canopy-height raster (no GPU call is made):
// pcq_query_resident_bounds_canopy_raster makes its argument checks — null arguments (the two class sets among them; height and
// points_scanned may be null), nx * ny == 0, too many cells, a cell size that is not finite or not above 0 — before it touches a
// dataset or a device, and leaves the caller's words alone, whatever the sets hold.  Built with -fsanitize=address,undefined by
// tests/test_canopy_abi.py; prints "ok <refusals> <empty rasters>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "pcq.h"
#include "pcq_query_canopy.h"

int main() {
    static_assert(PCQ_ZRANGE_CLASSES_CELLS_MAX == 4096 && PCQ_QUERY_RASTER_CELLS_MAX == (1u << 20), "the two limits");
    const double lo[3] = {0, 0, 0};
    const uint32_t ground[8] = {1u << 2, 0, 0, 0, 0, 0, 0, 0}, none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t surface[8];
    for (uint32_t &w : surface) w = ~0u;
    surface[0] &= ~(1u << 7 | 1u << 18);
    double zg[64], zs[64], h[64];
    uint64_t scanned = 15;
    for (int c = 0; c < 64; c++) zg[c] = -3.25 - c, zs[c] = 1000.5 + 7 * c, h[c] = 0.125 * c;
    pcq_host_resident *dummy = reinterpret_cast<pcq_host_resident *>(uintptr_t(1));  // never dereferenced: a check refuses first
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    int refusals = 0, empties = 0;
    const uint32_t *pairs[][2] = {{ground, surface}, {surface, ground}, {none, surface}, {ground, none}, {none, none}};
    for (const auto &pair : pairs) {
        const uint32_t *g = pair[0], *s = pair[1];
        const struct {
            pcq_host_resident *r;
            const double *bmin;
            double cell;
            uint64_t nx, ny;
            const uint32_t *g, *s;
            double *zg, *zs;
            const char *text;
        } bad[] = {{nullptr, lo, 1.0, 8, 8, g, s, zg, zs, "null argument"},
                   {dummy, nullptr, 1.0, 8, 8, g, s, zg, zs, "null argument"},
                   {dummy, lo, 1.0, 8, 8, nullptr, s, zg, zs, "null argument"},
                   {dummy, lo, 1.0, 8, 8, g, nullptr, zg, zs, "null argument"},
                   {dummy, lo, 1.0, 8, 8, g, s, nullptr, zs, "null argument"},
                   {dummy, lo, 1.0, 8, 8, g, s, zg, nullptr, "null argument"},
                   {nullptr, nullptr, 1.0, 0, 0, nullptr, nullptr, nullptr, nullptr, "null argument"},
                   {dummy, lo, nan, 1ull << 32, 1ull << 32, nullptr, s, zg, zs, "null argument"},  // a null set comes before the cells
                   {dummy, lo, nan, 1ull << 32, 1ull << 32, g, nullptr, zg, zs, "null argument"},
                   {dummy, lo, 1.0, 1025, 1024, g, s, zg, zs, "cells"},
                   {dummy, lo, 1.0, (1u << 20) + 1, 1, g, s, zg, zs, "cells"},
                   {dummy, lo, 1.0, 1, (1u << 20) + 1, g, s, zg, zs, "cells"},
                   {dummy, lo, 1.0, 1ull << 32, 1ull << 32, g, s, zg, zs, "cells"},
                   {dummy, lo, nan, ~0ull, ~0ull, g, s, zg, zs, "cells"},                          // the cells before the cell size
                   {dummy, lo, 0.0, 8, 8, g, s, zg, zs, "cell_size"},
                   {dummy, lo, -1.0, 8, 8, g, s, zg, zs, "cell_size"},
                   {dummy, lo, inf, 8, 8, g, s, zg, zs, "cell_size"},
                   {dummy, lo, -inf, 8, 8, g, s, zg, zs, "cell_size"},
                   {dummy, lo, nan, 8, 8, g, s, zg, zs, "cell_size"}};
        for (const auto &a : bad) {
            for (uint64_t *ps : {&scanned, (uint64_t *)nullptr}) {
                for (double *ph : {h, (double *)nullptr}) {
                    const int rc = pcq_query_resident_bounds_canopy_raster(a.r, a.bmin, 10.0, a.cell, a.nx, a.ny, a.g, a.s, a.zg, a.zs, ph, ps);
                    if (rc != PCQ_ERR_ARG || !strstr(pcq_query_last_error(), a.text)) {
                        printf("rc %d: %s (wanted '%s')\n", rc, pcq_query_last_error(), a.text);
                        return 1;
                    }
                    refusals++;
                }
            }
        }
        // nx * ny == 0: PCQ_OK with nothing written, whatever the cell size
        const uint64_t zero[][2] = {{0, 8}, {8, 0}, {0, 0}, {0, ~0ull}};
        for (const auto &z : zero) {
            if (pcq_query_resident_bounds_canopy_raster(dummy, lo, 10.0, nan, z[0], z[1], g, s, zg, zs, h, &scanned) != PCQ_OK) return 4;
            empties++;
        }
    }
    for (int c = 0; c < 64; c++)
        if (zg[c] != -3.25 - c || zs[c] != 1000.5 + 7 * c || h[c] != 0.125 * c) return 2;
    if (scanned != 15) return 3;
    printf("ok %d %d\n", refusals, empties);
    return 0;
}
