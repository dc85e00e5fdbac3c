// Memory-safety driver for the host entry of the mean-height raster of a set of classes (no GPU call is made):
// pcq_query_resident_bounds_zmean_raster_classes makes its argument checks — null arguments (the class set among them), nx * ny == 0,
// too many cells, a cell size that is not finite or not above 0 — before it touches a dataset or a device, and leaves the caller's
// words alone, whatever the set holds.  Built with -fsanitize=address,undefined by tests/test_zsum_classes_abi.py; prints
// "ok <refusals> <empty rasters>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "pcq.h"
#include "pcq_query_classes.h"

int main() {
    static_assert(PCQ_ZSUM_CELLS_MAX == 2048 && PCQ_QUERY_RASTER_CELLS_MAX == (1u << 20), "the two limits");
    const double lo[3] = {0, 0, 0};
    const uint32_t ground[8] = {1u << 2 | 1u << 9, 0, 0, 0, 0, 0, 0, 0}, none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t all[8];
    for (uint32_t &w : all) w = ~0u;
    uint64_t count[64];
    double zmean[64];
    uint64_t scanned = 15;
    for (int c = 0; c < 64; c++) count[c] = 1000 + 7 * c, zmean[c] = -3.25 - c;
    pcq_host_resident *dummy = reinterpret_cast<pcq_host_resident *>(uintptr_t(1));  // never dereferenced: a check refuses first
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    int refusals = 0, empties = 0;
    for (const uint32_t *set : {ground, none, (const uint32_t *)all}) {
        const struct {
            pcq_host_resident *r;
            const double *bmin;
            double cell;
            uint64_t nx, ny;
            const uint32_t *set;
            uint64_t *count;
            double *zmean;
            const char *text;
        } bad[] = {{nullptr, lo, 1.0, 8, 8, set, count, zmean, "null argument"},
                   {dummy, nullptr, 1.0, 8, 8, set, count, zmean, "null argument"},
                   {dummy, lo, 1.0, 8, 8, nullptr, count, zmean, "null argument"},
                   {dummy, lo, 1.0, 8, 8, set, nullptr, zmean, "null argument"},
                   {dummy, lo, 1.0, 8, 8, set, count, nullptr, "null argument"},
                   {nullptr, nullptr, 1.0, 0, 0, nullptr, nullptr, nullptr, "null argument"},
                   {dummy, lo, nan, 1ull << 32, 1ull << 32, nullptr, count, zmean, "null argument"},  // the null set comes before the cells
                   {dummy, lo, 1.0, 1025, 1024, set, count, zmean, "cells"},
                   {dummy, lo, 1.0, (1u << 20) + 1, 1, set, count, zmean, "cells"},
                   {dummy, lo, 1.0, 1, (1u << 20) + 1, set, count, zmean, "cells"},
                   {dummy, lo, 1.0, 1ull << 32, 1ull << 32, set, count, zmean, "cells"},
                   {dummy, lo, nan, ~0ull, ~0ull, set, count, zmean, "cells"},                         // the cells before the cell size
                   {dummy, lo, 0.0, 8, 8, set, count, zmean, "cell_size"},
                   {dummy, lo, -1.0, 8, 8, set, count, zmean, "cell_size"},
                   {dummy, lo, inf, 8, 8, set, count, zmean, "cell_size"},
                   {dummy, lo, -inf, 8, 8, set, count, zmean, "cell_size"},
                   {dummy, lo, nan, 8, 8, set, count, zmean, "cell_size"}};
        for (const auto &a : bad) {
            for (uint64_t *ps : {&scanned, (uint64_t *)nullptr}) {
                const int rc = pcq_query_resident_bounds_zmean_raster_classes(a.r, a.bmin, 10.0, a.cell, a.nx, a.ny, a.set, a.count, a.zmean, ps);
                if (rc != PCQ_ERR_ARG || !strstr(pcq_query_last_error(), a.text)) {
                    printf("rc %d: %s (wanted '%s')\n", rc, pcq_query_last_error(), a.text);
                    return 1;
                }
                refusals++;
            }
        }
        // nx * ny == 0: PCQ_OK with nothing written, whatever the cell size
        const uint64_t zero[][2] = {{0, 8}, {8, 0}, {0, 0}, {0, ~0ull}};
        for (const auto &z : zero) {
            if (pcq_query_resident_bounds_zmean_raster_classes(dummy, lo, 10.0, nan, z[0], z[1], set, count, zmean, &scanned) != PCQ_OK) return 4;
            empties++;
        }
    }
    for (int c = 0; c < 64; c++)
        if (count[c] != (uint64_t)(1000 + 7 * c) || zmean[c] != -3.25 - c) return 2;
    if (scanned != 15) return 3;
    printf("ok %d %d\n", refusals, empties);
    return 0;
}
