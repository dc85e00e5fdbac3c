// zmoments_merge.h — the one place where the height-spread raster (ResidentDataset::bounds_zstd_raster) makes floats: a cell's exact
// integer words of every batch — the u64 count cnt, the i64 sum of the stored z and the two u64 halves lo and hi of the sum of their
// squares (pcq.h: pcq_scan_dev_zmoments_raster_batch), with the z scale and z offset of the batch's lattice — merged into the count,
// the mean world z and the POPULATION standard deviation of the world z.  Pure host arithmetic without a HIP include and without the
// dataset type: tests/native/zmoments_merge_driver.cpp compiles it with g++ alone, and tests/_zmoments.py restates it in python.
//
// Per cell, over the batches in the mean-height raster's order, in f64 under the default rounding, every product and quotient a named
// value, no fused multiply-add (host/Makefile compiles with -ffp-contract=off).  W, M and N start at 0; a batch with cnt == 0 is
// skipped:
//
//     Q  = hi * 2^32 + lo                              (unsigned 128-bit, exact: the sum of z^2)
//     D  = cnt * Q - (int128)sum * sum                 (exact, >= 0, < 2^127: cnt^2 times the variance in lattice steps)
//     d  = (double)(uint64_t)(D >> 64) * 0x1p64 + (double)(uint64_t)D
//     wb = offset * (double)cnt + scale * (double)(int64_t)sum         (the mean-height raster's term, unchanged)
//     m2 = (scale * scale) * (d / (double)cnt)
//     if (N) { delta = wb / (double)cnt - W / (double)N;
//              M += (delta * delta) * ((double)N * (double)cnt / (double)(N + cnt)); }
//     M += m2;  W += wb;  N += cnt;
//     count = N;  zmean = N ? W / (double)N : NaN;  zstd = N ? sqrt(M / (double)N) : NaN
//
// Nothing cancels in floats: the one subtraction that could, n sum z^2 - (sum z)^2, is made in integers.  W and N are the mean-height
// raster's, so count and zmean are bit for bit what pcq_query_resident_bounds_zmean_raster returns.  M is the sum of squared
// deviations from the mean: a batch brings its own (m2) and the batches' means are joined by the pairwise update of Chan, Golub and
// LeVeque.  The requirements on a batch: cnt < 2^32 and the four words those of cnt points of i32 heights, which makes D fit.
#pragma once

#include <cmath>
#include <cstdint>

namespace zmoments_merge {

struct Cell {
    double W = 0.0;  // sum of the world z
    double M = 0.0;  // sum of the squared deviations of the world z from their mean
    uint64_t N = 0;  // points
};

// One batch's words of a cell into the cell.
inline void add(Cell &c, double scale, double offset, uint64_t cnt, int64_t sum, uint64_t lo, uint64_t hi) {
    if (cnt == 0) return;
    const unsigned __int128 Q = ((unsigned __int128)hi << 32) + lo;
    const unsigned __int128 S = (unsigned __int128)((__int128)sum * sum);
    const unsigned __int128 D = (unsigned __int128)cnt * Q - S;
    const double n = (double)cnt;
    const double dh = (double)(uint64_t)(D >> 64) * 0x1p64, dl = (double)(uint64_t)D;
    const double d = dh + dl;
    const double a = offset * n, b = scale * (double)sum;
    const double wb = a + b;
    const double ss = scale * scale, q = d / n;
    const double m2 = ss * q;
    if (c.N) {
        const double mb = wb / n, mw = c.W / (double)c.N;
        const double delta = mb - mw;
        const double dd = delta * delta, nn = (double)c.N * n;
        const double f = nn / (double)(c.N + cnt);
        const double t = dd * f;
        c.M += t;
    }
    c.M += m2;
    c.W += wb;
    c.N += cnt;
}

inline double zmean(const Cell &c) { return c.N ? c.W / (double)c.N : std::nan(""); }
inline double zstd(const Cell &c) {
    if (!c.N) return std::nan("");
    const double v = c.M / (double)c.N;
    return std::sqrt(v);
}

}  // namespace zmoments_merge
