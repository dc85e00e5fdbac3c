// raster_div.h — the exact u32 / u32 floor division of the density raster (scan_raster.hip) by a divisor known on the host:
// a multiply-high by a precomputed magic and one fix-up.  Compiles as host code too (tests/native/raster_div_driver.cpp).
//
// For d >= 2 let m = floor(2^32 / d) = 2^32 / d - e with 0 <= e < 1.  For every a < 2^32: a m / 2^32 = a / d - a e / 2^32, and
// a e / 2^32 < 1, so q' = floor(a m / 2^32) is floor(a / d) or one below it.  Then r = a - q' d lies in [0, 2d) and is at most a,
// so it fits a u32 without wrapping, and the quotient is q' + (r >= d).  d = 1 takes m = 2^32 - 1: q' = a - 1 (0 for a = 0) and the
// same fix-up holds.  No 64-bit division and no loop where a point is binned; the magic's own division runs once per segment, on
// the host.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCQ_RASTER_HD __host__ __device__ __forceinline__
#else
#define PCQ_RASTER_HD inline
#endif

// the magic of divisor d (1 .. 2^32 - 1; 0 has no quotient: the entry refuses it where points could meet it)
inline uint32_t raster_div_magic(uint32_t d) { return d <= 1 ? 0xffffffffu : (uint32_t)(0x100000000ull / d); }

// floor(a / d), m = raster_div_magic(d)
PCQ_RASTER_HD uint32_t raster_div(uint32_t a, uint32_t d, uint32_t m) {
    const uint32_t q = (uint32_t)(((uint64_t)a * m) >> 32);  // (v_mul_hi_u32)
    const uint32_t r = a - q * d;
    return q + (r >= d ? 1u : 0u);
}
