// The division of the density raster (adhoc-queries-pointclouds_amd/csrc/raster_div.h) against `/`, as host code: divisors 1, 2,
// 3, 5, 7, 641, 65537, 2^24, 2^31 - 1, 2^31, 2^31 + 1 and 2^32 - 1, and for every quotient q below 8192 the numerators q d - 1, q d,
// q d + 1 and (q + 1) d - 1 where they are below 2^32, and 2^32 - 1; then 10^6 random pairs.  Built with -fsanitize=undefined by
// tests/test_raster_abi.py; prints "ok <divisions checked>".
#include <cstdint>
#include <cstdio>

#include "raster_div.h"

static uint64_t checked = 0;

static bool check(uint32_t a, uint32_t d) {
    checked++;
    const uint32_t got = raster_div(a, d, raster_div_magic(d));
    if (got == a / d) return true;
    printf("%u / %u: got %u, want %u\n", a, d, got, a / d);
    return false;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main() {
    const uint32_t divisors[] = {1u, 2u, 3u, 5u, 7u, 641u, 65537u, 1u << 24, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xffffffffu};
    for (uint32_t d : divisors) {
        for (uint64_t q = 0; q < 8192; q++) {
            const int64_t cand[4] = {(int64_t)(q * d) - 1, (int64_t)(q * d), (int64_t)(q * d) + 1, (int64_t)((q + 1) * d) - 1};
            for (int64_t a : cand)
                if (a >= 0 && a <= 0xffffffffll && !check((uint32_t)a, d)) return 1;
        }
        if (!check(0xffffffffu, d)) return 1;
    }
    for (int i = 0; i < 1000000; i++) {
        const uint64_t r = rng();
        uint32_t a = (uint32_t)r, d = (uint32_t)(r >> 32);
        if (i % 4 == 1) d >>= rng() % 32;  // small divisors and large quotients as well
        if (i % 4 == 2) a >>= rng() % 32;
        if (d == 0) d = 1;
        if (!check(a, d)) return 1;
    }
    printf("ok %llu\n", (unsigned long long)checked);
    return 0;
}
