// zmoments_merge_driver.cpp — host/zmoments_merge.h as a stand-alone program (built by tests/test_zmoments_merge.py with ASan and
// UBSan and -ffp-contract=off; g++ alone, no HIP, no dataset).  argv[1] is a text file of cells: a line "<batches>" and then per
// batch a line "<scale> <offset> <cnt> <sum> <lo> <hi>", scale and offset as hexadecimal floats (so that no decimal conversion stands
// between the test's f64 and this program's), the four words in decimal.  Per cell it prints "<count> <zmean> <zstd>", the two f64
// as the 16 hex digits of their bits.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "zmoments_merge.h"

static uint64_t bits(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned long long nb;
    while (fscanf(f, "%llu", &nb) == 1) {
        zmoments_merge::Cell c;
        for (unsigned long long b = 0; b < nb; b++) {
            char scale[64], offset[64];
            unsigned long long cnt, lo, hi;
            long long sum;
            if (fscanf(f, "%63s %63s %llu %lld %llu %llu", scale, offset, &cnt, &sum, &lo, &hi) != 6) {
                fclose(f);
                return 3;
            }
            zmoments_merge::add(c, strtod(scale, nullptr), strtod(offset, nullptr), cnt, sum, lo, hi);
        }
        printf("%" PRIu64 " %016" PRIx64 " %016" PRIx64 "\n", c.N, bits(zmoments_merge::zmean(c)), bits(zmoments_merge::zstd(c)));
    }
    fclose(f);
    return 0;
}
