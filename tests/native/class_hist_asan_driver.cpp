// Memory-safety driver for the host entry of the class histogram of a box (no GPU call is made):
// pcq_query_resident_count_bounds_by_class refuses every null argument before it touches a dataset or a device, and leaves the
// caller's 256 words alone.  Built with -fsanitize=address,undefined by tests/test_class_hist_abi.py; prints "ok <refusals>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "pcq.h"
#include "pcq_query.h"

int main() {
    static_assert(PCQ_CLASS_BINS == 256, "one bin per class byte");
    const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    uint64_t hist[PCQ_CLASS_BINS], scanned = 15;
    for (int c = 0; c < PCQ_CLASS_BINS; c++) hist[c] = 1000u + 7u * (unsigned)c;
    pcq_host_resident *dummy = reinterpret_cast<pcq_host_resident *>(uintptr_t(1));  // never dereferenced: another argument is null
    int refusals = 0;
    const struct {
        pcq_host_resident *r;
        const double *bmin, *bmax;
        uint64_t *hist;
    } calls[] = {{nullptr, lo, hi, hist}, {dummy, nullptr, hi, hist}, {dummy, lo, nullptr, hist}, {dummy, lo, hi, nullptr},
                 {nullptr, nullptr, nullptr, nullptr}};
    for (const auto &a : calls) {
        for (uint64_t *ps : {&scanned, (uint64_t *)nullptr}) {
            const int rc = pcq_query_resident_count_bounds_by_class(a.r, a.bmin, a.bmax, a.hist, ps);
            if (rc != PCQ_ERR_ARG || !strstr(pcq_query_last_error(), "null argument")) {
                printf("rc %d: %s\n", rc, pcq_query_last_error());
                return 1;
            }
            refusals++;
        }
    }
    for (int c = 0; c < PCQ_CLASS_BINS; c++)
        if (hist[c] != 1000u + 7u * (unsigned)c) return 2;
    if (scanned != 15) return 3;
    printf("ok %d\n", refusals);
    return 0;
}
