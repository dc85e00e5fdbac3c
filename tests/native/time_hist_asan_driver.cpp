// Memory-safety driver for the host entry of the time histogram of a box (no GPU call is made):
// pcq_query_resident_count_bounds_by_time refuses a null argument, a NaN edge and decreasing edges, and accepts nbins == 0, before it
// touches a dataset or a device, and leaves the caller's words alone.  The edge tables are heap blocks of exactly nbins + 1
// doubles, so a read past the last edge is an ASan report.  Built with -fsanitize=address,undefined by
// tests/test_time_hist_abi.py; prints "ok <refusals> <accepted>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "pcq.h"
#include "pcq_query.h"

int main() {
    static_assert(PCQ_TIME_BINS_MAX >= 512, "the bins of one launch");
    const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    const size_t words = PCQ_TIME_BINS_MAX + 8;
    std::vector<uint64_t> hist(words);
    uint64_t scanned = 15;
    for (size_t c = 0; c < words; c++) hist[c] = 1000u + 7u * (unsigned)c;
    pcq_host_resident *dummy = reinterpret_cast<pcq_host_resident *>(uintptr_t(1));  // never dereferenced: the call ends before it
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::vector<double> good = {1.0, 2.0, 3.0, 4.0};
    int refusals = 0, accepted = 0;
    const struct {
        pcq_host_resident *r;
        const double *bmin, *bmax, *edges;
        uint64_t *hist;
    } nulls[] = {{nullptr, lo, hi, good.data(), hist.data()}, {dummy, nullptr, hi, good.data(), hist.data()},
                 {dummy, lo, nullptr, good.data(), hist.data()}, {dummy, lo, hi, nullptr, hist.data()},
                 {dummy, lo, hi, good.data(), nullptr},          {nullptr, nullptr, nullptr, nullptr, nullptr}};
    for (const auto &a : nulls) {
        for (uint64_t *ps : {&scanned, (uint64_t *)nullptr}) {
            for (size_t nbins : {(size_t)3, (size_t)0}) {  // (a null argument comes before nbins == 0)
                const int rc = pcq_query_resident_count_bounds_by_time(a.r, a.bmin, a.bmax, a.edges, nbins, a.hist, ps);
                if (rc != PCQ_ERR_ARG || !strstr(pcq_query_last_error(), "null argument")) {
                    printf("rc %d: %s\n", rc, pcq_query_last_error());
                    return 1;
                }
                refusals++;
            }
        }
    }
    // nbins == 0: PCQ_OK, nothing written, no edge read (the table is one double long)
    std::vector<double> one = {nan};
    if (pcq_query_resident_count_bounds_by_time(dummy, lo, hi, one.data(), 0, hist.data(), &scanned) != PCQ_OK) return 4;
    accepted++;
    // bad edges: a NaN first, in the middle and last; a decrease at the front and at the back; +inf then a finite value; many bins
    std::vector<std::vector<double>> bad = {{nan, 2.0, 3.0},      {1.0, nan, 3.0}, {1.0, 2.0, nan}, {2.0, 1.0, 3.0},
                                            {1.0, 3.0, 2.0},      {-inf, inf, 0.0}, {0.0, -0.5},    {nan, nan}};
    std::vector<double> many(PCQ_TIME_BINS_MAX + 4);
    for (size_t i = 0; i < many.size(); i++) many[i] = (double)i;
    many[many.size() - 1] = 5.0;  // the decrease lies in the second group of bins
    bad.push_back(many);
    for (const auto &e : bad) {
        const int rc = pcq_query_resident_count_bounds_by_time(dummy, lo, hi, e.data(), e.size() - 1, hist.data(), &scanned);
        if (rc != PCQ_ERR_ARG || !strstr(pcq_query_last_error(), "edge")) {
            printf("rc %d: %s\n", rc, pcq_query_last_error());
            return 5;
        }
        refusals++;
    }
    for (size_t c = 0; c < words; c++)
        if (hist[c] != 1000u + 7u * (unsigned)c) return 2;
    if (scanned != 15) return 3;
    printf("ok %d %d\n", refusals, accepted);
    return 0;
}
