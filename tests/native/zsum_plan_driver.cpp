// zsum_plan_driver.cpp — host/zsum_plan.h with small limits passed as the parameter, as a stand-alone program (built by
// tests/test_zsum_abi.py with ASan and UBSan; g++ alone, no HIP, no dataset).  Every accepted cut is checked for the three
// properties the launches rest on — every batch's total below the limit, file order kept, no file lost — and then against the
// batches worked out by hand.  Prints "ok <checks>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "zsum_plan.h"

using namespace zsum_plan;

static int checks = 0;
#define CHECK(c)                                   \
    do {                                           \
        checks++;                                  \
        if (!(c)) {                                \
            printf("line %d: %s\n", __LINE__, #c); \
            return 1;                              \
        }                                          \
    } while (0)

// consecutive, non-empty batches that cover 0 .. n - 1 in order, totals right and below the limit
static bool sound(const std::vector<uint64_t> &points, uint64_t limit, const std::vector<Batch> &b) {
    size_t at = 0;
    for (const Batch &x : b) {
        if (x.begin != at || x.end <= x.begin || x.end > points.size()) return false;
        uint64_t total = 0;
        for (size_t i = x.begin; i < x.end; i++) total += points[i];
        if (total != x.points || !(total < limit)) return false;
        at = x.end;
    }
    return at == points.size();
}

static bool is(const std::vector<Batch> &b, std::vector<std::vector<size_t>> want) {
    if (b.size() != want.size()) return false;
    for (size_t k = 0; k < b.size(); k++)
        if (b[k].begin != want[k][0] || b[k].end != want[k][1]) return false;
    return true;
}

int main() {
    static_assert(POINTS_LIMIT == (1ull << 32), "the product's limit");
    std::vector<Batch> b;
    size_t refused = 99;
    {  // an empty list: no batch
        b.push_back({7, 8, 9});
        CHECK(cut({}, 10, &b, &refused) && b.empty() && refused == 99);
    }
    {  // one file, and one file of no points
        const std::vector<uint64_t> p = {5}, z = {0};
        CHECK(cut(p, 10, &b, &refused) && sound(p, 10, b) && is(b, {{0, 1}}) && b[0].points == 5);
        CHECK(cut(z, 10, &b, &refused) && sound(z, 10, b) && is(b, {{0, 1}}) && b[0].points == 0);
        CHECK(cut(z, 1, &b, &refused) && sound(z, 1, b) && is(b, {{0, 1}}));
    }
    {  // a total exactly at limit - 1 stays one batch; exactly at the limit is cut before the file that reaches it
        const std::vector<uint64_t> under = {4, 3, 2}, at = {4, 3, 3}, at2 = {4, 3, 2, 1};
        CHECK(cut(under, 10, &b, &refused) && sound(under, 10, b) && is(b, {{0, 3}}) && b[0].points == 9);
        CHECK(cut(at, 10, &b, &refused) && sound(at, 10, b) && is(b, {{0, 2}, {2, 3}}) && b[0].points == 7 && b[1].points == 3);
        CHECK(cut(at2, 10, &b, &refused) && sound(at2, 10, b) && is(b, {{0, 3}, {3, 4}}));
    }
    {  // a file that alone reaches the limit is refused with its position, and `out` stays as it was; limit - 1 alone is served
        const std::vector<uint64_t> p = {1, 2, 10, 3}, q = {1, 2, 11, 3}, r = {1, 2, 9, 3}, first = {10};
        CHECK(cut(r, 10, &b, &refused) && sound(r, 10, b) && is(b, {{0, 2}, {2, 3}, {3, 4}}));
        const std::vector<Batch> before = b;
        refused = 99;
        CHECK(!cut(p, 10, &b, &refused) && refused == 2 && b.size() == before.size() && b[1].begin == before[1].begin);
        CHECK(!cut(q, 10, &b, &refused) && refused == 2);
        CHECK(!cut(first, 10, &b, &refused) && refused == 0);
        CHECK(!cut(first, 10, &b, nullptr));
        CHECK(!cut({0}, 0, &b, &refused) && refused == 0);  // (below 0 is nothing)
    }
    {  // many files: greedy in order, files of no points join the open batch
        std::vector<uint64_t> p;
        for (int i = 0; i < 1000; i++) p.push_back((uint64_t)(i * 7 % 13));  // 0 .. 12
        for (uint64_t limit : {13ull, 14ull, 25ull, 100ull, 6001ull}) {
            CHECK(cut(p, limit, &b, &refused) && sound(p, limit, b));
            for (size_t k = 0; k + 1 < b.size(); k++) CHECK(b[k].points + p[b[k + 1].begin] >= limit);  // (greedy: the next file did not fit)
        }
        uint64_t all = 0;
        for (uint64_t v : p) all += v;
        CHECK(cut(p, all + 1, &b, &refused) && b.size() == 1 && b[0].points == all);
        CHECK(cut(p, all, &b, &refused) && b.size() == 2);
        CHECK(!cut(p, 12, &b, &refused) && p[refused] == 12);
        const std::vector<uint64_t> q = {0, 0, 6, 0, 5, 0, 0, 4, 0};
        CHECK(cut(q, 10, &b, &refused) && sound(q, 10, b) && is(b, {{0, 4}, {4, 9}}));
    }
    {  // the product's limit with totals that would overflow a u64 if they were formed
        const uint64_t big = POINTS_LIMIT - 1;
        const std::vector<uint64_t> p = {big, 0, 1, big, big}, huge = {~0ull - 1, ~0ull - 1, 3};
        CHECK(cut(p, POINTS_LIMIT, &b, &refused) && sound(p, POINTS_LIMIT, b) && is(b, {{0, 2}, {2, 3}, {3, 4}, {4, 5}}));
        CHECK(cut(huge, ~0ull, &b, &refused) && sound(huge, ~0ull, b) && is(b, {{0, 1}, {1, 2}, {2, 3}}));
        const std::vector<uint64_t> over = {5, POINTS_LIMIT};
        CHECK(!cut(over, POINTS_LIMIT, &b, &refused) && refused == 1);
    }
    printf("ok %d\n", checks);
    return 0;
}
