// polygon_plan_driver.cpp — host/polygon_plan.h against numbers worked out by hand, as a stand-alone program (built by
// tests/test_polygon_abi.py with ASan and UBSan; g++ alone, no HIP, no dataset).  Prints "ok <checks>".
#include <cmath>
#include <cstdio>
#include <limits>

#include "polygon_plan.h"

using namespace polygon_plan;

static int checks = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        checks++;                                                 \
        if (!(c)) {                                               \
            printf("line %d: %s\n", __LINE__, #c);                \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    const double one[2] = {1.0, 1.0}, zero[2] = {0.0, 0.0};
    Outline o;
    {  // ties to even at x.5 lattice steps, on both sides of zero: scale 2, so world 1, 3, 5 are 0.5, 1.5, 2.5 steps
        const double two[2] = {2.0, 2.0};
        const double xy[] = {1.0, -1.0, 3.0, -3.0, 5.0, -5.0, 7.0, -7.0};
        CHECK(to_lattice(4, xy, two, zero, &o) == PLAN_OK);
        const int32_t want[] = {0, 0, 2, -2, 2, -2, 4, -4};
        for (int i = 0; i < 8; i++) CHECK(o.xy[i] == want[i]);
        CHECK(o.lo[0] == 0 && o.hi[0] == 4 && o.lo[1] == -4 && o.hi[1] == 0);
    }
    {  // an anisotropic scale with an offset: (11.5 - 10) / 0.5 = 3, (-19 + 20) / 0.25 = 4; (9 - 10) / 0.5 = -2, (-20.75 + 20) / 0.25 = -3
        const double s[2] = {0.5, 0.25}, off[2] = {10.0, -20.0};
        const double xy[] = {11.5, -19.0, 9.0, -20.75, 10.0, -20.0};
        CHECK(to_lattice(3, xy, s, off, &o) == PLAN_OK);
        CHECK(o.xy[0] == 3 && o.xy[1] == 4 && o.xy[2] == -2 && o.xy[3] == -3 && o.xy[4] == 0 && o.xy[5] == 0);
        CHECK(o.lo[0] == -2 && o.hi[0] == 3 && o.lo[1] == -3 && o.hi[1] == 4);
    }
    {  // a vertex at INT32_MAX (INT32_MIN) is accepted, one step beyond is refused; `out` stays as it was on a refusal
        const double top[] = {2147483647.0, 0.0, 0.0, 5.0, 7.0, 9.0};
        CHECK(to_lattice(3, top, one, zero, &o) == PLAN_OK && o.hi[0] == 2147483647 && o.xy[0] == INT32_MAX);
        const double over[] = {2147483648.0, 0.0, 0.0, 5.0, 7.0, 9.0};
        CHECK(to_lattice(3, over, one, zero, &o) == PLAN_VERTEX && o.hi[0] == 2147483647);
        const double bottom[] = {-2147483648.0, 0.0, -1.0, 5.0, -7.0, 9.0};
        CHECK(to_lattice(3, bottom, one, zero, &o) == PLAN_OK && o.lo[0] == -2147483648LL && o.xy[0] == INT32_MIN);
        const double under[] = {-2147483649.0, 0.0, -1.0, 5.0, -7.0, 9.0};
        CHECK(to_lattice(3, under, one, zero, &o) == PLAN_VERTEX && o.lo[0] == -2147483648LL);
        const double up[] = {0.0, 2147483648.0, 1.0, 5.0, 7.0, 9.0};  // the same on y
        CHECK(to_lattice(3, up, one, zero, &o) == PLAN_VERTEX);
        // 2147483647.4 rounds down to INT32_MAX, 2147483647.5 is a tie that goes to the even 2147483648
        const double near[] = {2147483647.4, 0.0, 1.0, 5.0, 7.0, 9.0}, tie[] = {2147483647.5, 0.0, 1.0, 5.0, 7.0, 9.0};
        CHECK(to_lattice(3, near, one, zero, &o) == PLAN_OK && o.xy[0] == INT32_MAX);
        CHECK(to_lattice(3, tie, one, zero, &o) == PLAN_VERTEX);
    }
    {  // a span of 2^31 - 1 is accepted, 2^31 is refused, on either axis
        const double fits[] = {-1073741824.0, 0.0, 1073741823.0, 1.0, 0.0, 9.0};
        CHECK(to_lattice(3, fits, one, zero, &o) == PLAN_OK && o.hi[0] - o.lo[0] == 2147483647LL);
        const double wide[] = {-1073741824.0, 0.0, 1073741824.0, 1.0, 0.0, 9.0};
        CHECK(to_lattice(3, wide, one, zero, &o) == PLAN_SPAN);
        const double fits_y[] = {0.0, -1073741824.0, 1.0, 1073741823.0, 9.0, 0.0};
        CHECK(to_lattice(3, fits_y, one, zero, &o) == PLAN_OK && o.hi[1] - o.lo[1] == 2147483647LL);
        const double wide_y[] = {0.0, -1073741824.0, 1.0, 1073741824.0, 9.0, 0.0};
        CHECK(to_lattice(3, wide_y, one, zero, &o) == PLAN_SPAN);
        // the same outline in a lattice ten times as fine spans too much; in one ten times as coarse it fits
        const double tri[] = {-150000000.0, 0.0, 150000000.0, 1.0, 0.0, 9.0}, fine[2] = {0.1, 0.1}, coarse[2] = {10.0, 10.0};
        CHECK(to_lattice(3, tri, fine, zero, &o) == PLAN_SPAN);
        CHECK(to_lattice(3, tri, coarse, zero, &o) == PLAN_OK && o.lo[0] == -15000000 && o.hi[0] == 15000000);
    }
    {  // scale 0, negative, NaN and infinite are refused, on either axis, before any vertex is looked at
        const double xy[] = {0.0, 0.0, 1.0, 0.0, 0.0, 1.0};
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        for (double bad : {0.0, -0.0, -1.0, nan, inf, -inf})
            for (int a = 0; a < 2; a++) {
                double s[2] = {1.0, 1.0};
                s[a] = bad;
                CHECK(to_lattice(3, xy, s, zero, &o) == PLAN_SCALE);
            }
        const double tiny[2] = {5e-324, 1.0};  // above 0 and finite: the vertex decides
        CHECK(to_lattice(3, xy, tiny, zero, &o) == PLAN_VERTEX);
    }
    {  // the box is the rounded vertices': 0.6 -> 1 and 9.5 -> 10, where the truncating conversion of the world box gives 0 and 9
        const double xy[] = {0.6, 0.6, 9.5, 0.7, 4.0, 7.5};
        CHECK(to_lattice(3, xy, one, zero, &o) == PLAN_OK);
        CHECK(o.lo[0] == 1 && o.hi[0] == 10 && o.lo[1] == 1 && o.hi[1] == 8);
        CHECK((int64_t)0.6 == 0 && (int64_t)9.5 == 9 && (int64_t)7.5 == 7);
        double lo[2], hi[2];
        world_box(3, xy, lo, hi);
        CHECK(lo[0] == 0.6 && hi[0] == 9.5 && lo[1] == 0.6 && hi[1] == 7.5);
    }
    CHECK(refusal_text(PLAN_SCALE)[0] && refusal_text(PLAN_VERTEX)[0] && refusal_text(PLAN_SPAN)[0] && !refusal_text(PLAN_OK)[0]);
    printf("ok %d\n", checks);
    return 0;
}
