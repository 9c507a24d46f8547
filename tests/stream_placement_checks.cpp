// Stand-alone host program (its own main, no HIP, no device): sc_place_streams of spatialcore_amd/csrc/sc_streams.h,
// the pure function behind the context's stream placement, for every per-level limit from 1 to 32.
// Built and run by tests/test_gpu_00_stream_placement.py::test_placement_function_for_limits_1_to_32.
#include <stdio.h>

#include "../spatialcore_amd/csrc/sc_streams.h"

static int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++failures;                  \
            printf("FAILED %s: ", #cond); \
            printf(__VA_ARGS__);         \
            printf("\n");                \
        }                                \
    } while (0)

int main()
{
    // the roles and groups the issue of the placement names: 3 consumers, 4 of the chain's group, 4 preparation streams
    int in_group[SG_COUNT] = {0, 0, 0};
    for (int r = 0; r < SR_COUNT; ++r) ++in_group[SC_ROLE_GROUP[r]];
    CHECK(SR_COUNT == 11 && in_group[SG_CONSUMER] == 3 && in_group[SG_CHAIN] == 4 && in_group[SG_PREP] == 4, "role table");
    CHECK(SC_ROLE_GROUP[SR_SCORE] == SG_CONSUMER && SC_GROUP_LEVEL[SG_CONSUMER] == SL_NORMAL, "the context stream is a plain stream");
    for (int r = SR_PREP0; r <= SR_PREP3; ++r) CHECK(SC_ROLE_GROUP[r] == SG_PREP, "role %d", r);

    for (int limit = 1; limit <= 32; ++limit)
        for (int failed = 0; failed <= 1; ++failed) {
            int level[SR_COUNT];
            for (int &v : level) v = -7;
            const int place = sc_place_streams(limit, failed != 0, SC_ROLE_GROUP, SR_COUNT, SC_GROUP_LEVEL, SG_COUNT, level);
            if (limit >= SR_COUNT && !failed) {
                CHECK(place == SC_PLACE_PLAIN, "limit %d: placement %d", limit, place);
                for (int r = 0; r < SR_COUNT; ++r) CHECK(level[r] == SL_NORMAL, "limit %d role %d level %d", limit, r, level[r]);
            } else if (limit >= 4) {
                CHECK(place == SC_PLACE_SPREAD, "limit %d failed %d: placement %d", limit, failed, place);
                int on[SL_COUNT] = {0, 0, 0};
                for (int r = 0; r < SR_COUNT; ++r) {
                    CHECK(level[r] >= 0 && level[r] < SL_COUNT, "limit %d role %d level %d", limit, r, level[r]);
                    if (level[r] >= 0 && level[r] < SL_COUNT) ++on[level[r]];
                    CHECK(level[r] == SC_GROUP_LEVEL[SC_ROLE_GROUP[r]], "limit %d role %d", limit, r);
                    for (int q = 0; q < SR_COUNT; ++q)   // one group per level: same level <=> same group
                        CHECK((level[r] == level[q]) == (SC_ROLE_GROUP[r] == SC_ROLE_GROUP[q]), "limit %d roles %d %d", limit, r, q);
                }
                // the null stream's copies land on the normal level: one queue there stays free at a limit of 4
                CHECK(on[SL_NORMAL] == 3 && on[SL_HIGH] <= 4 && on[SL_LOW] <= 4 && on[SL_HIGH] + on[SL_LOW] == 8, "limit %d", limit);
            } else {
                CHECK(place == SC_PLACE_NONE, "limit %d: placement %d", limit, place);
                for (int r = 0; r < SR_COUNT; ++r) CHECK(level[r] == -7, "limit %d: level written", limit);
            }
        }

    // tables the function must refuse: two groups on one level, a level or a group out of range, nothing to place
    int level[SR_COUNT];
    const int two_on_one[SG_COUNT] = {SL_NORMAL, SL_HIGH, SL_HIGH}, bad_level[SG_COUNT] = {SL_NORMAL, SL_LOW, 3};
    CHECK(sc_place_streams(4, false, SC_ROLE_GROUP, SR_COUNT, two_on_one, SG_COUNT, level) == SC_PLACE_NONE, "two groups on one level");
    CHECK(sc_place_streams(4, false, SC_ROLE_GROUP, SR_COUNT, bad_level, SG_COUNT, level) == SC_PLACE_NONE, "level out of range");
    int bad_group[SR_COUNT];
    for (int r = 0; r < SR_COUNT; ++r) bad_group[r] = SC_ROLE_GROUP[r];
    bad_group[4] = SG_COUNT;
    CHECK(sc_place_streams(4, false, bad_group, SR_COUNT, SC_GROUP_LEVEL, SG_COUNT, level) == SC_PLACE_NONE, "group out of range");
    CHECK(sc_place_streams(0, false, SC_ROLE_GROUP, SR_COUNT, SC_GROUP_LEVEL, SG_COUNT, level) == SC_PLACE_NONE, "limit 0");
    CHECK(sc_place_streams(4, false, SC_ROLE_GROUP, 0, SC_GROUP_LEVEL, SG_COUNT, level) == SC_PLACE_NONE, "no roles");
    // the generator groups exchanged is a valid table too (the alternative DESIGN.md 4.3 measures)
    const int exchanged[SG_COUNT] = {SL_NORMAL, SL_HIGH, SL_LOW};
    CHECK(sc_place_streams(4, false, SC_ROLE_GROUP, SR_COUNT, exchanged, SG_COUNT, level) == SC_PLACE_SPREAD && level[SR_CHAIN] == SL_HIGH &&
              level[SR_PREP2] == SL_LOW && level[SR_FINALISE] == SL_NORMAL, "exchanged table");
    // five roles on a level of four do not fit, whatever the other levels hold
    int crowded[SR_COUNT];
    for (int r = 0; r < SR_COUNT; ++r) crowded[r] = SC_ROLE_GROUP[r];
    crowded[SR_MOMENTS] = SG_PREP;
    CHECK(sc_place_streams(4, false, crowded, SR_COUNT, SC_GROUP_LEVEL, SG_COUNT, level) == SC_PLACE_NONE, "five on one level");
    CHECK(sc_place_streams(5, false, crowded, SR_COUNT, SC_GROUP_LEVEL, SG_COUNT, level) == SC_PLACE_SPREAD, "five on a level of five");

    if (failures) return 1;
    printf("stream placement: ok\n");
    return 0;
}
