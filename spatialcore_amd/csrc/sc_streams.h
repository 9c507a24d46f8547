// The stream roles of a context and their placement on the runtime's hardware queues (host only; no HIP in this file,
// so that tests/stream_placement_checks.cpp compiles it with any C++ compiler).
//
// The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues PER STREAM PRIORITY (its own
// message: "maximum per priority is"), and kernels of streams that share a queue run one after the other.  A context
// whose eleven roles fit the limit creates plain streams (all on the normal level).  One that is held to fewer spreads
// its roles over the three priority levels, one group per level, so that 4 queues per level hold all of them.
#pragma once

enum StreamRole {
    SR_SCORE = 0,   // sc_ctx::stream: the context stream (scoring, and everything outside the pipelines)
    SR_FINALISE,    // stream_out: what leaves a pipeline beside it (Moran's finalise, result copies)
    SR_MOMENTS,     // stream_m: graph moments, neighbour-list copies
    SR_CHAIN,       // stream2: the generator's chain
    SR_EXPAND,      // pg.stream_px: verification + expansion of a scanned chunk
    SR_SWAP_A,      // stream3: Fisher-Yates swaps
    SR_SWAP_B,      // stream4: ... alternating with this one
    SR_PREP0,       // pg.stream_pg[0 .. 3]: the generator's preparation
    SR_PREP1,
    SR_PREP2,
    SR_PREP3,
    SR_COUNT
};

enum StreamGroup { SG_CONSUMER = 0, SG_CHAIN, SG_PREP, SG_COUNT };
enum StreamLevel { SL_NORMAL = 0, SL_HIGH, SL_LOW, SL_COUNT };   // (the null stream's rare synchronous copies land on normal)
enum StreamPlacement { SC_PLACE_NONE = -1, SC_PLACE_PLAIN = 0, SC_PLACE_SPREAD = 1 };

static const int SC_ROLE_GROUP[SR_COUNT] = {SG_CONSUMER, SG_CONSUMER, SG_CONSUMER, SG_CHAIN, SG_CHAIN, SG_CHAIN,
                                            SG_CHAIN,    SG_PREP,     SG_PREP,     SG_PREP,  SG_PREP};
// group -> level of the priority-spread placement (DESIGN.md 4.3 has the measurements behind the choice)
static const int SC_GROUP_LEVEL[SG_COUNT] = {SL_NORMAL, SL_LOW, SL_HIGH};

// The placement for `per_level_limit` hardware queues per priority level: SC_PLACE_PLAIN (every role on the normal level)
// when the roles fit the limit and plain streams have not been found to share queues already (plain_failed: a process
// whose runtime initialised with another limit than the environment shows now), else SC_PLACE_SPREAD when every group
// fits its level, else SC_PLACE_NONE (level_of_role is not written).  Groups must map to different levels.
static inline int sc_place_streams(int per_level_limit, bool plain_failed, const int *group_of_role, int n_roles,
                                   const int *level_of_group, int n_groups, int *level_of_role)
{
    if (per_level_limit < 1 || n_roles < 1 || n_groups < 1 || n_groups > SL_COUNT) return SC_PLACE_NONE;
    if (!plain_failed && per_level_limit >= n_roles) {
        for (int r = 0; r < n_roles; ++r) level_of_role[r] = SL_NORMAL;
        return SC_PLACE_PLAIN;
    }
    int members[SL_COUNT] = {0, 0, 0}, groups_on[SL_COUNT] = {0, 0, 0};
    for (int g = 0; g < n_groups; ++g) {
        if (level_of_group[g] < 0 || level_of_group[g] >= SL_COUNT) return SC_PLACE_NONE;
        if (++groups_on[level_of_group[g]] > 1) return SC_PLACE_NONE;
    }
    for (int r = 0; r < n_roles; ++r) {
        if (group_of_role[r] < 0 || group_of_role[r] >= n_groups) return SC_PLACE_NONE;
        if (++members[level_of_group[group_of_role[r]]] > per_level_limit) return SC_PLACE_NONE;
    }
    for (int r = 0; r < n_roles; ++r) level_of_role[r] = level_of_group[group_of_role[r]];
    return SC_PLACE_SPREAD;
}
