// Device-wide radix sort and exclusive scan (hipcub's size query, the scratch, the call: sc_sortscan.hip, the one unit that
// includes hipcub's device algorithms), and the front that "CSR from sorted (row << 32 | column) keys" starts with.  The
// caller hands in the scratch buffer and the stream: each scratch keeps its owner and its lifetime (rs_tmp, cub_tmp,
// gt_tmp for the transpose that may run on the moments stream, Louvain's tmp that dies with its state).  DESIGN.md 4.6v.
#pragma once

#include "sc_ctx.h"

// bits that hold 0 .. count - 1 (at least 1): the end_bit of a sort on such values
inline int sc_bits_for(int64_t count)
{
    int b = 1;
    while (((int64_t)1 << b) < count) ++b;
    return b;
}

// cnt (key, payload) pairs sorted on the key bits [0, end_bit), stable, enqueued on s.  Instantiated in sc_sortscan.hip for
// the combinations in use.
template <class K, class V>
int sc_sort_pairs(sc_ctx *c, DBuf &tmp, hipStream_t s, const K *k_in, K *k_out, const V *v_in, V *v_out, int64_t cnt, int end_bit);

// offsets[0 .. n_plus_1) = exclusive sums of counts[0 .. n_plus_1), enqueued on s (counts[n_plus_1 - 1] = 0 makes the last
// offset the total)
int sc_exclusive_sum(sc_ctx *c, DBuf &tmp, hipStream_t s, long long *counts, long long *offsets, int64_t n_plus_1);

// heads[p] = 1 where sorted key p differs from the one before it, p < total; heads[total] = 0 for the scan.  Enqueued on s.
void sc_run_heads(hipStream_t s, const unsigned long long *keys, int64_t total, long long *heads);
