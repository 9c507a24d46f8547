// What the label-permutation tests share across translation units (sc_labelperm.hip: enrichment and Ripley's K, where
// these are defined; sc_ligrec.hip: the ligand-receptor test; sc_ripley_g.hip: Ripley's G).  gfx950 only.
#pragma once

#include <functional>

#include "sc_ctx.h"

// The labels of one cell under NP consecutive permutations, one byte each, as one machine word.
template <int NP> struct LpWord;
template <> struct LpWord<16> { typedef uint4 type; };
template <> struct LpWord<8> { typedef uint2 type; };
template <> struct LpWord<4> { typedef uint32_t type; };
template <> struct LpWord<2> { typedef uint16_t type; };
template <> struct LpWord<1> { typedef unsigned char type; };

// label byte s of a word, s a compile-time constant after unrolling (no per-lane indexing of a register array, which
// would go to scratch)
__device__ __forceinline__ int lp_label(const uint4 &w, int s)
{
    const uint32_t v = (s >> 2) == 0 ? w.x : (s >> 2) == 1 ? w.y : (s >> 2) == 2 ? w.z : w.w;
    return (int)((v >> (8 * (s & 3))) & 0xffu);
}
__device__ __forceinline__ int lp_label(const uint2 &w, int s) { return (int)((((s >> 2) ? w.y : w.x) >> (8 * (s & 3))) & 0xffu); }
__device__ __forceinline__ int lp_label(const uint32_t &w, int s) { return (int)((w >> (8 * (s & 3))) & 0xffu); }
__device__ __forceinline__ int lp_label(const uint16_t &w, int s) { return (int)(((uint32_t)w >> (8 * (s & 1))) & 0xffu); }
__device__ __forceinline__ int lp_label(const unsigned char &w, int) { return (int)w; }

// the labels, checked to lie in [0, n_types), as one byte per cell into scratch_idx (waited for: the bytes are staged in a
// local vector)
int lp_upload_labels(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types);

// k_lp_relabel_words on c->stream: lab16[g][rank[cell]] = the labels (scratch_idx) of `cell` under rows 16 g .. 16 g + 15
// of `table` (row stride c->p_stride; rows clamped to rows - 1), one 16-byte word per cell and group of 16 rows.
// rank = nullptr: the identity, the words stay in cell order (a test without a graph)
void lp_relabel_words(sc_ctx *c, int64_t n, const int32_t *rank, const int32_t *table, int rows, uint4 *lab16);

// k_lp_labels_by_position on c->stream: labp[r] = the label (scratch_idx) of the cell at position r, order[r]: the
// observed labels as the one-byte "words" of a pass without a table (NP = 1, cell_bytes = 1)
void lp_labels_by_position(sc_ctx *c, const int32_t *order, int64_t n, unsigned char *labp);

// k_lp_sums on c->stream: the integer sums of the null over a batch of `rows` NON-cumulative tables counts[p][cells],
// cells = type pairs x n_radii, against the observed one: sums[0 .. n_rows - 1][cells] += sum_p (u_p - u_obs),
// sum_p (u_p - u_obs)^2, #{p : u_p >= u_obs} and (n_rows = 4) #{p : u_p <= u_obs} on the counts cumulated over the radii
void lp_sums(sc_ctx *c, const unsigned long long *counts, const unsigned long long *obs, int rows, int cells, int n_radii,
             int n_rows, long long *sums);

// The batches of one rank's range of counter-based permutations p_first .. p_first + n_perm - 1, `batch` rows at a time
// (the observed pass is the caller's).  Batch b's rows are generated into the permutation table on stream3; then, on
// c->stream, relabel(rows) turns them into label words, count(rows) zeroes the per-batch table and counts the words into
// it, and accumulate(rows) adds that table to the device sums.  The label words are the only thing the counting reads,
// so the table is free again as soon as the relabel pass is through, and batch b + 1 is generated beside the counting
// of batch b:
//  * the first generation waits for c->stream (the table may still be read by an earlier call's kernels);
//  * the generation of b + 1 waits for the relabel of b;
//  * the counting of b waits for the generation of b.
// Returns with both streams synchronised and every event destroyed, on every path.
int lp_counter_batches(sc_ctx *c, const char *who, uint64_t seed, int64_t n, int64_t p_first, int64_t n_perm, int64_t batch,
                       const std::function<void(int)> &relabel, const std::function<int(int)> &count,
                       const std::function<void(int)> &accumulate);

// What a *_counts entry point asks of its rows of the resident permutation table: at most 65534 of them (a grid
// dimension), and, once the table is in forward form, inside it.  The device must be current.
static inline int lp_counts_rows(sc_ctx *c, const char *who, int64_t n, int64_t n_perm, int64_t perm_row0)
{
    SC_REQUIRE(n_perm >= 0 && perm_row0 >= 0, SC_ERR_INVALID, "%s: negative size", who);
    SC_REQUIRE(n_perm <= 65534, SC_ERR_INVALID, "%s: at most 65534 permutations per call (got %lld); call it per batch of the table",
               who, (long long)n_perm);
    if (n_perm <= 0) return SC_OK;
    SC_TRY(sc_perm_forward_ensure(c));
    SC_REQUIRE(c->p_n == n && perm_row0 + n_perm <= c->p_count, SC_ERR_STATE, "%s: needs permutation rows [%lld, %lld)", who,
               (long long)perm_row0, (long long)(perm_row0 + n_perm));
    return SC_OK;
}

// What a *_counter entry point asks of its range of counter-based permutations; *batch comes back clamped to the range
static inline int lp_counter_sizes(const char *who, int64_t p_first, int64_t n_perm, int64_t *batch)
{
    SC_REQUIRE(n_perm >= 0 && p_first >= 0 && *batch >= 1 && *batch <= 65534, SC_ERR_INVALID, "%s: bad sizes", who);
    if (*batch > n_perm) *batch = n_perm > 0 ? n_perm : 1;
    return SC_OK;
}
