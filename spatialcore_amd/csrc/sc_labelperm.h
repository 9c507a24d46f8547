// What the label-permutation tests share across translation units (sc_labelperm.hip: enrichment and Ripley's K, where
// these are defined; sc_ligrec.hip: the ligand-receptor test).  gfx950 only.
#pragma once

#include <functional>

#include "sc_ctx.h"

// the labels, checked to lie in [0, n_types), as one byte per cell into scratch_idx (waited for: the bytes are staged in a
// local vector)
int lp_upload_labels(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types);

// k_enrich_relabel16 on c->stream: lab16[g][rank[cell]] = the labels (scratch_idx) of `cell` under rows 16 g .. 16 g + 15
// of `table` (row stride c->p_stride; rows clamped to rows - 1), one 16-byte word per cell and group of 16 rows.
// rank = nullptr: the identity, the words stay in cell order (a test without a graph)
void lp_relabel_words(sc_ctx *c, int64_t n, const int32_t *rank, const int32_t *table, int rows, uint4 *lab16);

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
