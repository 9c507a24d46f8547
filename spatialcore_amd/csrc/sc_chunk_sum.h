// The ONE order of a sum over the cells (sc_diffusion.hip's dot products: k_df_dots; sc_umap.hip's distance sum:
// k_um_chunk_sum): chunks of SUM_CHUNK = 1024 elements; inside a chunk element e = r * 64 + lane, a lane adds its 16 terms
// for r ascending starting from the first, the 64 lane sums meet in the adjacent-pair tree (lane l takes lane l ^ 1, then
// l ^ 2, ...), a short last chunk is padded with zero terms.  The chunk sums are then added in chunk order, a running sum
// from 0 (k_df_chunk_add, k_um_mean).
//
// The two kernels write these sixteen additions and the tree out themselves.  Through one device helper (a functor per
// term, or the vector and the weights as arguments) both compiled to other register allocations, k_df_dots to 14 fewer
// instructions; their code is kept as it was (scripts/isa_diff.py), and what they share is the constant and this text.
#pragma once

constexpr int SUM_CHUNK = 1024;
