// What the three files of Lee's L share: host functions only, kernels are not launched across units.  gfx950 only.
//   sc_lee.hip        the global statistic: pair by pair on the resident table (sc_lee), batched with a fresh block of
//                     permutations per pair (sc_lee_seeded) or one block for a whole grid (sc_lee_shared)
//   sc_lee_f32.hip    the float32-faithful observed value (sc_lee_observed_f32)
//   sc_lee_local.hip  local Lee (sc_lee_local, sc_lee_local_seeded)
#pragma once

#include "sc_ctx.h"

// Every gene of a[0 .. k) (and of b[0 .. k), if given) is a loaded one; if not, the error is fmt with the entry point's
// name and the index of the offending entry.
int lee_check_genes(const sc_ctx *c, const char *name, const char *fmt, const int32_t *a, const int32_t *b, int64_t k);
// The operands every entry point starts from: z-scores (population sd, 0 for zero variance) and Lag = W Z of every
// loaded gene; transposed >= 1: the transposed graph; 2: and U = W^T Z in c->lee_U.  var (optional): the variances.
int lee_operands(sc_ctx *c, int transposed, std::vector<double> *var);
// out[k][cell] = gene d_genes[k] of the tiles T: gene-major contiguous copies (d_genes is device memory)
void lee_gene_major(sc_ctx *c, const double *T, const int32_t *d_genes, int k, double *out);

// One pair at a time on contiguous vectors (sc_lee's loop, sc_lee_local_seeded): the observed row and P permutation rows.
struct LeePair {
    int64_t n = 0, P = 0;                    // cells; permutation rows of the pair in hand (lee_pair_prepare)
    const int32_t *d_xy = nullptr;           // device: (gene x, gene y) of every pair of the list
    const int2 *d_slot = nullptr;            // device: the one-entry slot table (0, 0) of k_lee_rows
    double *zx = nullptr, *zy = nullptr;     // z_x | z_y side by side
    double *lagy = nullptr, *u = nullptr;    // (W z_y) out of the Lag tiles; u = W^T z_x
    std::vector<double> sums;                // host: the P row sums, then the observed one
};
// Scratch of the pairs xy[2 q], xy[2 q + 1] with up to P_max rows each; `extra` doubles behind the four vectors in
// c->scratch_a are the caller's.  xy is read until c->stream is next synchronised.
int lee_pair_alloc(sc_ctx *c, const int32_t *xy, int64_t n_pairs, int64_t P_max, size_t extra, LeePair &j);
// z_x, z_y, the observed partial sums of pair q and, for P > 0 rows, u = W^T z_x (needs lee_operands(c, 1, ..))
int lee_pair_prepare(sc_ctx *c, LeePair &j, int64_t q, int64_t P);
// partial sums of the pair's rows [p0, p1): rows row0 + p0 .. of the forward table
int lee_pair_score(sc_ctx *c, const LeePair &j, int64_t row0, int64_t p0, int64_t p1);
// the row sums, their download (ONE synchronisation of c->stream), L and #{|L_perm| >= |L|}; L_perm (optional): the P sums
int lee_pair_finish(sc_ctx *c, LeePair &j, double *L, int64_t *count_abs_ge, double *L_perm);
