// What the per-cell (LISA) statistics share: sc_local_moran.hip (local Moran's I; owner of the preparation, of phase A
// and of the histogram) and sc_local_stats.hip (Getis-Ord Gi / Gi*, local Geary's C).  gfx950 only.
#pragma once

#include <functional>

#include "sc_ctx.h"

#define LM_PERM_BATCH 8      // float rows: permutations per launch
#define LM_CODES 32          // code rows: values 0 .. 31
#define LM_TAB_STRIDE 36     // floats per table row: (q, value) pairs of one load land in different LDS banks for small values
#define LM_U8_QUAD 4         // code rows: permutations in flight per thread
#define LM_U8_BATCH_MAX 32   // code rows: permutations per launch (the counts are read and written once per launch)

// which statistic the resident z / lag / counts belong to (sc_ctx::lm_stat; 1 and 2 are the header's SC_LOCAL_* codes)
enum { LM_STAT_MORAN = 0 };

// One job: the operands of the per-cell permutation counts
struct LmJob {
    int64_t n = 0, G = 0, T = 0;
    size_t tile_f = 0;
    // I32: the observed statistic the counts compare with, in the tile layout (local Moran: z lag, written by lm_prepare)
    float *mean32 = nullptr, *sd32 = nullptr, *Z32 = nullptr, *I32 = nullptr, *Lag32 = nullptr;
    int32_t *cnt = nullptr;
    unsigned char *zero = nullptr;
    dim3 gc;
    int mode = 2;        // 1: uint8 code rows, 2: float rows
    int groups = 0;      // code rows: 128-gene groups
    int64_t batch = 0;   // permutations per launch
    bool uni = false;
};

// statistics in numpy's order, z, observed lag and z lag; then the form of the permutation counts and its buffers
int lm_prepare(sc_ctx *c, int64_t n_perm, LmJob &j);
// phase A: the permuted rows of permutations [row, row + nb) of the forward table into c->lm_ys, in the job's form
void lm_gather(sc_ctx *c, const LmJob &j, int64_t row, int nb);
// z / lag / I32 of the job, each un-tiled into the row-major (cells x genes) staging buffer and copied out on stream s
int lm_copy_arrays(const LmJob &j, float *stage, hipStream_t s, bool sync_each, float *z_out, float *lag_out, float *I_out);
// The job as one pipeline behind the numpy-exact generator (state6 advanced as sc_perm_generate would): lm_prepare, then
// observed(j) (may be empty: what a statistic adds to the preparation, I32 included), then count(j, p0, p1) chunk by
// chunk while the generator runs; a helper thread copies z / lag / I32 out beside it (*arrays_done) where one is to be had.
int lm_seeded_pipeline(sc_ctx *c, const char *who, uint64_t *state6, int64_t n_perm, LmJob &j,
                       const std::function<int(const LmJob &)> &observed,
                       const std::function<int(const LmJob &, int64_t, int64_t)> &count, float *z_out, float *lag_out,
                       float *I_out, bool *arrays_done);
// hist[gene][c] = cells of the gene whose resident count is c, c = 0 .. c->lm_perms
int lm_hist_run(sc_ctx *c, int64_t *hist_out);
// The staging of a classification: tables and flags to the device, classify(P1, p_tab, padj_tab, flags, p, p_adj, class)
// enqueues the kernel over row-major device arrays, results back to the host
int lm_classify_run(sc_ctx *c, const float *p_tab, const float *padj_tab, const uint8_t *force_ns, float *p_out,
                    float *padj_out, int8_t *class_out,
                    const std::function<void(int, const float *, const float *, const unsigned char *, float *, float *,
                                             signed char *)> &classify);
