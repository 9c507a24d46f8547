// What crosses between the two files of the per-cell (LISA) statistics: sc_local_prepare.hip (what no statistic owns) and
// sc_local_stats.hip (the counts, the finalisation and the entry points of local Moran's I, Getis-Ord Gi / Gi* and local
// Geary's C).  gfx950 only.
#pragma once

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
    // I32: the observed statistic in the tile layout (z lag as lm_prepare writes it; G or C once their kernels have run)
    float *mean32 = nullptr, *sd32 = nullptr, *Z32 = nullptr, *I32 = nullptr, *Lag32 = nullptr;
    uint32_t *cnt = nullptr;   // one word per (cell, gene): local Moran's count, or ge | le << 16
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
