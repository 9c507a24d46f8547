/*
 * spatialcore_hip.h -- C ABI of libspatialcore_hip.so (MI355X / gfx950).
 *
 * The reference (mcap91/SpatialCore, /root/reference) is pure Python: it has no FFI of its own.
 * The drop-in boundary is the Python surface of `spatialcore.spatial`
 * (reference src/spatialcore/spatial/__init__.py:11-52); spatialcore_amd/spatial/ mirrors those
 * functions and reaches the GPU only through the entry points declared here (ctypes).
 * Each entry point names the reference call site(s) whose arithmetic it replaces;
 * AC = src/spatialcore/spatial/autocorrelation.py, NB = src/spatialcore/spatial/neighborhoods.py,
 * CL = src/spatialcore/stats/classify.py, TH = src/spatialcore/stats/_thresholding.py.
 *
 * Conventions
 *  - plain pointers and sizes only; every function returns an int status (SC_OK = 0) and never
 *    throws; sc_last_error() returns the text of the last failure on the calling thread.
 *  - the caller owns all host buffers; the library owns device memory behind the opaque handle.
 *  - one handle = one GPU + one HIP stream; a handle is not thread-safe.
 *  - host arrays are C-contiguous.  "gene-major" means [gene][cell].
 */
#ifndef SPATIALCORE_HIP_H
#define SPATIALCORE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_OK 0
#define SC_ERR_INVALID 1  /* bad argument            -> ValueError in the Python shim */
#define SC_ERR_STATE 2    /* call order / missing setup -> RuntimeError                */
#define SC_ERR_HIP 3      /* HIP runtime failure     -> RuntimeError                   */
#define SC_ERR_NOMEM 4    /* device/host allocation  -> MemoryError                    */
#define SC_ERR_EMPTY 5    /* empty neighbourhoods (NB:253-260) -> ValueError           */
#define SC_ERR_ILLDEFINED 6 /* sc_mixture_*: a covariance is not positive definite -> ValueError (sklearn's message) */

/* expression value types accepted by sc_expr_* */
#define SC_F32 0
#define SC_F64 1

/* kernel ids for sc_ctx_kernel_time */
#define SC_K_MORAN_PERM 0 /* gather-dot permutation kernel (the metric's dominant kernel) */
#define SC_K_LAG 1
#define SC_K_KNN 2
#define SC_K_PERMGEN 3
#define SC_K_LEE_PERM 4
#define SC_K_PERM_SCAN 5 /* rejection scan of the permutation generator (chain of exact block states + verification) */
#define SC_K_PERM_SWAP 6 /* Fisher-Yates application, one workgroup (or wavefront) per permutation */
#define SC_K_KMEANS_SEED 7  /* centring + k-means++ seeding rounds of sc_kmeans_fit (all runs) */
#define SC_K_KMEANS_LLOYD 8 /* Lloyd E-step + fixed-order centre reduction of sc_kmeans_fit, final E-step included */
#define SC_K_RANK_EMIT 9    /* sc_ranksum: counting + scatter of the non-zero (key, group) pairs */
#define SC_K_RANK_SORT 10   /* ... the device-wide radix sort(s) of the pairs */
#define SC_K_RANK_RUNS 11   /* ... tie runs -> rank sums and tie sums */
#define SC_K_THRESH_SCORE 12 /* sc_metagene_score: per-cell score, mask and the fixed-order statistics */
#define SC_K_THRESH_SORT 13  /* sc_ks_prepare: device-wide radix sort of the scores + background moments */
#define SC_K_THRESH_KS 14    /* sc_ks_argmax / sc_ks_classify: D = ECDF - Phi, its argmax, deviation scores and labels */
#define SC_K_GMM_EM 15       /* sc_gmm_fit: the fused E-step / M-sums pass and the per-run parameter stage, all runs */
#define SC_K_GMM_POST 16     /* sc_gmm_posterior: P(high) and labels of every cell */
#define SC_K_COOCCUR 17      /* sc_cooccurrence_2d: the all-pairs distance-bin histogram */
#define SC_K_LIGREC 18       /* sc_ligrec_*: expression summed by (permuted) cluster label, observed pass included */
#define SC_K_RIPLEY_G_LIST 19    /* sc_ripley_g_build: count and fill passes of the ordered neighbour lists */
#define SC_K_RIPLEY_G_RELABEL 20 /* sc_ripley_g_*: permutation rows -> label words at the cells' positions */
#define SC_K_RIPLEY_G_COUNT 21   /* sc_ripley_g_*: the per-cell first-contact counting kernel, observed pass included */
#define SC_K_NMF_SETUP 22  /* sc_nmf_fit, sc_nmf_fit_graph: fp64 values, the column-sorted copy (stable device sort) and its chunk table */
#define SC_K_NMF_W 23      /* ... H H^T / rowsum(H) and the W pass over the rows (sc_nmf_fit_graph: with the graph term) */
#define SC_K_NMF_H 24      /* ... W^T W / colsum(W), the H pass over the column chunks and its finish */
#define SC_K_NMF_ERR 25    /* ... an error evaluation (the initial one, every tenth iteration, the final one; sc_nmf_fit_graph: with the penalty) */
#define SC_K_DIFF_KNN 26   /* sc_knn_dense: the brute-force search kernel and the merge of the candidate splits */
#define SC_K_DIFF_GRAPH 27 /* sc_diffmap_graph*: scales, union (sort), kernel weights, normalisation, components */
#define SC_K_DIFF_SPMV 28  /* sc_lanczos_run: the sparse matrix-vector products */
#define SC_K_DIFF_ORTH 29  /* ... the two Gram-Schmidt passes, the norm and the scaling of every step */
#define SC_K_ANNOT_SETUP 30   /* sc_annot_*: normalisation, scaler statistics, the D values, the column-sorted copy */
#define SC_K_ANNOT_ROWS 31    /* ... the row pass as a training forward pass (scores or direction product) */
#define SC_K_ANNOT_GRAD 32    /* ... residuals, their cell-chunk sums, the column-chunk gradient pass and its finish */
#define SC_K_ANNOT_LINE 33    /* ... one evaluation of the line search's derivatives */
#define SC_K_ANNOT_PREDICT 34 /* sc_annot_predict / sc_annot_transform: the row pass with the fused per-cell epilogue */
#define SC_K_ANNOT_STEP 35    /* sc_annot_train_step: the score update S <- S + alpha Dir */
#define SC_K_PCA_SETUP 36     /* sc_pca_begin: the normalisation of the resident values */
#define SC_K_PCA_GRAM 37      /* sc_pca_gram: the MFMA Gram kernel, the slice reduction and the column sums */
#define SC_K_PCA_PROJECT 38   /* sc_pca_project: the row pass X V^T - offset */
#define SC_K_LOUVAIN_MOVE 39  /* sc_louvain_level: the move kernels of a round and the sum of tot^2 */
#define SC_K_LOUVAIN_LEVEL 40 /* sc_louvain_*: degrees, the split (union-find, scans) and the aggregation (sort, run sums) */
#define SC_K_NEIGHBORS_GRAM 41 /* sc_knn_dense_gram: norms, the MFMA filter, the exact re-rank and the fallback scan */
#define SC_K_UMAP_GRAPH 42  /* sc_fuzzy_graph: rho, the distance mean, the bisection, union (sort), memberships, normalisation */
#define SC_K_UMAP_LAYOUT 43 /* sc_umap_layout: the maximum weight and one launch per epoch */
#define SC_K_HVG_SETUP 44   /* sc_hvg_pearson: row sums, the column-sorted copy, the per-gene sums of x and x^2, their total */
#define SC_K_HVG_DENSE 45   /* ... the dense zero term: one division and one square root per (cell, gene) pair */
#define SC_K_HVG_SPARSE 46  /* ... the correction per stored entry and the per-gene finish */
#define SC_K_COUNT_ 47      /* the ids up to here; stays as tests/test_cpu_hvg.py pins it.  The table ends at SC_K_END_ */
#define SC_K_MIX_ESTEP 47   /* sc_mixture_*: weighted log-probabilities, normalisation and the log-likelihood sum */
#define SC_K_MIX_MSTEP 48   /* sc_mixture_*: both M-step passes with their slice reductions, and the precision stage */
#define SC_K_INGEST 49      /* sc_cross_vote / sc_cross_regress: the gather kernels on the lists of sc_knn_cross */
#define SC_K_END_ 50        /* one past the last kernel id: what sc_ctx_kernel_time accepts */

typedef struct sc_ctx sc_ctx;

int sc_version(void);
const char *sc_last_error(void);
int sc_device_count(int *count);

/* ---- context ------------------------------------------------------------------------------ */
int sc_ctx_create(int device, sc_ctx **out);
int sc_ctx_destroy(sc_ctx *ctx);
int sc_ctx_sync(sc_ctx *ctx);
/* Accumulated HIP-event time (ms) and launch count of one kernel family since the last reset. */
int sc_ctx_kernel_time(sc_ctx *ctx, int kernel_id, double *ms, int64_t *launches);
int sc_ctx_reset_timers(sc_ctx *ctx);
/* Enable/disable per-launch HIP-event timing (default on; events are recorded on the ctx stream). */
int sc_ctx_set_timing(sc_ctx *ctx, int enabled);
int sc_ctx_device_mem(sc_ctx *ctx, int64_t *bytes_in_use);
/* Free memory of the context's device as the runtime reports it now (hipMemGetInfo). */
int sc_ctx_device_free(sc_ctx *ctx, int64_t *bytes_free);
/* Development aid (scripts/concurrency_probe4.py, scripts/pipeline_soak.py): raw bytes of one of the generator's device buffers
 * (0 J, 1 raw stream, 2 accept masks, 3 entering counts, 4 block states, 5 scan state, 6 table, 7 inverse table). */
int sc_debug_copy(sc_ctx *ctx, int which, int64_t offset_bytes, void *out, int64_t bytes);
/* The permutation kernels of sc_moran / sc_moran_seeded gather the narrowest EXACT copy of the raw expression values,
 * one 128-byte row per cell and gene group: uint8 when every value is an integer count in [0, 255] (128 genes per
 * row; only when every loaded gene is a lattice gene, below), uint16 for counts up to 65535 (64 genes), else float32
 * when every value is a float32 (32 genes), else the fp64 rows of the centred tiles (16 genes).  Every width rebuilds
 * the same operands and adds the same products in the same order: a gene's statistics do not depend on the width, i.e.
 * not on the genes it is loaded with.  Lattice genes (integer counts on a graph whose weights are all equal, e.g. kNN):
 * scored as the exact integer sum_j S_j x[inv_p(j)] (S = unweighted neighbour sums), #{sims >= I} decided on integers.
 * r04, opt-in (min_bits = 4): 4-bit slots, 256 per row, when that takes fewer rows than uint8 (a count below 16 is one
 * nibble, a count up to 255 the exact sum of two nibble pseudo-genes, x = lo + 16 hi; integer sums) -- same results bit for
 * bit; measured: the kernel alone 15 % faster, the pipelined step slower (heavier set-up), hence not the default.
 * min_bits (4, 8, 16, 32 or 64; default 8) forbids the narrower sources; sc_ctx_moran_source_bits reports what the last
 * scoring call gathered. */
int sc_ctx_set_moran_source_bits(sc_ctx *ctx, int min_bits);
int sc_ctx_moran_source_bits(sc_ctx *ctx, int *bits);
/* Element width of the STREAMED operand (the lag rows, `W @ z` of AC:307,864) of the last scoring call: 16 when an
 * all-count uint8 batch on an equal-weight graph kept its neighbour sums as the 16-bit integers they are (converted to
 * the same fp64 values inside the kernel), else 64.  Diagnostic: bench.py prices the kernel's compulsory bytes with it. */
int sc_ctx_moran_lag_bits(sc_ctx *ctx, int *bits);
/* ... and the number of 128-byte rows it gathers per (permutation, cell): the gene groups of the source width in use. */
int sc_ctx_moran_row_groups(sc_ctx *ctx, int *groups);
/* How the device generator of sc_perm_generate / sc_moran_seeded resolves numpy's rejection stream
 * (results are identical in every mode): 0 = automatic (block-parallel scan for n >= 131072, verified on the
 * device, sequential scan otherwise or when the verification fails), 1 = sequential scan only,
 * 2 = inject a fault into the block-parallel scan (exercises the verification + fallback; tests only). */
int sc_ctx_set_permgen_mode(sc_ctx *ctx, int mode);
/* Why the generator is not using its block-parallel form, "" when it is.  The form orders its kernels through words in
 * device memory and needs its streams on different hardware queues (the library asks for GPU_MAX_HW_QUEUES=24 when it is
 * loaded before the HIP runtime initialises -- a host application that initialised HIP first keeps its own setting);
 * the context finds out once: plain streams and a probe where the environment's value holds its eleven streams; its
 * streams spread over the three stream priority levels (the runtime's limit is per level) and a probe of all eleven
 * where the value is smaller but at least 4, or the plain probe failed; else the sequential scan with identical results,
 * and the reason here.  The spread placement is no degradation and leaves "" here (sc_ctx_permgen_form names it).
 * Every probe wait is bounded (20 ms).  sc_ctx_set_permgen_mode re-arms the whole ladder. */
int sc_ctx_permgen_note(sc_ctx *ctx, const char **message);
/* The same question asked up front instead of discovered inside the first job (spatialcore_amd.init()): place and probe
 * the context's streams now (not while a job begun by sc_moran_seeded_begin is in flight: the streams may be
 * re-created); *concurrent = 1 when they overlap (the block-parallel form is available),
 * *hw_queues_requested = the GPU_MAX_HW_QUEUES value in this process's environment (0: unset).  The reference has no
 * counterpart (single process, no device: AC:580 n_jobs=1); SURVEY section 5 "failure detection": a degradation must
 * surface like an error does. */
int sc_ctx_probe_streams(sc_ctx *ctx, int *concurrent, int *hw_queues_requested);
/* The scan form a permutation job of length n takes on this context right now, in words -- "block-parallel",
 * "block-parallel; streams spread over three priority levels (GPU_MAX_HW_QUEUES=4)", "sequential (...)" or
 * "sequential: <reason>" -- for the provenance entry the drop-in functions append
 * (src/spatialcore/core/metadata.py:49-77).  Valid until the next call of this function on the context. */
int sc_ctx_permgen_form(sc_ctx *ctx, int64_t n, const char **form);
/* Completed generator jobs by scan form, how often the block-parallel form failed its verification and the
 * job was rerun sequentially (0 unless mode 2 injected a fault), and for the block-parallel jobs (failed ones
 * included) the 16384-draw blocks resolved by a prepared table lookup / computed by the chain workgroup itself. */
int sc_ctx_permgen_stats(sc_ctx *ctx, int64_t *jobs_parallel, int64_t *jobs_sequential, int64_t *fallbacks,
                         int64_t *blocks_prepared, int64_t *blocks_chain);

/* ---- A1: kNN graph ------------------------------------------------------------------------
 * Replaces sklearn NearestNeighbors(k+1, "ball_tree").kneighbors + "drop column 0" (AC:393-401),
 * squidpy's NearestNeighbors(k).kneighbors() behind sq.gr.spatial_neighbors (AC:565-570) and
 * scipy cKDTree.query(k+1) + "drop == i" (NB:213-228).
 * xy: [n][2] float64.  idx_out: [n][k] int32, neighbours ordered by (squared distance, index);
 * squared distance = fl(fl(dx*dx) + fl(dy*dy)) in fp64 (no FMA contraction), as the tree codes
 * compute it.  Self is excluded BY INDEX unless include_self (then k counts self, AC:398).
 * rdist_out (nullable): [n][k] squared distances.  The result also stays on the device and can be
 * turned into the active graph with sc_graph_from_knn.
 * LIFETIME: with both output pointers null the call returns WITHOUT waiting for the device -- the upload of `xy` is
 * then merely enqueued, so `xy` must stay valid and unmodified until the next call on this context that waits
 * (sc_knn_fetch, sc_ctx_sync, any call that returns results); kernel errors of the search surface there as well. */
int sc_knn_2d(sc_ctx *ctx, const double *xy, int64_t n, int k, int include_self,
              int32_t *idx_out, double *rdist_out);
/* The neighbour lists of the last sc_knn_2d that was called WITHOUT output arrays (it then returns without waiting),
 * copied out on a stream of their own: neither behind the work the context has been given since, nor in its way.  For a
 * caller that fetches the lists (squidpy's obsp side effects, AC:565-570) from one thread while another uploads the
 * expression.  Either pointer may be null. */
int sc_knn_fetch(sc_ctx *ctx, int32_t *idx_out, double *rdist_out);

/* ---- A2: radius graph ---------------------------------------------------------------------
 * Replaces cKDTree.query_ball_point(coords, r) with self removed (NB:241-244): closed ball
 * fl(dx*dx+dy*dy) <= fl(r*r).  Two-pass: count fills indptr_out[n+1]; fill writes nnz indices,
 * ascending within each row.  The binned coordinates of the count call stay resident for the fill call until the next
 * neighbour search of the context (sc_knn_2d, sc_radius_count_2d, sc_nearest_*, sc_ripley_build, sc_ripley_g_build, sc_domains_2d): after one of those
 * the fill call returns SC_ERR_STATE. */
int sc_radius_count_2d(sc_ctx *ctx, const double *xy, int64_t n, double radius, int64_t *indptr_out);
int sc_radius_fill_2d(sc_ctx *ctx, int64_t nnz, int32_t *indices_out);

/* ---- A3: graph / weights ------------------------------------------------------------------
 * The active graph is a general CSR with fp64 weights (user graphs from use_existing_graph,
 * AC:558-561, are general).  sc_graph_from_knn builds it on the device from the last sc_knn_2d
 * result with w = weight for every edge and rows sorted by column index, i.e. the matrix that
 * AC:402-413 (weight = (double)(float)(1/k)) or squidpy + l1 row normalisation (weight = 1.0/k)
 * produce.  sc_graph_get copies the device CSR back (indices ascending per row). */
int sc_graph_set_csr(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const double *data,
                     int64_t n, int64_t nnz);
int sc_graph_from_knn(sc_ctx *ctx, double weight);
int sc_graph_get(sc_ctx *ctx, int64_t *indptr_out, int32_t *indices_out, double *data_out);
int sc_graph_shape(sc_ctx *ctx, int64_t *n, int64_t *nnz);
/* A6 [upstream squidpy _g_moments]: s0 = sum w, s1 = 1/2 sum (w_ij + w_ji)^2, s2 = sum_i (row_i + col_i)^2 */
int sc_graph_moments(sc_ctx *ctx, double *s0, double *s1, double *s2);

/* ---- expression operands ------------------------------------------------------------------
 * Select n_genes columns of a cells x n_vars matrix and lay them out on the device as 16-gene
 * tiles [tile][cell][16] fp64 (one 128-byte row per cell and tile).  Replaces
 * `adata[:, genes]` + densify + cast (AC:573 then scanpy's float64 cast; AC:1118-1123).
 * CSR: indptr int64[n+1], indices int32[nnz], data f32/f64.  Dense: row-major, ld = n_vars. */
int sc_expr_set_csr(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const void *data,
                    int dtype, int64_t n, int64_t n_vars, const int32_t *gene_cols, int64_t n_genes);
int sc_expr_set_dense(sc_ctx *ctx, const void *data, int dtype, int64_t n, int64_t n_vars,
                      const int32_t *gene_cols, int64_t n_genes);
/* per-gene mean and population variance of the loaded columns (fp64) */
int sc_expr_stats(sc_ctx *ctx, double *mean_out, double *var_out);

/* ---- A4: permutation source ---------------------------------------------------------------
 * numpy-exact `rng.permutation(n)` stream (AC:839,879; AC:1109,324; AC:1367,1404; squidpy
 * _score_helper): state6 = {state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger} of a PCG64
 * Generator, updated in place.  sc_perm_numpy_host fills a host table [n_perm][n] int32 (no GPU);
 * sc_perm_generate makes the same table resident on the device as the active permutation table
 * (perm_out nullable: copy back).  sc_perm_set uploads a caller-made table. */
int sc_perm_numpy_host(uint64_t *state6, int64_t n, int64_t n_perm, int32_t *perm_out);
int sc_perm_generate(sc_ctx *ctx, uint64_t *state6, int64_t n, int64_t n_perm, int32_t *perm_out);
int sc_perm_set(sc_ctx *ctx, const int32_t *perm, int64_t n, int64_t n_perm);
/* EXTENSION (SURVEY 8(e) "alternative", H2) for the paths WITHOUT reference seed semantics (label-permutation
 * enrichment, shared-permutation Lee grids; the reference has neither: NB:48-296, AC:1109-1148): counter-based
 * permutations.  Permutation p is a pure function of (seed, p) -- Fisher-Yates with j = Lemire-bounded(Philox4x32-10(key =
 * seed words, counter = (i, retry, p))) -- so ranks / batches take disjoint ranges [p_first, p_first + n_perm) and merge
 * integer counts (sc_allreduce_sum_i64).  sc_perm_generate_counter makes them the resident table (rows 0 .. n_perm-1);
 * sc_perm_counter_host is the same definition on the host (no GPU). */
int sc_perm_generate_counter(sc_ctx *ctx, uint64_t seed, int64_t n, int64_t p_first, int64_t n_perm, int32_t *perm_out);
int sc_perm_counter_host(uint64_t seed, int64_t n, int64_t p_first, int64_t n_perm, int32_t *perm_out);

/* ---- A3 + A5 + A6 + A7: global Moran's I --------------------------------------------------
 * Replaces sq.gr.spatial_autocorr(mode="moran", n_perms=P, seed=seed) (AC:576-583):
 * z = x - mean; lag = W z (row-sequential fp64); I = n/s0 * sum z*lag / sum z^2;
 * sims[p][g] = n/s0 * sum_i z_g[i] * lag_g[perm_p[i]] / sum z_g^2  (== scoring g[perm_p, :]).
 * Needs: active graph, expression, and (if n_perm > 0) an active permutation table.
 * Outputs (host, all nullable except I_out): I_out[G]; sims_out[n_perm][G];
 * count_ge_out[G] = #{p : sims[p][g] >= I[g]}; sim_sum_out[G], sim_sumsq_out[G] = sum and sum of
 * squares of sims over p (for squidpy's pval_z_sim / var_sim). */
int sc_moran(sc_ctx *ctx, int64_t n_perm, double *I_out, double *sims_out, int64_t *count_ge_out,
             double *sim_sum_out, double *sim_sumsq_out);
/* Same result as sc_perm_generate(state6, n_cells, n_perm) followed by sc_moran(n_perm), but the
 * two are pipelined: the generator's rejection scan runs ahead on its own streams (a chain of exact block states
 * on a few CUs the scoring stream leaves free) while the rest of the chip applies the swaps and scores the
 * previous chunk of permutations.
 * state6 is advanced exactly as n_perm calls of rng.permutation(n_cells) would; the table stays
 * resident as the active permutation table (for a float32 matrix the pipeline only builds its inverse, the same
 * Fisher-Yates transpositions in ascending order; the rows themselves are materialised when a later call needs them). */
int sc_moran_seeded(sc_ctx *ctx, uint64_t *state6, int64_t n_perm, double *I_out, double *sims_out,
                    int64_t *count_ge_out, double *sim_sum_out, double *sim_sumsq_out);
/* sc_moran_seeded in two halves: _begin needs nothing but n_cells and the generator state and returns at once with the
 * whole generator job enqueued, so the longest chain of the call runs while the caller builds the graph and uploads the
 * expression (the reference's call order -- sq.gr.spatial_neighbors AC:565-570, then the matrix AC:573, then
 * spatial_autocorr AC:576-583 -- put 60 ms of graph + PCIe work in front of it); _finish prepares the operands and
 * scores chunk after chunk.  Same results and final state6 as sc_moran_seeded; _abort drops a begun job.
 * ahead_chunks: generator chunks (of <= 128 permutations) enqueued before _begin returns: 0 = all (callers with an upload
 * in front of _finish), n >= 2 = that many (each costs ~3.5 ms of host time; _finish enqueues the rest as it scores). */
int sc_moran_seeded_begin(sc_ctx *ctx, const uint64_t *state6, int64_t n_cells, int64_t n_perm, int64_t ahead_chunks);
int sc_moran_seeded_finish(sc_ctx *ctx, uint64_t *state6, double *I_out, double *sims_out, int64_t *count_ge_out,
                           double *sim_sum_out, double *sim_sumsq_out);
int sc_moran_seeded_abort(sc_ctx *ctx);

/* ---- A8: Lee's L ---------------------------------------------------------------------------
 * Replaces _compute_lees_l_core (AC:307-332) for a list of (x, y) pairs over the loaded genes.
 * Standardisation is the population-std z-score of AC:1126-1143.  L = sum_i zx_i * (W zy)_i.
 * L_perm[p] = sum_j (W^T zx)_j * zy[perm[j]] (== shuffling zy and redoing W @ zy).  Pair q uses
 * rows [perm_offset[q], perm_offset[q]+n_perm) of the active permutation table (the reference
 * draws a fresh block of P permutations per non-degenerate pair from ONE stream, AC:1109-1148);
 * pairs with perm_offset[q] < 0 (zero variance, AC:1129-1140) get L = 0, count = n_perm.
 * Outputs: L_out[n_pairs], count_abs_ge_out[n_pairs] = #{p : |L_perm| >= |L|}, L_perm_out
 * (nullable) [n_pairs][n_perm]. */
int sc_lee(sc_ctx *ctx, const int32_t *pair_x, const int32_t *pair_y, const int64_t *perm_offset,
           int64_t n_pairs, int64_t n_perm, double *L_out, int64_t *count_abs_ge_out,
           double *L_perm_out);
/* sc_lee_seeded: the whole pair loop of lees_l (AC:1113-1155) in one call.  Every distinct gene is standardised once;
 * the observed L[x][y] = sum_i z_x[i] (W z_y)[i] of all pairs is a dense contraction over the cells on the fp64 matrix
 * cores (v_mfma_f64_16x16x4_f64 per 16 x 16 genes); each pair with two live genes then draws its OWN block of n_perm
 * numpy-exact permutations, in pair order, from the one generator `state6` (pairs with a zero-variance gene draw
 * nothing: L = 0, count = n_perm, AC:1129-1140), scored as sum_j (W^T z_x)[j] z_y[perm[j]] while the generator runs.
 * count_abs_ge_out[q] = #{p : |L_perm| >= |L|}; L_perm_out (optional) is [n_pairs][n_perm].  state6 is advanced. */
int sc_lee_seeded(sc_ctx *ctx, uint64_t *state6, const int32_t *pair_x, const int32_t *pair_y, int64_t n_pairs,
                  int64_t n_perm, double *L_out, int64_t *count_abs_ge_out, double *L_perm_out);
/* sc_lee_observed_f32: the reference's OWN observed L for a float32 matrix (AC:1118-1146, 307-315 computed in
 * float32): numpy's pairwise float32 sums for mean / std / L, float32 standardisation, scipy's float32 csr_matvec for
 * the lag -- the same roundings in the same order, evaluated in parallel (the summation tree depends on n alone).
 * L32_out[q] is 0 for a pair with a zero-std gene; mean32_out / sd32_out (optional) are [n_pairs][2] (x, y). */
int sc_lee_observed_f32(sc_ctx *ctx, const int32_t *pair_x, const int32_t *pair_y, int64_t n_pairs, float *L32_out,
                        float *mean32_out, float *sd32_out);
/* sc_lee_shared (EXTENSION, no reference site: the reference draws fresh permutations per pair, AC:1109-1148): the
 * full grid genes_x x genes_y under ONE shared block of n_perm numpy-exact permutations.  The permutation statistics
 * of the grid are then n_perm dense contractions over the cells with a row-gathered operand -- fp64 matrix cores.
 * L_out / count_abs_ge_out are [n_x][n_y]; L_perm_out (optional) is [n_perm][n_x][n_y].  state6 is advanced. */
int sc_lee_shared(sc_ctx *ctx, uint64_t *state6, const int32_t *genes_x, int32_t n_x, const int32_t *genes_y,
                  int32_t n_y, int64_t n_perm, double *L_out, int64_t *count_abs_ge_out, double *L_perm_out);

/* ---- N1: Local Moran's I ---------------------------------------------------------------------
 * Replaces the batch body of local_morans_i (AC:845-896) for the loaded genes (= one batch), with the
 * reference's float32 arithmetic: z = (float(x) - mean32) / sd32, lag = W32 @ z (row-sequential
 * float32), I = z * lag, and per cell #{p : |Zs * (W @ Zs)| >= |I|} with Zs = z[perm_p], accumulated
 * on the fly instead of the reference's (P, N, B) tensor + Python loops.  Permutations are rows
 * [perm_row0, perm_row0 + n_perm) of the active table (the reference continues ONE stream across
 * batches, AC:839,879).  Outputs are row-major [n_cells][n_genes]; zero_var_out[g] = 1 where the
 * float32 sd is 0 (AC:825-830; the caller blanks those columns, AC:902-906). */
int sc_local_moran(sc_ctx *ctx, int64_t n_perm, int64_t perm_row0, float *z_out, float *lag_out,
                   float *I_out, int32_t *count_out, uint8_t *zero_var_out);
/* The same batch with its permutations drawn here: n_perm numpy-exact permutations from state6 (exactly the rows
 * sc_perm_generate would leave; state6 advanced the same way: AC:839,879, one stream across the batches), generated
 * chunk by chunk while the per-cell counts of the finished chunks are taken.  Count data (every value an integer below
 * 32) travels through the counts as uint8 code rows with z looked up per (gene, value); outputs identical either way. */
int sc_local_moran_seeded(sc_ctx *ctx, uint64_t *state6, int64_t n_perm, float *z_out, float *lag_out,
                          float *I_out, int32_t *count_out, uint8_t *zero_var_out);
/* Per-cell finalisation of the last sc_local_moran on the device (its z / lag / counts stay resident; count_out
 * above may then be null), replacing the p-value, FDR and quadrant passes of AC:888-934 over (n_cells x n_genes):
 * sc_local_moran_hist returns hist[g][c] = cells of gene g with permutation count c, c = 0..n_perm, from which the
 * caller builds per-gene lookup tables with the reference's own expressions (p = float32((c+1)/(P+1)), BH / Bonferroni
 * adjusted values per level); sc_local_moran_classify applies them: p = p_tab[g][count], p_adj = padj_tab[g][count],
 * quadrant int8 (AC:219-265: 1 HH, 2 LL, 3 HL, 4 LH by the signs of z and lag; 0 where p_adj >= alpha or
 * force_ns[g]).  Without permutations the tables / p outputs are null and quadrants come from the signs alone. */
int sc_local_moran_hist(sc_ctx *ctx, int64_t *hist_out);
int sc_local_moran_classify(sc_ctx *ctx, const float *p_tab, const float *padj_tab, const uint8_t *force_ns,
                            float alpha, float *p_out, float *padj_out, int8_t *quadrant_out);

/* ---- N1b: Getis-Ord Gi / Gi* and local Geary's C (EXTENSION: the reference has neither) -------------
 * The batch body of local_getis_ord / local_gearys_c for the loaded genes on the active graph.  z, lag, the zero-variance
 * flags, the permutation rows and the code / float row forms are sc_local_moran's.  stat selects the statistic:
 *   SC_LOCAL_GETIS  s_i = lag_i; stat_out = the standardised G_i in float64 stored as float32 -- star != 0: Gi*, the graph
 *                   holds the self edges, G = lag / sqrt((n S1 - W^2) / (n - 1)); star == 0: Gi (Ord & Getis 1995 in z
 *                   units), mi = -z / (n - 1), vi = (n - z^2) / (n - 1) - mi^2,
 *                   G = (lag - W mi) / (sqrt(vi) sqrt(((n - 1) S1 - W^2) / (n - 2))); W = sum_e w_e, S1 = sum_e w_e^2 over the
 *                   row; 0 where the denominator is 0 or not finite.
 *   SC_LOCAL_GEARY  s_i = stat_out = C_i = sum_e fl(w_e fl(d d)), d = fl(z_i - z_col(e)), float32 in edge order.
 * Per cell and gene count_ge_out = #{p : s_i(z[perm_p]) >= s_i(z)} and count_le_out = #{p : s_i(z[perm_p]) <= s_i(z)}
 * (signed, float32, the observed value's own products and sums in the same order: a tie is a tie); n_perm <= 65535.
 * Outputs are row-major [n_cells][n_genes]; the count outputs are optional. */
#define SC_LOCAL_GETIS 1
#define SC_LOCAL_GEARY 2
int sc_local_stat(sc_ctx *ctx, int32_t stat, int32_t star, int64_t n_perm, int64_t perm_row0, float *z_out, float *lag_out,
                  float *stat_out, int32_t *count_ge_out, int32_t *count_le_out, uint8_t *zero_var_out);
/* The same batch with its permutations drawn here, as one pipeline behind the numpy-exact generator: equal in every
 * output and in the state6 it leaves to sc_perm_generate + sc_local_stat (see sc_local_moran_seeded). */
int sc_local_stat_seeded(sc_ctx *ctx, int32_t stat, int32_t star, uint64_t *state6, int64_t n_perm, float *z_out,
                         float *lag_out, float *stat_out, int32_t *count_ge_out, int32_t *count_le_out, uint8_t *zero_var_out);
/* Per-cell finalisation of the last sc_local_stat, as sc_local_moran_hist / sc_local_moran_classify with the permutation
 * level m = min(ge, le) in the place of the count: hist[g][m], p = p_tab[g][m], p_adj = padj_tab[g][m].  class int8 --
 * Getis-Ord: 1 hot (G > 0), 2 cold (G < 0); Geary, against E_i = 2n / (n - 1) sum_{e : col(e) != i} w_e (float64, summed in
 * the kernel): C < E 1 high-high (z > 0, lag > 0), 2 low-low (z < 0, lag < 0), 3 other positive; C > E 4 negative.  0 where
 * p_adj >= alpha, force_ns[g], or G == 0 / C == E.  A result of sc_local_moran does not satisfy these two calls, nor one
 * of sc_local_stat sc_local_moran_hist / _classify: SC_ERR_STATE. */
int sc_local_stat_hist(sc_ctx *ctx, int64_t *hist_out);
int sc_local_stat_classify(sc_ctx *ctx, const float *p_tab, const float *padj_tab, const uint8_t *force_ns, float alpha,
                           float *p_out, float *padj_out, int8_t *class_out);

/* ---- N2: Local Lee's L -----------------------------------------------------------------------
 * Replaces the per-pair body of lees_l_local (AC:1373-1413): population-std z-scores of the two
 * loaded genes, lag = W z_y, L_local = z_x * lag, and (n_perm > 0) the per-cell count
 * #{p : |float32(z_x[i] * (W z_y[perm_p])[i])| >= |L_local[i]|} over rows [perm_row0, +n_perm). */
int sc_lee_local(sc_ctx *ctx, int32_t gene_x, int32_t gene_y, int64_t n_perm, int64_t perm_row0,
                 double *zx_out, double *lag_out, double *L_local_out, int32_t *count_out);
/* The whole pair body of lees_l_local (AC:1373-1413) as one pipeline behind the numpy-exact generator: equal, bit for bit
 * and in the generator state it leaves, to sc_perm_generate(state6, n_cells, n_perm_global + n_perm_local), sc_lee for the
 * pair on rows [0, n_perm_global) (AC:1394-1400: global L and the count of |L_perm| >= |L|) and sc_lee_local on rows
 * [n_perm_global, +n_perm_local) (AC:1402-1413) -- with the sums and counts taken chunk by chunk while the generator runs.
 * Both genes need a positive variance (the reference skips such pairs before it gets here, AC:1380-1392). */
int sc_lee_local_seeded(sc_ctx *ctx, uint64_t *state6, int32_t gene_x, int32_t gene_y, int64_t n_perm_global,
                        int64_t n_perm_local, double *L_out, int64_t *count_abs_ge_out, double *zx_out, double *lag_out,
                        double *L_local_out, int32_t *count_out);

/* ---- N3: domain distances (reference src/spatialcore/spatial/distance.py) -----------------------
 * sc_nearest_2d replaces cKDTree(target_coords).query(source_coords, k=1) (distance.py:222-232,
 * 359-367): index (into the target array, lowest index on ties) and euclidean distance
 * sqrt(fl(fl(dx*dx)+fl(dy*dy))) of the nearest target for every query point.
 * sc_pairwise_2d replaces cdist(a, b).mean() / .min() (distance.py:269, 349, 397): LDS-tiled
 * brute force over all |a| x |b| pairs.
 * Like every entry point that reads coordinates, sc_pairwise_2d and sc_pair_table_2d refuse a non-finite one with
 * SC_ERR_INVALID and its index in the message, on the host, before anything is enqueued. */
int sc_nearest_2d(sc_ctx *ctx, const double *xy_targets, int64_t n_targets, const double *xy_queries,
                  int64_t n_queries, int32_t *idx_out, double *dist_out);
int sc_pairwise_2d(sc_ctx *ctx, const double *xy_a, int64_t n_a, const double *xy_b, int64_t n_b,
                   double *mean_out, double *min_out);
/* sc_nearest_excluding_2d: the same search, but a target whose group code equals the query's excluded code is
 * skipped (idx -1 / +inf when no target is left): the per-cell "nearest other centroid" loop of
 * distance.py:305-326 (own domain skipped when source and target column coincide) as ONE launch.
 * sc_pair_table_2d: all (source group, target group) blocks of the pairwise distance matrix in one launch --
 * points arrive sorted by group with offsets a_off[n_groups_a + 1], b_off[n_groups_b + 1]; sum_out / min_out are
 * row-major [n_groups_a][n_groups_b] (sum of distances, minimum distance; +inf / 0 for an empty block).
 * Replaces the nested `for src ... for tgt ... cdist(...).mean() / .min()` loops of distance.py:329-350, 376-398. */
int sc_nearest_excluding_2d(sc_ctx *ctx, const double *xy_targets, const int32_t *target_code, int64_t n_targets,
                            const double *xy_queries, const int32_t *query_excluded_code, int64_t n_queries,
                            int32_t *idx_out, double *dist_out);
int sc_pair_table_2d(sc_ctx *ctx, const double *xy_a, const int64_t *a_off, int32_t n_groups_a, const double *xy_b,
                     const int64_t *b_off, int32_t n_groups_b, double *sum_out, double *min_out);

/* ---- A9: neighbourhood composition --------------------------------------------------------
 * Replaces the per-cell Python counting loops of NB:226-251 on the active graph's pattern:
 * counts_out[n][n_types] float32 = number of neighbours of each label.  Rows with no neighbour
 * give SC_ERR_EMPTY (NB:253-260) and n_empty_out is set. */
int sc_profile_counts(sc_ctx *ctx, const int32_t *labels, int64_t n, int32_t n_types,
                      float *counts_out, int64_t *n_empty_out);

/* ---- N4 (extension; nothing in the reference computes this) -----------------------------------
 * Cell-type pair counts over the active graph's edges for the observed labels and under label
 * permutations labels[perm_p] (rows [perm_row0, perm_row0 + n_perm) of the active table):
 * counts_out[(p * T + a) * T + b] = #{edges i -> j : type(i) = a, type(j) = b}; p = n_perm holds the
 * observed counts.  Integer arithmetic, exact. */
int sc_enrichment_counts(sc_ctx *ctx, const int32_t *labels, int64_t n, int32_t n_types, int64_t n_perm,
                         int64_t perm_row0, int64_t *counts_out);
/* The same test for ONE RANK'S RANGE [p_first, p_first + n_perm) of counter-based permutations (sc_perm_generate_counter's
 * definition) in one call: batches of `batch` permutations are generated on a second stream beside the edge counting of
 * the batch before, and only the integer sums come back -- observed_out[T*T]; sums_out[3][T*T] = sum_p (count_p - observed),
 * sum_p (count_p - observed)^2, #{p : count_p >= observed}: exact and order-free, ranks add theirs (sc_allreduce_sum_i64). */
int sc_enrichment_counter(sc_ctx *ctx, const int32_t *labels, int64_t n, int32_t n_types, uint64_t seed, int64_t p_first,
                          int64_t n_perm, int64_t batch, int64_t *observed_out, int64_t *sums_out);

/* ---- N5: niches -- k-means of the neighbourhood profiles (identify_niches, NB:299-522) ---------------------------
 * The reference calls sklearn's KMeans(n_clusters=K, init="k-means++", n_init, max_iter, random_state).fit_predict;
 * this replays sklearn 1.7.2 step for step, all n_init runs side by side on the device.  The caller supplies what
 * numpy computes: tol = mean(var(X, axis=0)) * 1e-4 and x_mean = X.mean(axis=0) of the input, and the runs' draws of
 * ONE RandomState(random_state): per run 1 + (K - 1) * L doubles, L = 2 + int(log(K)) -- the random_sample() of
 * choice(n, p=w / sum(w)) (mapped to the first centre here by numpy's rule: cdf of the unit weights in the input type,
 * searchsorted right), then uniform(size=L) of each later centre.  The stream does not depend on the data.
 *  - X: n x C, row-major, dtype SC_F32 or SC_F64 (x_mean and centers_out in the same type); centred on the device;
 *  - seeding: D^2 = (-2 x.c + |c|^2) + |x|^2 in fp64, stored in the input type and clipped at 0; potentials and the
 *    prefix sum searched for rand_vals = u * pot are fp64 sums in one fixed order, rounded to the input type once;
 *    the candidate of lowest potential wins (first on ties);
 *  - Lloyd: fp64 distances, first index on ties; per-workgroup fp64 partial sums reduced in a fixed order (no
 *    floating-point atomics); stop when the labels do not change (strict) or when sum |shift|^2 <= tol; without strict
 *    convergence one more E-step against the final centres; an empty cluster takes the point farthest from its centre
 *    (sklearn's _relocate_empty_clusters_dense; equal distances: lowest point index first);
 *  - best run: a later run replaces it only if inertia < best and its partition differs (_is_same_clustering).
 * Out: labels_out[n] of the best run, centers_out[K][C] (+ x_mean), inertia_out (fp64), seeds_out[n_init][K] (every
 * run's k-means++ indices), n_iter_out and strict_out (1: labels unchanged in the last iteration) of the best run,
 * distinct_out = number of distinct labels (< K: sklearn's ConvergenceWarning).  The result is a function of the
 * arguments alone, bit for bit.  Invalid arguments (K < 2, K > n, C < 1, ...) give SC_ERR_INVALID. */
int sc_kmeans_fit(sc_ctx *ctx, const void *X, int dtype, int64_t n, int32_t C, int32_t K, int32_t n_init,
                  int32_t max_iter, double tol, const void *x_mean, const double *uniforms, int32_t *labels_out,
                  void *centers_out, double *inertia_out, int64_t *seeds_out, int32_t *n_iter_out, int32_t *strict_out,
                  int32_t *distinct_out);

/* ---- N6 (extension; no reference site: nothing in the reference computes a point-pattern statistic) ----------------
 * Cross-type Ripley's K: pair counts by cell-type pair and radius, observed and under label permutations.
 * Definition: for radii r_1 < ... < r_R (1 <= R <= 32) and T cell types,
 *   count[a][b][j] = number of ORDERED pairs (i, i'), i != i', type(i) = a, type(i') = b, with
 *                    fl(fl(dx dx) + fl(dy dy)) <= fl(r_j r_j)   (fp64, no FMA: the closed ball of sc_radius_count_2d),
 * cumulative in j.  Hence sum_ab count[a][b][j] = nnz of the radius graph at r_j, count[.][.][j] = the counts of
 * sc_enrichment_counts on that graph, and count[a][b][j] = count[b][a][j].  Integer arithmetic, exact, run-to-run
 * identical.  K, L and the p-values are host arithmetic on these integers (spatialcore_amd.spatial.ripley_k).
 *
 * sc_ripley_build: bins the points and builds, on the device, the list of pairs within r_R, each with one byte (the
 *   index of the smallest radius that contains it).  The list is kept beside the active graph (which it does not touch)
 *   and stays valid until the next neighbour search of the context (sc_knn_2d, sc_radius_count_2d, sc_nearest_*,
 *   sc_ripley_build, sc_ripley_g_build, sc_domains_2d): the counting entry points then return SC_ERR_STATE.  n_pairs_out = ordered pairs within r_R.
 *   More than 4.2e9 stored pairs: SC_ERR_INVALID.
 * sc_ripley_counts: counts_out[((p T + a) T + b) R + j] for the label vectors labels[perm_p], perm_p = rows
 *   [perm_row0, perm_row0 + n_perm) of the active permutation table; p = n_perm holds the observed counts.
 * sc_ripley_counter: the same test for ONE RANK'S RANGE [p_first, p_first + n_perm) of counter-based permutations
 *   (sc_perm_generate_counter's definition) in one call: batch b + 1 is generated on a second stream beside the pair
 *   counting of batch b, and only integer sums come back -- observed_out[T*T*R]; sums_out[4][T*T*R] =
 *   sum_p (count_p - observed), sum_p (count_p - observed)^2, #{p : count_p >= observed}, #{p : count_p <= observed}:
 *   exact and order-free, ranks add theirs (sc_allreduce_sum_i64).
 * Envelope: T <= 96 and T (T + 1) / 2 * R <= 16384 (one histogram of the unordered type pairs in 64 KB of LDS; covers
 * every shape with T T R <= 16384); beyond it SC_ERR_INVALID with the limit in the message. */
int sc_ripley_build(sc_ctx *ctx, const double *xy, int64_t n, const double *radii, int32_t n_radii, int64_t *n_pairs_out);
int sc_ripley_counts(sc_ctx *ctx, const int32_t *labels, int64_t n, int32_t n_types, int64_t n_perm, int64_t perm_row0,
                     int64_t *counts_out);
int sc_ripley_counter(sc_ctx *ctx, const int32_t *labels, int64_t n, int32_t n_types, uint64_t seed, int64_t p_first,
                      int64_t n_perm, int64_t batch, int64_t *observed_out, int64_t *sums_out);

/* ---- N11 (extension; no reference site: spatstat's Gcross, squidpy's ripley(mode="G")) ----------------------------------
 * Cross-type nearest-neighbour distance distribution G: cells with a neighbour of a type within a radius, by cell-type
 * pair and radius, observed and under label permutations.
 * Definition: for radii r_1 < ... < r_R (1 <= R <= 32) and T cell types,
 *   count[a][b][j] = number of cells i of type a that have at least one OTHER cell i' != i of type b with
 *                    fl(fl(dx dx) + fl(dy dy)) <= fl(r_j r_j)   (fp64, no FMA: the closed ball and the exact distance rule
 *                    of sc_ripley_build / sc_radius_count_2d).  "Other" is decided by index: a coincident cell counts.
 * The table is cumulative in j, count[a][b][j] <= n_a, and NOT symmetric in (a, b).  Integer arithmetic, exact,
 * run-to-run identical.  G[a][b][j] = count / n_a (NaN where n_a = 0), the Poisson curve and the p-values are host
 * arithmetic on these integers (spatialcore_amd.spatial.ripley_g).  No edge correction, as for N6: it cancels in the
 * permutation null.  G is a minimum per cell, not a sum over pairs: none of the pair-count kernels can produce it.
 *
 * sc_ripley_g_build: bins the points (bins no smaller than r_R) and builds, on the device, the ORDERED neighbour lists
 *   within r_R of every cell in bin-position order: per cell a row of (int32 column position, one byte = the index of the
 *   smallest radius that contains the pair), the bytes of a row non-decreasing, with int64 offsets per row.  The lists
 *   never visit the host.  They are kept beside the active graph and beside the pair list of sc_ripley_build (neither is
 *   touched) and stay valid until the next neighbour search of the context (sc_knn_2d, sc_radius_count_2d, sc_nearest_*,
 *   sc_ripley_build, sc_ripley_g_build, sc_domains_2d): the counting entry points then return SC_ERR_STATE ("no list").
 *   n_entries_out = ordered pairs within r_R, the value sc_ripley_build reports.  More than 4.2e9 entries: SC_ERR_INVALID.
 * sc_ripley_g_counts: counts_out[((p T + a) T + b) R + j] for the label vectors labels[perm_p], perm_p = rows
 *   [perm_row0, perm_row0 + n_perm) of the active permutation table; p = n_perm holds the observed table.
 * sc_ripley_g_counter: the same test for ONE RANK'S RANGE [p_first, p_first + n_perm) of counter-based permutations
 *   (sc_perm_generate_counter's definition) in one call: batch b + 1 is generated on a second stream beside the counting
 *   of batch b, and only integer sums come back -- observed_out[T*T*R]; sums_out[4][T*T*R], the four rows of
 *   sc_ripley_counter: exact and order-free, ranks add theirs (sc_allreduce_sum_i64).
 * Envelope: T <= 64 (one bit per type in the per-cell mask of types already seen) and T T R <= 16384 (one histogram of
 * the ordered type pairs in 64 KB of LDS); beyond it SC_ERR_INVALID with the limit and the shape in the message. */
int sc_ripley_g_build(sc_ctx *ctx, const double *xy, int64_t n, const double *radii, int32_t n_radii, int64_t *n_entries_out);
int sc_ripley_g_counts(sc_ctx *ctx, const int32_t *labels, int64_t n, int32_t n_types, int64_t n_perm, int64_t perm_row0,
                       int64_t *counts_out);
int sc_ripley_g_counter(sc_ctx *ctx, const int32_t *labels, int64_t n, int32_t n_types, uint64_t seed, int64_t p_first,
                        int64_t n_perm, int64_t batch, int64_t *observed_out, int64_t *sums_out);

/* ---- N9 (extension; no reference site: squidpy's co_occurrence, the third cell-type pattern statistic beside ------
 * neighbourhood enrichment and Ripley's K) -- cell-type co-occurrence by distance: pair counts per type pair and
 * distance bin over ALL pairs of cells, one streaming pass, no pair list (the default looks out to half the tissue's
 * extent: 10^12 ordered pairs at 10^6 cells).
 * Inputs: n points in 2-D (fp64) SORTED BY TYPE with offsets type_off[n_types + 1] (the convention of sc_pair_table_2d;
 * empty types allowed, their rows and columns are zero), thresholds t_0 < t_1 < ... < t_R (fp64, finite, t_0 >= 0),
 * n_thresholds = R + 1, 2 <= n_thresholds <= 128.
 * Counts: for an ordered pair (i, i'), i != i', d2 = fl(fl(dx dx) + fl(dy dy)) (fp64, no FMA: the distance of every
 * search here); the pair's bin is the smallest j with d2 <= fl(t_j t_j), the closed-ball predicate of
 * sc_radius_count_2d and sc_ripley_build; a pair with d2 > fl(t_R t_R) is dropped.  counts_out, row-major
 * [n_types][n_types][n_thresholds] int64: count[a][b][j] = ordered pairs of types (a, b) in bin j -- bin 0 the pairs
 * within t_0, bins 1 .. R the annuli (t_{j-1}, t_j].  So count[a][b][j] == count[b][a][j]; the prefix sum over j,
 * summed over a and b, is the nnz of the radius graph at t_j; coincident points (d2 == 0) are in bin 0; the table is
 * identical from run to run and does not depend on the order of the cells (integer adds only).  The co-occurrence
 * ratio is host arithmetic on these integers (spatialcore_amd.spatial.co_occurrence).
 * Validated on the host before anything is enqueued (SC_ERR_INVALID with the argument in the message): null pointers,
 * offsets that do not start at 0 or are not monotone, n_types outside 1 .. 65535, thresholds outside the above, a
 * non-finite coordinate (with its index).  The call uses neither the bin grid nor the active graph: both, a pending
 * radius count and a built Ripley pair list are left as they were. */
int sc_cooccurrence_2d(sc_ctx *ctx, const double *xy, const int64_t *type_off, int32_t n_types,
                       const double *thresholds, int32_t n_thresholds, int64_t *counts_out);

/* ---- N10 (extension; no reference site: squidpy's gr.ligrec, the CellPhoneDB permutation test) ----------------------
 * Ligand-receptor test over ordered cluster pairs: for every interaction (L, R) of two loaded genes and every ordered
 * pair of clusters (a, b), how many label permutations give a mean of L in a plus a mean of R in b at least as large as
 * the observed one.  Exact integers, order-free.
 * Definition, on the G genes and n cells of sc_expr_set_* and labels[i] in [0, n_types):
 *  - gene g carries the shift s_g = shift[g]; a value x enters as the integer q = rint(x 2^s_g) (fp64 scaling by a power
 *    of two, round half to even), which must satisfy |q| < 2^32.  The caller chooses the shifts: 0 for a gene of integer
 *    counts in [0, 2^32) (raw counts are summed as they are), else 32 - e_g with e_g the smallest integer such that
 *    max |x| < 2^e_g.
 *  - S[c][g] = sum of q over the cells of cluster c (int64: n < 2^31), N[c][g] = #{cells of c with x > 0},
 *    n_c = cells of c.  sum_out and nnz_out are [n_types][G], group_n_out is [n_types].
 *  - A label permutation keeps every n_c.  With S_p the table under the labels labels[perm_p], the comparison
 *    "(mean_L,a + mean_R,b) / 2 under p >= observed" is decided as
 *        2^s_R n_b (S_p[a][L] - S[a][L]) + 2^s_L n_a (S_p[b][R] - S[b][R]) >= 0
 *    in 128-bit integer arithmetic (both powers divided by the smaller: |s_L - s_R| <= 30 is required, SC_ERR_INVALID
 *    naming the two genes otherwise).  count_ge_out[(i n_types + a) n_types + b] = #{p : the comparison holds} for
 *    interaction i = (pair_l[i], pair_r[i]), indices into the loaded genes; a gene may pair with itself and appear in
 *    any number of interactions.
 *  The result is a function of the inputs alone: it does not depend on batching, on the genes loaded together, on the
 *  rank count or on the run (integer adds and compares only; no floating-point atomics).  Means and p-values are host
 *  arithmetic on these integers (spatialcore_amd.spatial.ligrec).
 * sc_ligrec_counts: perm_p = rows [perm_row0, perm_row0 + n_perm) of the active permutation table.  null_sums_out
 *   (nullable): S_p for every row, [n_perm][n_types][G].
 * sc_ligrec_counter: ONE RANK'S RANGE [p_first, p_first + n_perm) of counter-based permutations
 *   (sc_perm_generate_counter's definition), `batch` rows at a time, batch b + 1 generated on a second stream beside the
 *   sums of batch b; ranks add their count_ge (sc_allreduce_sum_i64).  Like sc_ripley_counter it leaves no permutation
 *   table later calls may rely on.
 * Envelope: 1 <= n_types <= 96 (SC_ERR_INVALID beyond, limit in the message), n equal to the loaded cell count, every
 * label in range, pair indices within the loaded genes, 1 <= n_pairs <= 2^24, at most 65534 rows per call or batch;
 * n_perm = 0 is legal and gives the observed tables and zeros.  A value that is not finite, or whose rint(x 2^s) leaves
 * (-2^32, 2^32), gives SC_ERR_INVALID naming the gene; no loaded expression gives SC_ERR_STATE.  The call leaves the active
 * graph, the bin grid, a Ripley pair list and the loaded expression as they were. */
int sc_ligrec_counts(sc_ctx *ctx, const int32_t *labels, int64_t n, int32_t n_types, const int32_t *shift,
                     const int32_t *pair_l, const int32_t *pair_r, int64_t n_pairs, int64_t n_perm, int64_t perm_row0,
                     int64_t *sum_out, int64_t *nnz_out, int64_t *group_n_out, int64_t *null_sums_out, int64_t *count_ge_out);
int sc_ligrec_counter(sc_ctx *ctx, const int32_t *labels, int64_t n, int32_t n_types, const int32_t *shift,
                      const int32_t *pair_l, const int32_t *pair_r, int64_t n_pairs, uint64_t seed, int64_t p_first,
                      int64_t n_perm, int64_t batch, int64_t *sum_out, int64_t *nnz_out, int64_t *group_n_out,
                      int64_t *count_ge_out);

/* ---- N7: spatial domains (make_spatial_domains, reference src/spatialcore/spatial/domains.py:289-732) ---------------
 * The reference hands this step to R (domains.py:579-638, r_functions.R:34-124: st_buffer, st_union, negative
 * st_buffer, concaveman, st_join).  Here buffer - union - shrink is taken in its continuous meaning over discs and
 * computed from the points alone.  d = cell_dist, s = shrink (the caller's cell_dist - shrink_margin), 0 <= s < d.
 *  - U = union of the closed discs of radius d about the targets.  Its polygons are the connected components of the
 *    graph on the targets with an edge iff fl(fl(dx dx) + fl(dy dy)) <= fl((2d)(2d)) (fp64, no FMA; 2d is an exact
 *    doubling).  target_component_out[i] = the smallest target index in i's component: a function of the input alone,
 *    identical from run to run (integer atomics on a parent array, lock-free union-find with path halving).
 *  - A query p lies in the shrunken region iff the closed disc of radius s about p is contained in U.
 *    clearance_out[q] (nullable) = min(s, distance from p to the boundary of U) for p in U, and -1.0 when no target is
 *    within d (p outside U).  The boundary point nearest to p, when closer than s, is a foot point
 *    t_i + d (p - t_i) / |p - t_i| of a circle that contains p (targets on p's spot have none) or one of the two
 *    intersection points of circles i and j, 0 < |t_i - t_j| <= 2d; either counts only if no other disc holds it
 *    strictly inside (targets coincident with t_i or t_j are the same circle).  fp64 throughout.
 *    query_component_out[q] = the component of the targets within d of p when clearance >= s (they are pairwise
 *    within 2d, so it is unique), else -1.
 *  - n_queries = 0: components only (xy_queries and the query outputs may be null).
 * The targets are binned by the context's bin grid: like every neighbour search, the call ends a pending
 * sc_radius_count_2d and the lists of sc_ripley_build and sc_ripley_g_build.  Bad sizes, a non-finite or non-positive cell_dist, a shrink
 * outside [0, cell_dist) or a non-finite coordinate give SC_ERR_INVALID with the argument in the message. */
int sc_domains_2d(sc_ctx *ctx, const double *xy_targets, int64_t n_targets, const double *xy_queries, int64_t n_queries,
                  double cell_dist, double shrink, int32_t *target_component_out, int32_t *query_component_out,
                  double *clearance_out);

/* ---- N8 (extension; no reference site: the reference's domain vignette calls scanpy's rank_genes_groups) ----------
 * Wilcoxon rank sums of the loaded genes (sc_expr_set_*: G genes, n cells) per group of cells, as exact integers.
 * Definition:
 *  - group_code[i] in [0, n_groups) places cell i in a group; -1 excludes the cell from the ranking altogether (the
 *    two-group comparison `reference=<group>`); anything else is SC_ERR_INVALID with the cell index in the message.
 *  - Per gene the ranked cells get average ranks, 1-based, ties sharing the mean of their positions:
 *    scipy.stats.rankdata(x[code >= 0]).  Ties are decided on the loaded fp64 values; those represent a float32
 *    matrix exactly, so float32 input has float32's tie structure.
 *  - rank2_out[g][k] = sum over the ranked cells of group k of 2 * rank: an integer.
 *  Only the non-zero values are sorted.  With N ranked cells, n_neg of them below zero, n_zero equal to zero, and a
 *  run of equal non-zero values at sorted positions [a, b) among the gene's non-zeros:
 *    a run of negative values has 2 * rank = a + b + 1, a run of positive values 2 * rank = 2 n_zero + a + b + 1,
 *    every zero has 2 * rank = 2 n_neg + n_zero + 1 (added on the device from group_n - nnz).
 *  - tie_out[g] = (hi, lo) words of the sum over the tie runs of NON-ZERO values of t^3 - t, exact for every accepted
 *    n (128-bit).  The zero block's n_zero^3 - n_zero is NOT part of it: the caller adds it.
 *  - nnz_out[g][k] = cells of group k with a non-zero value; sum_out[g][k] = sum of the group's values (per-workgroup
 *    partials over at most 256 cells of one group, reduced in a fixed order: no floating-point atomics);
 *    n_neg_out[g] = ranked cells with a negative value; group_n_out[k] = ranked cells of group k.
 *  All integer outputs are exact, order-free and identical from run to run, and a gene's results do not depend on the
 *  genes it is loaded with.  One device-wide radix sort per batch of pairs: genes whose values are all float32-exact
 *  sort once on a 64-bit key (gene | ordered float32 bits); other batches sort by the ordered fp64 bits and then
 *  stably by gene.
 * n must equal the loaded cell count.  Envelope: 1 <= n_groups <= 4096 (SC_ERR_INVALID beyond, limit in the message).
 * A non-finite expression value gives SC_ERR_INVALID and names the gene; no loaded expression gives SC_ERR_STATE. */
int sc_ranksum(sc_ctx *ctx, const int32_t *group_code, int64_t n, int32_t n_groups, int64_t *rank2_out,
               uint64_t *tie_out, int64_t *nnz_out, double *sum_out, int64_t *n_neg_out, int64_t *group_n_out);

/* ---- T1-T4: classify_by_threshold (CL:419-894, TH:27-344) -----------------------------------------------------------
 * Every floating-point sum of these entry points is taken in ONE order ("block order"): workgroup b owns the 2048
 * consecutive points [2048 b, 2048 b + 2048), its thread t adds the points 2048 b + 256 j + t, j = 0 .. 7, in that order;
 * the 256 thread values are added as a fixed tree (value[t] += value[t + h], h = 128, 64, .. 1); the workgroups are added
 * in index order.  No floating-point atomics: each result is a function of the arguments alone, bit for bit.
 * tests/threshold_restated.py states the same in numpy.
 *
 * T1 sc_metagene_score -- compute_metagene_score (TH:27-99) plus the mask and checks of CL:680-745.
 *  - features: n x n_features, row-major, SC_F32 or SC_F64; 1 <= n_features <= 64.
 *  - method: 0 shifted_geometric_mean (exp(mean(log(x + pseudocount))) - pseudocount), 1 geometric_mean (eps = 1e-10,
 *    TH:82), 2 arithmetic_mean, 3 median, 4 minimum.  The mean over the features is numpy's pairwise sum of a
 *    contiguous row (fewer than 8 terms: in order; otherwise 8 accumulators, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the
 *    remainder in order).  Methods 2-4 compute in the input type and equal numpy bit for bit; methods 0 and 1 compute
 *    in fp64 and round to the input type once.
 *  - valid_out[n]: 1 where every feature of the row is finite (CL:680); score_out[n] in the input type, NaN on the
 *    other rows.
 *  - stats_out[3]: min, max and mean (fp64; block order over all rows, a row that is not valid adding nothing) of the
 *    valid scores (CL:723-726);
 *    counts_out[3]: valid rows, valid rows with a score < 1e-6 (1e-6 rounded to the input type as numpy compares it,
 *    CL:732-733), valid rows with a negative feature (CL:702). */
int sc_metagene_score(sc_ctx *ctx, const void *features, int dtype, int64_t n, int32_t n_features, int32_t method,
                      double pseudocount, uint8_t *valid_out, void *score_out, double *stats_out, int64_t *counts_out);

/* T2 threshold_ks (TH:102-198), in three calls around the host's two O(1) fallbacks (TH:158-165, 181-182).
 * sc_ks_prepare: sorts the n scores (SC_F32 or SC_F64, all finite; n >= 10) with the device-wide radix sort of
 *  sc_ranksum on the ordered bits of their fp64 values and keeps the sorted fp64 array in the context.
 *  bg_out[2] = mean and POPULATION standard deviation (two passes, block order, fp64) of the first
 *  max(int(n * background_quantile), 10) sorted scores (TH:151-155); rank_out[k] = sorted[ranks[k]] for the n_ranks
 *  order statistics the host asks for; sorted_out[n] (may be NULL) = the whole sorted array.
 * sc_ks_argmax: D_i = (i + 1) / n - Phi((s_i - mean) / std) (TH:168-177) over the sorted array of the last
 *  sc_ks_prepare, Phi as scipy's ndtr (x = a / sqrt 2: 0.5 + 0.5 erf(x) for |x| < 1, else 0.5 erfc(|x|), mirrored for x > 0); out: the FIRST index of the largest D, its score and D itself.
 * sc_ks_classify: deviation_out[i] = clip((score_i - threshold) / range, 0, 1) in fp64 with range = max(max_score -
 *  threshold, 1e-10) (TH:185-190), labels_out[i] = score_i >= threshold (CL:770), *n_high_out = their number. */
int sc_ks_prepare(sc_ctx *ctx, const void *scores, int dtype, int64_t n, double background_quantile,
                  const int64_t *ranks, int32_t n_ranks, double *rank_out, double *bg_out, double *sorted_out);
int sc_ks_argmax(sc_ctx *ctx, double bg_mean, double bg_std, int64_t *index_out, double *score_out, double *d_out);
int sc_ks_classify(sc_ctx *ctx, const void *scores, int dtype, int64_t n, double threshold, double max_score,
                   double *deviation_out, int32_t *labels_out, int64_t *n_high_out);

/* T3 sc_gmm_fit -- GaussianMixture(n_components=K, n_init, covariance_type="full", random_state).fit on n x 1 scores
 * (TH:271-277), sklearn 1.7.2 (mixture/_base.py, _gaussian_mixture.py) replayed with all n_init runs side by side.
 *  - k-means labels: run r starts from KMeans(K, n_init=1, random_state=<the one shared RandomState>).fit(X).labels_;
 *    the ten calls consume the stream consecutively, so `uniforms` is the layout of sc_kmeans_fit for n_init runs,
 *    and km_tol / x_mean / km_max_iter are what that entry takes (C = 1).  The same seeding and Lloyd kernels run;
 *    EVERY run's final labels are kept (km_labels_out[n_init][n], may be NULL).
 *  - initialisation from one-hot responsibilities: nk = sum r + 10 eps (eps = 2^-52), mean = sum r x / nk, variance
 *    = sum r (x - mean)^2 / nk + reg_covar in a second pass around that mean, weights = nk / n.
 *  - one EM iteration = one launch over the scores serving every active run (log-probabilities, log-sum-exp as
 *    max + log sum exp(. - max), lower-bound sum and the M-step sums S0 = sum r, S1 = sum r x, A = sum r (x - c),
 *    B = sum r (x - c)^2 around the current mean c, block order) and one small launch per run: nk = S0 + 10 eps,
 *    mean = S1 / nk, d = mean - c, variance = (B - 2 d A + d d S0) / nk + reg_covar (ONE pass, shifted; sklearn takes
 *    a second pass around the new mean), weights = nk / sum nk, lower bound = mean log-likelihood; a run stops when
 *    |change| < tol (converged) or after max_iter iterations, with the parameters of its last M-step.
 *  - best run: strictly larger lower bound, so the first of equal runs wins.
 * All arithmetic is fp64 whatever the score type.  Out, per run: weights / means / variances [n_init][K],
 * lower_bound [n_init], n_iter and converged [n_init]; *best_out.  2 <= K <= 8, K <= n <= 2^31 - 1. */
int sc_gmm_fit(sc_ctx *ctx, const void *scores, int dtype, int64_t n, int32_t K, int32_t n_init, int32_t km_max_iter,
               double km_tol, const void *x_mean, const double *uniforms, int32_t max_iter, double tol, double reg_covar,
               int32_t *km_labels_out, double *weights_out, double *means_out, double *variances_out,
               double *lower_bound_out, int32_t *n_iter_out, int32_t *converged_out, int32_t *best_out);

/* T4 sc_gmm_posterior -- predict_proba under given parameters (TH:308-331, CL:785-795): for every score the
 * responsibilities as in T3, prob_out[i] = sum of those of the components high[0 .. n_high) in that order,
 * labels_out[i] = prob > cutoff, *n_high_cells_out = their number.  The scores need not be those of the fit. */
int sc_gmm_posterior(sc_ctx *ctx, const void *scores, int dtype, int64_t n, int32_t K, const double *weights,
                     const double *means, const double *variances, const int32_t *high, int32_t n_high, double cutoff,
                     double *prob_out, int32_t *labels_out, int64_t *n_high_cells_out);

/* ---- N12 (extension): sc_nmf_fit -- NMF(solver="mu") of a sparse cells x genes matrix ------------------------------
 * Replays sklearn 1.7.2 decomposition/_nmf.py, _fit_multiplicative_update with gamma = 1 and no regularisation, for
 * beta_loss "frobenius" (loss = 2) and "kullback-leibler" (loss = 1).  X is a CANONICAL CSR (indptr[n + 1] int64 from 0,
 * columns int32 strictly ascending inside a row, values SC_F32 or SC_F64, finite and >= 0; stored zeros are legal and
 * add nothing); anything else gives SC_ERR_INVALID.  All arithmetic is fp64 whatever the value type; EPS = 2^-23.
 *  - per iteration, first W, then (update_H != 0) H with the new W:
 *    Frobenius: W <- W o ((X H^T) / (W (H H^T))), H <- H o ((W^T X) / ((W^T W) H)), a denominator of exactly 0 -> EPS;
 *    Kullback-Leibler: q = x / max((W H)_ig, EPS) at every stored entry, W <- W o ((Q H^T) / rowsum(H)) (0 -> EPS), q again
 *    with the new W, H <- H o ((W^T Q) / colsum(W)) (0 -> 1), then H[H < 2^-52] = 0.  W H is formed at stored entries only.
 *    update_H = 0 keeps H (NMF.transform); H H^T / rowsum(H) are then computed once.
 *  - error(W, H) = sqrt(2 max(D, 0)); Frobenius: D = ((sum x^2 + tr((W^T W)(H H^T))) - 2 sum_ig x_ig (W H)_ig) / 2;
 *    Kullback-Leibler: D = sum x log(x / max((W H)_ig, EPS)) + (colsum(W) . rowsum(H) - sum x), both sums over the stored
 *    entries with x > EPS only.
 *  - e0 = error(W0, H0), prev = e0; if tol > 0 the error is evaluated after every iteration whose number is a multiple
 *    of 10: stop if (prev - e) / e0 < tol, else prev = e.  *n_iter_out = iterations done (<= max_iter).
 *  - summation order (no floating-point atomics; the result is a function of the arguments alone, bit for bit, whatever
 *    the grid): sums over a row's stored entries, over genes and over components run in index order from 0; the K-term
 *    dot (W H)_ig is the adjacent-pair tree over the K products padded with zeros to the next power of two; a gene
 *    column's stored entries (rows ascending) are added in chunks of 512 entries and the cells (W^T W, colsum(W), the
 *    per-cell error terms) in chunks of 1024 cells, each chunk in index order from 0 and the chunk sums in chunk order;
 *    sum x^2 and sum x run over the stored entries in index order.  The factors involve + x / only.
 * In / out: W[n][K] = W0 -> W, H[K][n_genes] = H0 -> H (H0 is returned as it came with update_H = 0), both finite, >= 0.
 * Out: err_trace_out[1 + max_iter / 10] = e0 and the error of every check, *n_checks_out = their number,
 * *recon_err_out = the error of the returned factors.
 * 1 <= K <= 64, 1 <= n <= 2^31 - 1, 1 <= n_genes <= 32768, 1 <= stored entries <= 2^32 - 1, max_iter >= 1, tol >= 0. */
int sc_nmf_fit(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
               int32_t n_genes, int32_t K, int32_t loss, int32_t update_H, int32_t max_iter, double tol, double *W, double *H,
               double *err_trace_out, int32_t *n_checks_out, int32_t *n_iter_out, double *recon_err_out);

/* sc_nmf_fit_graph -- graph-regularised NMF (GNMF; Cai, He, Han & Huang, IEEE TPAMI 2011), Frobenius loss, H updated:
 *   F(W, H) = 1/2 ||X - W H||_F^2 + (lambda / 2) tr(W^T L W),  L = diag(d) - A,  d_i = sum_j a_ij,
 *   tr(W^T L W) = 1/2 sum_ij a_ij ||w_i - w_j||^2.
 * X as for sc_nmf_fit.  A is an n x n CANONICAL CSR (gptr[n + 1] int64 from 0, gidx int32 strictly ascending inside a
 * row, gval double): no diagonal entry, every value finite and > 0, every entry (i, j) with a mirror (j, i) of equal
 * value; empty rows are legal (an isolated cell gets sc_nmf_fit's update) and so is a graph without entries (gidx and
 * gval may then be NULL).  lambda finite and >= 0.  Each refusal is SC_ERR_INVALID and names the first offending entry.
 *  - per iteration, first W, then H with the new W (sc_nmf_fit's Frobenius H pass):
 *      W_ik <- W_ik ((X H^T)_ik + lambda (A W)_ik) / ((W H H^T)_ik + lambda d_i W_ik)
 *    A W reads the W of the PREVIOUS iteration for every row (Jacobi: the form Cai et al. prove non-increasing in F), so
 *    the pass reads one W buffer and writes the other.  No normalisation inside the loop: the descent is kept, and the
 *    scale may drift (W shrinks, H grows; reconstruction_err and penalty show it).
 *  - order, on top of sc_nmf_fit's: d_i = sum_e a_e and g_ik = sum_e a_e Wold[j_e][k] over the row's stored entries in
 *    index order from 0; num = nx + lambda g (nx = sc_nmf_fit's numerator); den = dx + (lambda d_i) w (dx = sc_nmf_fit's
 *    denominator); den == 0 -> EPS; Wnew = w (num / den).
 *  - penalty: r_i = sum_e a_e T_k((w_ik - w_jk)^2) over the row's entries in index order, T the adjacent-pair tree over
 *    the components padded with zeros to the next power of two; R = the r_i added in chunks of 1024 cells, each in index
 *    order, the chunk sums in chunk order; tr(W^T L W) = R / 2.
 *  - F = D + (lambda (R / 2)) / 2 with D as sc_nmf_fit's Frobenius D; the objective is e = sqrt(2 max(F, 0)).
 *    e0 = e(W0, H0), prev = e0; e is evaluated after every iteration whose number is a multiple of 10, whatever tol is;
 *    if tol > 0: stop if (prev - e) / e0 < tol, else prev = e.
 *  - with lambda = 0 every added term is + 0 x finite: W and H equal sc_nmf_fit's (loss 2, update_H 1) byte for byte.
 * Out: obj_trace_out[1 + max_iter / 10] and err_trace_out[1 + max_iter / 10] = e and sqrt(2 max(D, 0)) at the start and
 * at every check, *n_checks_out = their number, *recon_err_out = sqrt(2 max(D, 0)) and *penalty_out = tr(W^T L W) of the
 * returned factors.  Limits as sc_nmf_fit's; stored graph entries <= 2^32 - 1. */
int sc_nmf_fit_graph(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                     int32_t n_genes, int32_t K, const int64_t *gptr, const int32_t *gidx, const double *gval, double lambda,
                     int32_t max_iter, double tol, double *W, double *H, double *obj_trace_out, double *err_trace_out,
                     int32_t *n_checks_out, int32_t *n_iter_out, double *recon_err_out, double *penalty_out);

/* ---- N13 (extension): diffusion maps (Haghverdi et al. 2016) -- spatialcore_amd.diffusion -----------------------------
 * All arithmetic fp64, every product and sum rounded separately, no floating-point atomics: every result is a function
 * of the arguments alone, bit for bit.  The calls leave their results on the device for the next one:
 *   sc_knn_dense -> sc_diffmap_graph   (or sc_diffmap_graph_csr alone) -> sc_lanczos_begin -> sc_lanczos_run ... ->
 *   sc_lanczos_ritz -> sc_lanczos_end.
 * sc_knn_dense: exact brute-force k nearest neighbours in d dimensions.  X[n][d] row-major SC_F32 (widened exactly) or
 *   SC_F64, finite, |x| < 2^500.  d2(i, j) = sum_c (x_ic - x_jc)^2 added in column order from the c = 0 term; the neighbours of i are the
 *   k cells j != i smallest in (d2, j).  idx_out[n][k] / d2_out[n][k] may be NULL (results stay on the device).
 *   1 <= d <= 64, 2 <= k <= 32, k < n <= 2^31 - 1, n * k <= 2^29.  `splits` = 0 lets the library split the candidates over
 *   workgroups for small n (any value gives the same bits); splits >= 1 forces that many (tests).
 * sc_diffmap_graph: from the kept lists.  s2_i = median of row i's k squared distances ((a + b) / 2 for k even); a zero
 *   scale is SC_ERR_INVALID.  Edges = symmetric union; w_ij = sqrt(2 sqrt(s2_i) sqrt(s2_j) / (s2_i + s2_j)) *
 *   exp(-d2(i, j) / (s2_i + s2_j)); CSR rows sorted by column.  q_i = sum_j w_ij (column order, from 0), K'_ij = w_ij /
 *   (q_i q_j), D_i = sum_j K'_ij, T_ij = K'_ij / (sqrt(D_i) sqrt(D_j)).  *n_components_out = connected components of the
 *   edge set.  s2_out[n] may be NULL.
 * sc_diffmap_graph_csr: the same from a caller's symmetric kernel matrix (canonical CSR, n x n, values finite and > 0,
 *   every row non-empty; symmetry is the caller's to check).
 * sc_diffmap_graph_get: indptr[n + 1], indices[nnz], w[nnz] (kernel weights) and, if not NULL, T[nnz].
 * sc_lanczos_begin: v_0 = start / ||start|| (start[n], non-zero, finite); room for max_basis steps (1 <= max_basis <= n).
 * sc_lanczos_run: `steps` more steps of Lanczos with full reorthogonalisation (classical Gram-Schmidt twice against
 *   v_0 .. v_j); alpha_out[m], beta_out[m + 1] (beta[0] = ||start||, beta[j + 1] = norm after step j) for all m steps so
 *   far, *m_out = m.  A beta below n 2^-52 is SC_ERR_STATE ("Krylov breakdown").
 *   Step j: w = T v_j (row sums in column order from 0); pass 1: c_l = v_l . w for l = 0 .. j, then w_i <- w_i - v_li c_l
 *   for l ascending; pass 2 the same with c'; alpha_j = c_j + c'_j; beta_{j+1} = sqrt(w . w); v_{j+1} = w / beta_{j+1}.
 *   Every dot product: the index range in chunks of 1024; inside a chunk element e = r * 64 + lane, each lane adds its 16
 *   products for r ascending from the first, the 64 lane sums meet in the adjacent-pair tree, a short last chunk is
 *   padded with zero products; the chunk sums are added in chunk order from 0.
 * sc_lanczos_ritz: y_l = sum_j v_j S[j][l] (j ascending from the first product; S is m x c row-major, c <= 64), scaled to
 *   unit norm; vecs_out[c][n]; resid_out[l] = ||T y_l - lambda[l] y_l||_2, dots as above.
 * sc_lanczos_end releases the basis. */
int sc_knn_dense(sc_ctx *ctx, const void *X, int dtype, int64_t n, int32_t d, int32_t k, int32_t splits, int32_t *idx_out,
                 double *d2_out);
/* sc_knn_dense_gram: the lists of sc_knn_dense, bit for bit, for every input; the same arguments, limits and refusals, and the
 *   same state left on the device (sc_diffmap_graph follows unchanged).  `path`: 0 = the library's choice by (n, padded d),
 *   1 = the direct kernels (the call is sc_knn_dense), 2 = the certified Gram-form filter: norms n_i, g_ij = x_i . x_j by
 *   v_mfma_f64_16x16x4_f64, s_ij = (n_i + n_j) - 2 g_ij, lo_ij = s_ij - E_ij with E_ij = (4 dp + 32) 2^-52 (n_i + n_j) + 2^-1000
 *   (dp = d rounded up to a multiple of 8), so that lo_ij <= d2(i, j) as the direct form computes it; a row keeps its
 *   L = k + slack smallest (lo, j), re-ranks them by the direct form and is certified iff it kept fewer than L or its k-th
 *   d2 < its L-th lo; the other rows are searched again by the direct form.  `slack`: 0 = the library's choice (8), else
 *   1 .. 16.  info_out[4] = path taken, L (k on path 1), rows certified by the filter, rows sent to the fallback (both 0 on
 *   path 1). */
int sc_knn_dense_gram(sc_ctx *ctx, const void *X, int dtype, int64_t n, int32_t d, int32_t k, int32_t path, int32_t slack,
                      int32_t *idx_out, double *d2_out, int64_t *info_out);
int sc_diffmap_graph(sc_ctx *ctx, double *s2_out, int64_t *n_edges_out, int64_t *n_components_out);
/* ---- ingest (extension; restated by tests/ingest_restated.py): query rows among reference rows ---------
 * sc_knn_cross: for every row q of Q[n_query][d] the k rows j of R[n_ref][d] smallest in (d2(q, j), j), d2 as sc_knn_dense
 *   computes it (the terms (q_c - r_jc)^2 added in column order from the c = 0 term).  Nothing is excluded: a query equal
 *   to a reference row finds it at d2 = 0.  R and Q are row-major SC_F32 or SC_F64, each widened exactly and on its own
 *   (mixed dtypes are legal), finite, |x| < 2^500.  1 <= d <= 64, 1 <= k <= 32, k <= n_ref <= 2^31 - 1, 1 <= n_query,
 *   n_query * k <= 2^29.  `path`, `slack` and info_out[4] as sc_knn_dense_gram's; path 0 chooses by (n_query, n_query * n_ref,
 *   padded d), the rule of sc_knn_dense_gram where the two sets are one (the same kernels in their cross form:
 *   lo_qj = (n_q + n_j) - 2 g_qj - E_qj; a row is certified iff it kept fewer than L = k + slack candidates, which
 *   includes n_ref < L, or its k-th d2 < its L-th lo); the lists are the same bytes on every path and for every slack.
 *   idx_out[n_query][k] / d2_out[n_query][k] may be NULL (the lists stay on the device for the two calls below).
 *   What it invalidates: everything a new sc_knn_dense invalidates (the self lists, the resident graph, an open Lanczos
 *   run), and it leaves NO self lists: sc_diffmap_graph and sc_fuzzy_graph ("no neighbour lists are resident") and every
 *   reader of the resident graph (sc_louvain_begin_resident, ...) return SC_ERR_STATE until sc_knn_dense[_gram] has run
 *   again.  The cross lists in turn are gone with the next search of either kind.
 * sc_cross_vote: on the resident cross lists.  codes_ref[n_ref] in [0, n_classes), 1 <= n_classes <= 2^31 - 1 (an entry's
 *   class is compared with the <= 32 entries of its own row, so the cost does not depend on n_classes).
 *   weighting SC_CROSS_UNIFORM: integer counts per class; label = the class with the largest count, the lowest code on
 *   ties; conf = count / k; proba = count / k.  SC_CROSS_DISTANCE (sklearn's weights="distance"): w_t = 1 / sqrt(d2_t); a row
 *   that holds any d2 = 0 gives weight 1 to its zero-distance entries and 0 to the rest; class sums and the total are added
 *   in list order (t ascending, the first term starts the sum); proba = class sum / total; label = the class of the
 *   largest proba, the lowest code on ties; conf = that proba.  label_out[n_query] (int32), conf_out[n_query];
 *   proba_out[n_query][n_classes] may be NULL (with it, n_query * n_classes <= 2^28).
 * sc_cross_regress: out[q][c] = (sum_t w_t Y[j_t][c]) / (sum_t w_t), both sums in list order from their first term, with
 *   the weights above (uniform: w_t = 1).  Y[n_ref][C] SC_F32 or SC_F64, finite; 1 <= C <= 64; out[n_query][C] fp64.
 * No cross lists resident: SC_ERR_STATE.  fp64 throughout, no floating-point atomics. */
#define SC_CROSS_UNIFORM 0
#define SC_CROSS_DISTANCE 1
int sc_knn_cross(sc_ctx *ctx, const void *R, int dtype_r, int64_t n_ref, const void *Q, int dtype_q, int64_t n_query, int32_t d,
                 int32_t k, int32_t path, int32_t slack, int32_t *idx_out, double *d2_out, int64_t *info_out);
int sc_cross_vote(sc_ctx *ctx, const int32_t *codes_ref, int32_t n_classes, int32_t weighting, int32_t *label_out, double *conf_out,
                  double *proba_out);
int sc_cross_regress(sc_ctx *ctx, const void *Y_ref, int dtype, int32_t C, int32_t weighting, double *out);
int sc_diffmap_graph_csr(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const double *w, int64_t n,
                         int64_t *n_components_out);
int sc_diffmap_graph_get(sc_ctx *ctx, int64_t *indptr, int32_t *indices, double *w, double *T);
int sc_lanczos_begin(sc_ctx *ctx, const double *start, int64_t max_basis);
int sc_lanczos_run(sc_ctx *ctx, int32_t steps, double *alpha_out, double *beta_out, int64_t *m_out);
int sc_lanczos_ritz(sc_ctx *ctx, const double *S, int64_t m, int32_t c, const double *lambda, double *vecs_out,
                    double *resid_out);
int sc_lanczos_end(sc_ctx *ctx);

/* ---- N14 (extension): CellTypist-style annotation -- spatialcore_amd.annotation ----------------------
 * The model is a StandardScaler, a clip at 10 and one-vs-rest L2 logistic regression.  X is a CANONICAL CSR as for
 * sc_nmf_fit (values SC_F32 or SC_F64, finite, >= 0) over the genes in use.  mode 0: counts, normalised on the device to
 * log1p(x / rowsum * 1e4), the row sum over the stored entries in index order; mode 1: log1p values, taken as they are;
 * mode 2: log1p values of a larger gene set: expm1, then as mode 0.  Stored zeros are legal; a row whose stored values are
 * all 0 (row sum 0 in modes 0 and 2) is an empty row.  All arithmetic is fp64, every product and sum
 * rounded separately, no floating-point atomics: every result is a function of the arguments alone, bit for bit.
 * z_ig = min((x_ig - mean_g) / scale_g, 10); a zero entry gives z0_g = -mean_g / scale_g; d_ig = z_ig - z0_g at the stored
 * entries.  A product with a table: row_it = (bias_t + sum_g z0_g w_tg, genes in index order from 0, formed on the host)
 * + d_ig w_tg over the row's stored entries in index order.
 * sc_annot_predict: scores = the product with coef[T][n_genes] and intercept[T].  labels_out[i] = first argmax of the fp64
 *   scores; conf_out[5][n] = expit(max score), then the four transforms below of the row rounded to float32;
 *   scores_out[n][T] (may be NULL) = the float32 scores.
 * sc_annot_transform: the reference's transform_confidence of any n x T matrix (SC_F32 is widened), conf_out[4][n] = raw
 *   (the maximum m), zscore = expit((m - mean) / sd) with the population sd (sd < 1e-10 -> 1), softmax = 1 / sum_t
 *   exp(x_t - m), minmax = (m - min) / (m - min) with a range < 1e-10 -> 1.  Sums over the classes: class t = 64 b + l in
 *   lane l, every lane adds its values for b ascending from 0, the lane sums (0 for a lane without a class) meet in the
 *   adjacent-pair tree over T rounded up to a power of two (64 for T > 64) lanes.
 * Training keeps one problem on the device: sc_annot_train_begin -> (_forward, _grad, _line, _step) ... -> _end.
 *   _begin: normalisation, mean_out[g] = column sum / n, the population variance with the zeros counted, scale_out[g] =
 *     its square root (1 where sklearn's StandardScaler calls the feature constant), the D values in row order and in a
 *     column-sorted copy.  Column sums: chunks of 512 stored entries (rows ascending), chunk sums in chunk order.
 *     labels[n] in [0, T), weights[n] finite and > 0 (the s_i of the objective).
 *   _forward: which = 0: S = the product with (coef, bias); which = 1: Dir = the same for a direction.
 *   _grad: with R_it = s_i (expit(S_it) - [labels_i = t]): grad_out[t][g] = sum_i d_ig R_it (the column's chunks) + z0_g
 *     sum_i R_it, grad_out[t][n_genes] = sum_i R_it, loss_out[t] = sum_i s_i (softplus(S_it) - y_it S_it); sums over cells in
 *     chunks of 1024 cells, chunk sums in chunk order.  The penalty's terms are the caller's.
 *   _line: at u = S + alpha_t Dir: d1_out[t] = sum_i s_i (expit(u) - y) Dir_it, d2_out[t] = sum_i s_i expit(u) (1 - expit(u))
 *     Dir_it^2.   _step: S <- S + alpha_t Dir.
 * 2 <= T <= 256, 1 <= n <= 2^31 - 1, 1 <= n_genes <= 32768, 1 <= stored entries <= 2^32 - 1. */
int sc_annot_predict(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                     int32_t n_genes, int32_t mode, int32_t T, const double *coef, const double *intercept, const double *mean,
                     const double *scale, float *scores_out, int32_t *labels_out, double *conf_out);
int sc_annot_transform(sc_ctx *ctx, const void *scores, int dtype, int64_t n, int32_t T, double *conf_out);
int sc_annot_train_begin(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                         int32_t n_genes, int32_t mode, int32_t T, const int32_t *labels, const double *weights,
                         double *mean_out, double *scale_out);
int sc_annot_train_forward(sc_ctx *ctx, const double *coef, const double *bias, int32_t which);
int sc_annot_train_grad(sc_ctx *ctx, double *grad_out, double *loss_out);
int sc_annot_train_line(sc_ctx *ctx, const double *alpha, double *d1_out, double *d2_out);
int sc_annot_train_step(sc_ctx *ctx, const double *alpha);
int sc_annot_train_end(sc_ctx *ctx);

/* ---- N15 (extension): exact covariance PCA -- spatialcore_amd.pca ------------------------------------
 * X is a CANONICAL CSR (rows' columns strictly ascending inside [0, n_genes), values SC_F32 or SC_F64, finite) over the
 * genes in use; negative values are legal unless normalize != 0.  Everything is fp64, -ffp-contract=off for the plain
 * C++ sums, no floating-point atomics, and the bytes of every result are a function of the arguments alone.
 * sc_pca_begin: validates the CSR on the host, uploads it and keeps the fp64 values resident: as they are, or with
 *   normalize != 0 log1p(x / rowsum * target_sum), the row sum over the stored entries in index order (a row whose sum is
 *   0 stays 0).  A second _begin replaces the resident matrix (as sc_annot_train_begin does).
 * sc_pca_gram: gram_out[G][G] = X^T X and colsum_out[G] = column sums of the resident values.  The G x G output is cut
 *   into 128 x 128 blocks, of which the upper triangle is computed; the rows are cut into S slices of R rows, with
 *   R = max(16384, ceil(n / max(1, 2048 / blocks)) rounded up to a multiple of 32) and S = ceil(n / R) -- functions of
 *   (n, n_genes) alone.  One workgroup owns (block, slice): it densifies 32 rows at a time into two column panels and
 *   accumulates with v_mfma_f64_16x16x4_f64, i.e. an element's slice sum runs over the rows in groups of four: within
 *   a k-step the hardware's order, the k-steps ascending.  gram[i][j] = the S slice sums added in ascending slice order,
 *   mirrored into [j][i].  colsum[g] = per slice the rows in ascending order from 0.0, the slice sums in ascending order.
 * sc_pca_project: scores_out[i][c] = (0.0 + sum_p val[p] * V[c][idx[p]], the row's stored entries in index order,
 *   multiply and add rounded separately) - offset[c]; out_dtype SC_F64, or SC_F32 = that value rounded once.
 *   V is [K][n_genes] row-major.  Needs _begin, not _gram.
 * sc_pca_end: frees the resident matrix.
 * 2 <= n <= 2^31 - 1, 1 <= n_genes <= 4096, 1 <= K <= 64, stored entries <= 2^32 - 1. */
int sc_pca_begin(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                 int32_t n_genes, int32_t normalize, double target_sum);
int sc_pca_values(sc_ctx *ctx, double *values_out);   /* the resident fp64 values, one per stored entry in CSR order */
int sc_pca_gram(sc_ctx *ctx, double *colsum_out, double *gram_out);
int sc_pca_project(sc_ctx *ctx, const double *V, const double *offset, int32_t K, int out_dtype, void *scores_out);
int sc_pca_end(sc_ctx *ctx);

/* ---- N16 (extension): deterministic Louvain communities -- spatialcore_amd.cluster -------------------------
 * Louvain with a connectivity split, not Leiden.  The graph is a symmetric CANONICAL CSR (columns strictly ascending
 * inside [0, n)), 1 <= n <= 2^31 - 1, stored entries <= 2^31 - 1, integer weights q_ij = q_ji in [1, 65535]; diagonal
 * entries count once in the degree and never as a neighbour; rows may be empty and the graph disconnected.
 * g = rint(resolution 2^16) in [1, 2^23].  Everything on the device is exact integer arithmetic (64-bit degrees and
 * totals, 128-bit S and Qnum, integer atomics), so every output is a function of the arguments alone.
 * One level on A with n_l vertices: k_i = sum_j A_ij, M = sum_i k_i, comm_i = i, Qnum(comm) = 2^16 M sum_{comm_i = comm_j}
 *   A_ij - g sum_c tot_c^2, tot_c = sum_{comm_i = c} k_i; best = the singletons, stale = 0.  Round r = 0, 1, ...: every vertex
 *   reads the same comm and tot; its candidates are comm_i and the comm_j of its stored neighbours j != i; k_ic = sum_{j != i,
 *   comm_j = c} A_ij; S_i(c) = 2^16 M k_ic - g k_i (tot_c - [c = comm_i] k_i); allowed are comm_i, c > comm_i in even rounds,
 *   c < comm_i in odd rounds; the vertex takes the allowed c with the largest S, on equal S its current community, then
 *   the lowest c; all moves at once; if Qnum of the new comm exceeds the best so far it becomes best and stale = 0, else
 *   stale += 1; the level ends at stale = 2 or after max_rounds rounds (the search goes on from comm, not from best).
 *   Split: the connected components of the edges (i != j) inside the communities of best, labelled by the rank of their
 *   smallest vertex.  As many components as vertices: the hierarchy is finished.  Otherwise A'_ab = sum_{i in a, j in b}
 *   A_ij is the next level's graph.
 * sc_louvain_begin: validates on the host, before its first HIP call (SC_ERR_INVALID names the first offending entry: a
 *   row that is not canonical, a weight of 0, an entry without its mirror, a mirror of another weight), uploads.  A second
 *   _begin replaces the state.
 * sc_louvain_resident_weights / sc_louvain_begin_resident: the same on the graph sc_diffmap_graph* left on the device,
 *   whose structure does not visit the host: _resident_weights fetches its nnz fp64 kernel weights so that the host can
 *   quantise them, _begin_resident takes the nnz quantised weights in CSR order (NULL: 1 per edge) and checks the
 *   symmetry on the device.  No resident graph: SC_ERR_STATE.
 * sc_louvain_level: runs one level.  info_out[12] = n_l, rounds, communities of best, components after the split, Qnum of
 *   the split partition (signed high limb, low limb), 1 if the hierarchy is finished, 1 if the level ended at max_rounds,
 *   rows in the wavefront / workgroup / global class of the move kernels (<= 64 / <= 2048 / more entries), stored entries
 *   of the level.  labels_out[n_l] (may be NULL) = the level's component labels.  After the finished level: SC_ERR_STATE.
 * sc_louvain_labels: labels_out[n] = the composition of the levels run so far, clusters numbered by descending size, ties
 *   to the smaller smallest member; *n_clusters_out their number.
 * sc_louvain_end: frees every device buffer of the state. */
int sc_louvain_begin(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const uint16_t *q, int64_t n, int32_t g,
                     int32_t max_rounds);
int sc_louvain_resident_weights(sc_ctx *ctx, double *w_out, int64_t nnz);
int sc_louvain_begin_resident(sc_ctx *ctx, const uint16_t *q, int64_t nnz, int32_t g, int32_t max_rounds);
int sc_louvain_level(sc_ctx *ctx, int64_t *info_out, int32_t *labels_out);
int sc_louvain_labels(sc_ctx *ctx, int32_t *labels_out, int64_t *n_clusters_out);
int sc_louvain_end(sc_ctx *ctx);

/* ---- N17 (extension): UMAP connectivities and a deterministic layout -- spatialcore_amd.neighbors(method="umap"),
 * spatialcore_amd.embedding -------------------------------------------------------------------------
 * Reference site: umap-learn's umap_.py (smooth_knn_dist, compute_membership_strengths, fuzzy_simplicial_set,
 * make_epochs_per_sample) and layouts.py (optimize_layout_euclidean), McInnes, Healy, Melville 2018, restated from the
 * published algorithm with that library's defaults only (local_connectivity = 1, bandwidth = 1, set_op_mix_ratio = 1).
 * Parity with umap-learn is not pinned.  fp64, every product and sum rounded separately, no floating-point atomics: every
 * result is a function of the arguments alone, bit for bit.
 * sc_fuzzy_graph: after sc_knn_dense / sc_knn_dense_gram, on the lists (idx, d2)[n][k] they left on the device.  k counts
 *   OTHER cells (umap's k is k + 1 and its list holds the cell itself at distance 0).  With d_ij = sqrt(d2_ij), j running
 *   over row i's list in list order (ascending (d2, j)):
 *   rho_i = the smallest d_ij > 0, 0 if there is none.  S_i = sum_j d_ij, a running sum from 0.
 *   target = log2(k + 1) (the host's log2 of the double k + 1).
 *   sigma_i: lo = 0, hi = inf, mid = 1; at most 64 times: psum = sum_j (t_ij > 0 ? exp(-(t_ij / mid)) : 1) with t_ij = d_ij -
 *     rho_i, a running sum from 0; stop if |psum - target| < 1e-5; if psum > target: hi = mid, mid = (lo + hi) / 2; else
 *     lo = mid and mid = mid * 2 while hi is inf, else mid = (lo + hi) / 2.  sigma_i = the last mid, then the floor: sigma_i =
 *     max(sigma_i, 1e-3 * m_i) with m_i = S_i / (k + 1) if rho_i > 0, else the mean of all distances M = (sum_i S_i) / (n (k + 1)).
 *     sum_i S_i runs in the order of the Lanczos dot products above: chunks of 1024 rows, inside a chunk element e = r * 64 +
 *     lane, every lane adds its 16 values for r ascending from the first, the 64 lane sums meet in the adjacent-pair tree, a
 *     short last chunk is padded with zeros, the chunk sums are added in chunk order from 0.
 *   p_ij = (t_ij > 0 ? exp(-(t_ij / sigma_i)) : 1) for j in row i's list, 0 otherwise.
 *   Edges = the symmetric union of the lists, the CSR pattern of sc_diffmap_graph byte for byte (rows sorted by column);
 *   w_ij = (p_ij + p_ji) - p_ij * p_ji at both positions, which makes the weights bit-symmetric.  A weight can underflow to 0
 *   only where t_ij > 745 sigma_i in the one direction that lists the edge.
 *   Then the tail of sc_diffmap_graph on these weights (q, K', D, T, the components), so that sc_diffmap_graph_get,
 *   sc_lanczos_begin, sc_louvain_resident_weights and sc_louvain_begin_resident follow as after sc_diffmap_graph.
 *   rho_out[n], sigma_out[n] may be NULL.  No lists resident: SC_ERR_STATE.
 * sc_umap_layout: epochs [e0, e1) of n_epochs on a symmetric canonical CSR (columns strictly ascending inside [0, n), w
 *   finite and > 0, rows may be empty; the symmetry is the caller's to check), 1 <= n <= 2^31 - 1; indptr = indices = w =
 *   NULL takes the graph resident on the device (sc_fuzzy_graph, sc_diffmap_graph*; n must be its size).  Y[n][C] row-major,
 *   finite, in and out, C = 2 or 3; a, b, alpha0 finite > 0, gamma finite >= 0, 0 <= neg <= 16, n_epochs >= 1, 0 <= e0 <= e1
 *   <= n_epochs.  Everything is checked on the host before the first HIP call.  A graph without entries leaves Y as it is.
 *   w_max = the exact maximum of w.  r_t = w_t / w_max.  Stored entry t (its global CSR position) FIRES in epoch e iff
 *   floor((e + 1) * r_t) > floor(e * r_t), e and e + 1 as doubles.
 *   Epoch e: alpha = alpha0 * (1 - e / n_epochs) (the division first).  Every vertex i reads the positions Y_old of the
 *   previous epoch only: cur = Y_old[i]; for every firing entry (i, j) of its row in stored order:
 *     attract:  step(cur, Y_old[j], attract);
 *     repel, q = 0 .. neg - 1:  o = Philox4x32-10(key = (seed low word, seed high word), counter = (t low word, t high word,
 *       e, q >> 2)); s = (o[q & 3] * n) >> 32 (the 64-bit product); unless s == i: step(cur, Y_old[s], repel);
 *   then Y_new[i] = cur.  step(cur, y, kind): dlt_c = cur_c - y_c; d2 = dlt_0 * dlt_0, then d2 = d2 + dlt_c * dlt_c for c = 1 ..;
 *     nothing happens unless d2 > 0; pb = pow(d2, b); den = a * pb + 1; coef = (((-2 * a) * b) * (pb / d2)) / den to attract,
 *     ((2 * gamma) * b) / ((0.001 + d2) * den) to repel; per coordinate g = coef * dlt_c clipped to [-4, 4], cur_c = cur_c +
 *     alpha * g.  One pow per interaction: d2^(b - 1) is pb / d2.
 *   Two differences from umap-learn's optimize_layout_euclidean, on purpose: (1) reads come from the previous epoch's
 *   positions, not from positions other threads are writing (no race, no atomic, no dependence on the schedule); the move
 *   of an edge's tail is made by the mirrored entry (j, i), which has the same weight and fires in the same epochs; (2) a
 *   vertex therefore gets 1 attraction per firing and exactly neg negatives, 1 : neg against umap-learn's 2 : neg.
 *   A call with [e0, e1) followed by one with [e1, e2) gives the bytes of one call with [e0, e2). */
int sc_fuzzy_graph(sc_ctx *ctx, double *rho_out, double *sigma_out, int64_t *n_edges_out, int64_t *n_components_out);
int sc_umap_layout(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const double *w, int64_t n, double *Y, int32_t C,
                   double a, double b, double gamma, double alpha0, int32_t neg, int32_t n_epochs, uint64_t seed, int32_t e0,
                   int32_t e1);

/* ---- N18 (extension): Pearson-residual gene selection -- spatialcore_amd.preprocessing ---------------
 * Lause, Berens & Kobak 2021, the analytic Pearson residuals of a count matrix under a negative binomial null with the
 * overdispersion theta (infinity: Poisson), restated from the published formula; parity with scanpy is not pinned.
 * X is a CANONICAL CSR (rows' columns strictly ascending inside [0, n_genes), values SC_F32 or SC_F64, finite, >= 0, at
 * least one > 0).  fp64, every multiply and add rounded separately, correctly rounded division and square root, no
 * floating-point atomics: every result is a function of the arguments alone, bit for bit.
 * sc_hvg_pearson: with s_i = the sum of row i (stored entries in index order), t_g = the sum of column g, T = sum_g t_g,
 *   p_g = t_g / T, mu = s_i * p_g, v = mu * (1 + mu * (1 / theta)), z(x) = (x - mu) / sqrt(v), the residual of a pair is
 *   r = min(max(z(x_ig), -clip), clip), and 0 where mu == 0 (an empty cell, an all-zero gene).  Nothing is densified:
 *   sum_i r = [sum over all n cells of r0 = max(z(0), -clip)] + [sum over the stored entries of r - r0], and the same for
 *   r^2 with r0^2 and r^2 - r0^2.  The first term is cut into slices of 1024 ceil(n / 2^22) cells, added in slice order;
 *   the second and t_g, q_g = sum x^2 run over the column-sorted copy in chunks of 512 entries, added in chunk order;
 *   T adds t_j + t_(j + 256) + ... per j < 256, then those 256 sums in order.  sum_out[g] = t_g, sumsq_out[g] = q_g (exact
 *   on integer counts below 2^53), resid_mean_out[g] = S1 / n, resid_var_out[g] = max(S2 / n - mean^2, 0): the population
 *   variance over all n cells.
 * Validated on the host before the first HIP call: null pointers, dtype, the canonical CSR, finite non-negative values,
 * 2 <= n <= 2^31 - 1, 1 <= n_genes <= 32768, stored entries <= 2^32 - 1, theta > 0, clip > 0 (either may be infinite). */
int sc_hvg_pearson(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                   int32_t n_genes, double theta, double clip, double *sum_out, double *sumsq_out, double *resid_mean_out,
                   double *resid_var_out);

/* ---- N19 (extension): Harmony batch correction of an embedding -- spatialcore_amd.integration --------
 * Korsunsky et al. 2019, restated from the published algorithm (harmonypy's cluster / update_R / moe_correct_ridge for ONE
 * one-hot covariate); parity with harmonypy is not pinned.  On-purpose differences: strided blocks (cell i is in block
 * i mod n_blocks) in place of a random order, per-block tables that are summed and never subtracted, the row-minimum shift
 * of the distances before exp.  fp64, no floating-point atomics, sums over cells in slices that depend on the shape alone
 * and are added in slice order: every result is a function of the arguments alone, bit for bit.  sc_harmony.hip's head
 * states the one expression order; tests/harmony_restated.py restates the algorithm.
 * sc_harmony_begin: Z[n][d] row-major (SC_F32 or SC_F64), batch[n] codes in [0, n_batches), Y[K][d] the starting centres
 *   (any scale; row-normalised here), n_blocks, sigma, theta, lamb.  Leaves on the device: Z, Zc = Z with unit rows,
 *   dist = 2 (1 - Zc Y^T), S = exp(-(dist - rowmin) / sigma), R = S / rowsum, the per-block tables O[n_blocks][K][n_batches]
 *   (O[t][k][b] = the sum of R[i][k] over the cells of block t and batch b); objective_out[0] = the objective of that state.
 *   Validated on the host before the first HIP call: null pointers, dtype, 2 <= n <= 2^31 - 1, 1 <= d <= 64,
 *   2 <= K <= min(128, n), 2 <= n_batches <= 64, 1 <= n_blocks <= min(1024, n), every code in range, every batch with a
 *   cell, Z and Y finite without an all-zero row, sigma > 0, theta >= 0, lamb > 0 (all finite).
 * sc_harmony_cluster: at most max_iter (1 .. 4096) clustering rounds.  A round: Y = the row-normalised R^T Zc (a cluster
 *   without mass keeps its centre); dist and S again; then the blocks in order, for block t: O- = the sum of the other
 *   blocks' tables in ascending order, E-_kb = (sum_b O-_kb) n_b / n, R_ik proportional to S_ik ((E-_kb + 1) / (O-_kb + 1))^theta
 *   for the block's cells, and O[t] rebuilt from them; then the objective sum R dist + sigma sum R log R + sigma theta
 *   sum_i sum_k R_ik log((O_kb(i) + 1) / (E_kb(i) + 1)).  objectives_out[r] = the objective after round r, rounds_out = the
 *   rounds done.  Stops after round r > 3 when |old - new| / |old| < epsilon with old = obj[r-1] + obj[r-2] + obj[r-3] and
 *   new = obj[r] + obj[r-1] + obj[r-2] (harmonypy's window of 3); epsilon < 0 never stops and waits for the device once.
 *   9 + 2 n_blocks launches per round.
 * sc_harmony_correct: per cluster the ridge system [[s, o^T], [o, diag(o + lamb)]] of the one-hot design, in closed form:
 *   r_b = sum_{i in b} R_ik Z_i (the original Z), r_0 = sum_b r_b, w_0 = (r_0 - sum_b o_b r_b / (o_b + lamb)) / (s - sum_b
 *   o_b^2 / (o_b + lamb)), W_kb = (r_b - o_b w_0) / (o_b + lamb), intercept dropped; Zcorr_i = Z_i - sum_k R_ik W_kb(i) and
 *   Zc = Zcorr with unit rows.
 * sc_harmony_get: one array of the resident state in the CALLER's cell order: SC_HARMONY_ZCORR / _ZC [n][d] (Zcorr is Z
 *   before the first correction), _R / _DIST [n][K], _Y [K][d], _O [n_blocks][K][n_batches], _W [K][n_batches][d] (zero
 *   before the first correction), all double; _ORDER int64[n], the cell at every position of the (block, batch, cell) sort.
 * sc_harmony_end frees the state (also done by the next sc_harmony_begin and by sc_ctx_destroy). */
#define SC_HARMONY_ZCORR 0
#define SC_HARMONY_ZC 1
#define SC_HARMONY_R 2
#define SC_HARMONY_Y 3
#define SC_HARMONY_O 4
#define SC_HARMONY_W 5
#define SC_HARMONY_ORDER 6
#define SC_HARMONY_DIST 7
int sc_harmony_begin(sc_ctx *ctx, const void *Z, int dtype, int64_t n, int32_t d, const int32_t *batch, int32_t n_batches,
                     const double *Y, int32_t K, int32_t n_blocks, double sigma, double theta, double lamb,
                     double *objective_out);
int sc_harmony_cluster(sc_ctx *ctx, int32_t max_iter, double epsilon, int32_t *rounds_out, double *objectives_out);
int sc_harmony_correct(sc_ctx *ctx);
int sc_harmony_get(sc_ctx *ctx, int32_t what, void *out);
int sc_harmony_end(sc_ctx *ctx);

/* ---- multi-hop neighbourhood shells and their aggregates (sc_hops.hip) ----------
 * CellCharter's neighbourhood aggregation (Varrone et al. 2024), restated from the published algorithm; parity with a
 * cellcharter run is not pinned.  The graph is a pattern on n cells: shell l of cell i = the cells whose shortest path
 * from i, along stored entries, has exactly l edges.  tests/hops_restated.py restates shells and aggregates.
 * sc_hop_begin: the pattern as CSR (int64 indptr[n + 1], int32 indices), 1 <= n <= 2^31 - 1, every row's columns strictly
 *   ascending inside [0, n) and off the diagonal; anything else is SC_ERR_INVALID naming the first offending row, on the
 *   host, before the first HIP call.  Leaves shell 1 (the rows themselves) resident.
 * sc_hop_next: shell l + 1 from shell l, which stays as part of the visited set (at most SC_HOP_MAX shells).  Per cell an
 *   open-addressing table of the visited cells (integer atomicCAS), in one of three places chosen by the bound
 *   1 + sum |shells 1 .. l| + sum of the degrees of shell l's members: a wavefront's LDS (bound <= SC_HOP_WAVE_KEYS), a
 *   workgroup's LDS (<= SC_HOP_WG_KEYS), global memory in batches of at most 64 MiB beyond.  Count, exclusive scan, fill,
 *   then the device-wide radix sort on (row, column): the shell is a canonical CSR whatever the class.  nnz_out = its
 *   stored entries, max_row_out = its longest row, empty_rows_out = its empty rows.  A shell whose arrays exceed the free
 *   device memory gives SC_ERR_NOMEM after the count, before anything is written; the resident shell is then unchanged.
 * sc_hop_get: the resident shell, indptr_out[n + 1] and indices_out[nnz].
 * sc_hop_aggregate: out[n][d] (fp64) over the resident shell of X[n][d] (row-major, SC_F32 widened on load, or SC_F64;
 *   finite; 1 <= d <= 64).  what = SC_HOP_MEAN: m = (sum_j x_j) / c, the sum in ascending j from 0.0, one division;
 *   SC_HOP_VAR: (sum_j x_j x_j) / c - m m, product, division and subtraction rounded one by one.  An empty shell gives
 *   zeros.  X goes to the device on the first call after sc_hop_begin and stays; a later call re-sends it only if the
 *   pointer, dtype or d differ.
 * sc_hop_times: milliseconds of the last sc_hop_next's count (bound included), fill and sort, and of the last
 *   sc_hop_aggregate's kernel (0.0 for a phase that did not run).
 * sc_hop_end frees the state (also done by the next sc_hop_begin and by sc_ctx_destroy).  No floating-point atomics:
 * every result is a function of the arguments alone, bit for bit. */
#define SC_HOP_MEAN 1
#define SC_HOP_VAR 2
#define SC_HOP_MAX 64
#define SC_HOP_WAVE_KEYS 512
#define SC_HOP_WG_KEYS 16384
int sc_hop_begin(sc_ctx *ctx, const int64_t *indptr, const int32_t *indices, int64_t n);
int sc_hop_next(sc_ctx *ctx, int64_t *nnz_out, int32_t *max_row_out, int64_t *empty_rows_out);
int sc_hop_get(sc_ctx *ctx, int64_t *indptr_out, int32_t *indices_out);
int sc_hop_aggregate(sc_ctx *ctx, const void *X, int dtype, int32_t d, int32_t what, double *out);
int sc_hop_times(sc_ctx *ctx, double *ms_out_4);
int sc_hop_end(sc_ctx *ctx);

/* ---- Gaussian mixtures (extension; restated by tests/mixture_restated.py) --------------------------------
 * sc_mixture_fit -- sklearn 1.7.2's GaussianMixture(n_components=K, covariance_type, n_init, max_iter, tol, reg_covar,
 *   init_params="kmeans", random_state).fit_predict on X[n][D] (float32 or float64; every value is widened to fp64 first
 *   and all arithmetic is fp64).  cov_type SC_MIX_FULL or SC_MIX_DIAG.  Envelope: 1 <= n <= 2^31 - 1, 1 <= D <= 256,
 *   1 <= K <= min(64, n), 1 <= n_init <= 10, max_iter >= 1, tol >= 0, reg_covar >= 0, every value finite: anything else is
 *   SC_ERR_INVALID with the argument in the message, on the host, before the first HIP call.
 *   Start (_initialize_parameters): run r takes the labels of KMeans(K, n_init=1, random_state=<the shared RandomState>)
 *   from sc_kmeans_fit's seeding and Lloyd kernels on the fp64 values: km_max_iter, km_tol and x_mean[D] (fp64) are sklearn's
 *   KMeans arguments as in sc_kmeans_fit, uniforms[n_init][1 + (K - 1) L] the draws of ONE RandomState shared by the runs,
 *   exactly as T3 documents (kmeans_draws' layout).  One-hot responsibilities, then the M-step.  K = 1 runs no k-means
 *   (x_mean and uniforms may be NULL): every responsibility is 1.
 *   M-step (_estimate_gaussian_parameters): rows are cut into slices of S rows, S = max(1024, ceil(n / smax) rounded up to
 *   32), smax = clamp(2^28 / bytes of one slice's partials, 1, 4096), the partials being K nq 64 64 8 bytes ("full", nq =
 *   nb (nb + 1) / 2, nb = ceil(D / 64)) or K D 8 bytes ("diag"): a function of (n, D, K, cov_type) alone, and the
 *   covariance partials stay within 256 MiB.  nk = (sum_i r_ik: rows ascending in a slice, slices ascending) + 10 * 2^-52,
 *   mean = (sum_i r_ik x_i, same order) / nk, weights = nk / (sum_k nk, k ascending).  Then a second pass around the NEW
 *   mean: cov_k = (sum_i r_ik (x_i - mu_k)(x_i - mu_k)^T) / nk + reg_covar I; "full": upper triangle by
 *   v_mfma_f64_16x16x4_f64, 32 rows at a time, four rows per k-step in ascending order, slices added in ascending order,
 *   then mirrored; "diag": the diagonal of the same, rows ascending, product and sum rounded separately.
 *   Precisions (_compute_precision_cholesky): cov = L L^T by right-looking column steps, P = L^-T by forward
 *   substitution in ascending order, log det = sum_j log P_jj, b = mu^T P; "diag": P = 1 / sqrt(var).  A pivot (variance)
 *   that is not finite and > 0 gives SC_ERR_ILLDEFINED (decided by a flag the host reads; the context stays usable).
 *   E-step (_estimate_log_prob_resp): q_ik = sum_j ((x_i P_k)_j - b_kj)^2 ("diag": ((x_ij - mu_kj) P_kj)^2), log p_ik =
 *   (-(D log 2 pi + q_ik) / 2 + log det_k) + log w_k; log-sum-exp as max + log sum_k exp(. - max), k ascending with Kahan's compensation;
 *   responsibilities exp(log p - max) / that sum (sklearn's exp(log p - lse) without the rounding of lse, so that a
 *   row adds up to 1 within a few ulp); label = the first largest log p.  The mean log-likelihood adds 256-row block sums
 *   (rows ascending) in two levels: 256 runs of ceil(blocks / 256) consecutive blocks, each ascending, then the runs
 *   ascending.
 *   Loop (fit_predict): prev = -inf; per iteration E-step, M-step, lb = that E-step's mean log-likelihood; converged when
 *   |lb - prev| < tol.  Runs go one after another; a later run replaces the best only on a strictly larger lb.
 *   Out, per run r: weights_out[n_init][K], means_out[n_init][K][D], covariances_out[n_init][K][D][D] ("diag":
 *   [n_init][K][D]), lower_bound_out, n_iter_out, converged_out [n_init]; *best_out.  For the best run: labels_out[n] and
 *   (may be NULL) proba_out[n][K], from one more E-step under its final parameters, and *loglik_out, that E-step's mean
 *   log-likelihood (sklearn's score(X), what bic and aic are made of).
 * sc_mixture_predict -- that last E-step for any cells under given parameters: labels_out[n], proba_out[n][K] (may be
 *   NULL), *loglik_out = the mean log-likelihood.  On the fitted cells and the fit's parameters it returns the fit's
 *   labels and responsibilities byte for byte.  Weights must be finite and > 0, means and covariances finite.
 * sc_mixture_slice_rows -- *rows_out = S, the rows per M-step slice sc_mixture_fit uses for this shape (host only, no
 *   context, no HIP call): what the tests place n around.
 * No floating-point atomics: every result is a function of the arguments alone, bit for bit. */
#define SC_MIX_FULL 0
#define SC_MIX_DIAG 1
int sc_mixture_fit(sc_ctx *ctx, const void *X, int dtype, int64_t n, int32_t D, int32_t K, int32_t cov_type, int32_t n_init,
                   int32_t km_max_iter, double km_tol, const double *x_mean, const double *uniforms, int32_t max_iter, double tol,
                   double reg_covar, double *weights_out, double *means_out, double *covariances_out, double *lower_bound_out,
                   int32_t *n_iter_out, int32_t *converged_out, int32_t *best_out, int32_t *labels_out, double *proba_out,
                   double *loglik_out);
int sc_mixture_predict(sc_ctx *ctx, const void *X, int dtype, int64_t n, int32_t D, int32_t K, int32_t cov_type, const double *weights,
                       const double *means, const double *covariances, int32_t *labels_out, double *proba_out, double *loglik_out);
int sc_mixture_slice_rows(int64_t n, int32_t D, int32_t K, int32_t cov_type, int64_t *rows_out);

/* ---- multi-GPU: the path's one collective -------------------------------
 * The reference is single-process (n_jobs=1 hard-coded at AC:580; no collective anywhere).  Here genes shard across
 * one process per GPU with no data-path communication; at the end ONE ncclAllGather over RCCL (xGMI inside a node)
 * hands every rank the per-gene rows (I, expected_I, z_score, p_value) of all shards.  RCCL is dlopen'ed on first
 * use.  Rendezvous: one rank calls sc_comm_unique_id and passes the 128 bytes to the others by any side channel
 * (spatialcore_amd/parallel.py: a file keyed by the launcher's environment); all ranks call sc_comm_create.
 * sc_allgather: host arrays; every rank contributes `count` doubles, out holds world * count, in rank order.
 * sc_allreduce_max: in-place element-wise maximum over ranks (bench: slowest rank's clock; doubles as a barrier).
 * sc_allreduce_sum_i64: in-place element-wise integer sum over ranks (permutation sharding, SURVEY 8(e) "alternative":
 *   ranks score disjoint permutation ranges and add their exceedance counts -- integers, hence exact and order-free).
 * sc_comm_info: what RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice). */
typedef struct sc_comm sc_comm;
int sc_comm_unique_id(uint8_t *id_out_128);
int sc_comm_create(sc_ctx *ctx, const uint8_t *id_128, int world, int rank, sc_comm **out);
int sc_comm_destroy(sc_comm *comm);
int sc_allgather(sc_comm *comm, const double *local, int64_t count, double *out);
int sc_allreduce_max(sc_comm *comm, double *values, int64_t count);
int sc_allreduce_sum_i64(sc_comm *comm, int64_t *values, int64_t count);
int sc_comm_info(sc_comm *comm, int *world_out, int *rank_out, int *device_out);

#ifdef __cplusplus
}
#endif
#endif /* SPATIALCORE_HIP_H */
