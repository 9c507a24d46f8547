// Internal definitions shared by the translation units of libspatialcore_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/spatialcore_hip.h"
#include "sc_streams.h"

#define SC_TILE 16  // genes per tile: one 128-byte fp64 row per cell and tile
#define PERM_CHUNK 128  // permutations per pipeline stage (generator scan -> swaps -> scoring)

void sc_set_error(const char *fmt, ...);

#define SC_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess) {                                                             \
            sc_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__,  \
                         __LINE__);                                                          \
            return e__ == hipErrorOutOfMemory ? SC_ERR_NOMEM : SC_ERR_HIP;                   \
        }                                                                                    \
    } while (0)

#define SC_TRY(call)              \
    do {                          \
        int rc__ = (call);        \
        if (rc__ != SC_OK) return rc__; \
    } while (0)

#define SC_REQUIRE(cond, code, ...)    \
    do {                               \
        if (!(cond)) {                 \
            sc_set_error(__VA_ARGS__); \
            return (code);             \
        }                              \
    } while (0)

// Device buffer that only ever grows and frees itself with its owner: the context, a resident problem or a call
// (DESIGN.md "Device memory").  It remembers the counter its bytes were charged to and takes them off again when it dies;
// a buffer that never allocated makes no HIP call.  Moving leaves the source empty; copying is not possible.
struct DBuf {
    void *p = nullptr;
    size_t cap = 0;
    int64_t *acct = nullptr;   // the counter `cap` is charged to (the one handed to ensure)
    DBuf() = default;
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
    DBuf(DBuf &&o) noexcept : p(o.p), cap(o.cap), acct(o.acct) { o.p = nullptr, o.cap = 0; }
    DBuf &operator=(DBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap, acct = o.acct;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DBuf() { release(); }
    int ensure(size_t bytes, int64_t *charge_to);
    void release();   // gives the memory back early; the buffer is empty again and may grow anew
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Waits for the context stream when its scope ends.  A call whose buffers (or host vectors that an asynchronous copy
// still reads) may be in use on an early return declares one AFTER them, so that the wait runs before they go.
struct StreamWaitOnExit {
    hipStream_t &stream;
    ~StreamWaitOnExit() { (void)hipStreamSynchronize(stream); }
};

struct KTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double ms = 0.0;
    int64_t launches = 0;
    KTimer() = default;
    KTimer(const KTimer &) = delete;
    ~KTimer();   // destroys the events of both lists
};

// The one owner of a context's streams (sc_streams.h: roles, placements; sc_api.hip).  A role's stream is created on
// demand, the way the placement says: plain = hipStreamNonBlocking on the normal level, priority-spread = the same flag
// on the role's level.  The placement is chosen once per context by permgen_place_streams (sc_permgen_phi.hip).
constexpr unsigned SR_MASK_GENERATOR = (1u << SR_EXPAND) | (1u << SR_PREP0) | (1u << SR_PREP1) | (1u << SR_PREP2) | (1u << SR_PREP3);
constexpr unsigned SR_MASK_PIPELINE = ((1u << SR_COUNT) - 1u) & ~(1u << SR_MOMENTS);   // what a pipeline's drain waits for
struct StreamTable {
    hipStream_t s[SR_COUNT] = {};
    int placement = SC_PLACE_PLAIN;
    int level[SR_COUNT] = {};            // priority-spread: StreamLevel per role
    int ensure(int role);                // create the role's stream if it does not exist yet
    int sync(unsigned roles);            // wait for the existing streams among `roles` (bit r = role r)
    // Take another placement.  Existing streams must be idle: they are destroyed and created again where they belong.
    int replace(int new_placement, const int *new_level);
    StreamTable() = default;
    StreamTable(const StreamTable &) = delete;
    ~StreamTable();                      // destroys the streams
};

// The numpy-exact permutation generator's state in the context (sc_permgen.h): scratch, its events, its form, counters
struct PermGen {
    DBuf J, raw, out, bits, enter, sblk;  // accepted j per step, raw 32-bit stream, scan state + chunk ranges, per block: accept masks, entering counts, entry state
    DBuf flags;       // hand-over words between the chain workgroup and the preparation launches (sc_permgen_phi.hip)
    DBuf desc, tbits, events, hard;  // block-parallel scan: per-block descriptors + gap-transfer tables (ring), hard flags
    DBuf seglist;                    // ... per unit in flight: [count | first blocks of the segments k_phi_compose builds]
    DBuf seg, ctbits, segmode;       // ... segments of prepared blocks: descriptors + composed tables (ring), per-block mode
    StreamTable *streams = nullptr;  // the context's table: SR_PREP0 .. 3 (the chip prepares blocks there ahead of the chain), SR_EXPAND
    hipEvent_t ev[34] = {};          // [0 .. 3] k_seg_fill of a chunk done on preparation stream q, [32] raw stream written, [33] chain of a chunk done
    int mode = 0;                    // 0 auto, 1 sequential scan only, 2 fault injection (tests)
    bool streams_serial = false;     // a wait on a hand-over word gave up once: the streams of this process do not run concurrently (profiler
                                     // that serialises kernels, shared hardware queues) -- later jobs take the sequential scan at once
    bool probed = false;             // the placement ladder and its probe ran (once per context, before the first block-parallel job)
    std::string note;                // why the generator left the block-parallel form, if it did (sc_ctx_permgen_note)
    std::string placement_note;      // the block-parallel form on another placement than plain streams (sc_ctx_permgen_form; no degradation)
    std::string form;                // scratch of sc_ctx_permgen_form
    int64_t jobs_parallel = 0, jobs_sequential = 0, fallbacks = 0;  // generator jobs by scan form
    int64_t blocks_prepared = 0, blocks_chain = 0;  // block-parallel jobs: blocks resolved by table lookup / by the chain workgroup
    int ensure(bool preparation)     // create what is missing: the events, and (preparation) the preparation streams
    {
        if (preparation)
            for (int r = SR_PREP0; r <= SR_PREP3; ++r) SC_TRY(streams->ensure(r));
        for (hipEvent_t &e : ev)
            if (!e) SC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return SC_OK;
    }
    int sync() { return streams ? streams->sync(SR_MASK_GENERATOR) : SC_OK; }   // wait for the generator's own streams
    // sc_ctx_set_permgen_mode.  Re-arms: a context that fell back to the sequential scan after one stalled hand-over (a transient: GPU
    // shared with another process, a profiler pass) goes through the placement ladder again and may return to the block-parallel form
    void rearm(int new_mode) { mode = new_mode; streams_serial = false; probed = false; note.clear(); placement_note.clear(); }
    PermGen() = default;
    PermGen(const PermGen &) = delete;
    ~PermGen()                       // waits for its streams (the table's, which outlives it), drops the events; then the buffers go
    {
        (void)sync();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// Moran's partial sums as a ring of slices (sc_moran.hip): scoring launch k of a job writes slice k % MORAN_RING on the
// context stream, and its finalise reads that slice on the side stream (sc_ctx::stream_out) beside launch k + 1
constexpr int MORAN_RING = 3;
struct MoranRing {
    size_t slice = 0;                   // doubles per slice: one chunk's partial sums (sized by moran_prepare)
    int64_t launches = 0;               // scoring launches of the job so far (0 again once moran_finish has waited for them)
    hipEvent_t scored[MORAN_RING] = {}; // behind the scoring launch that last wrote the slice
    hipEvent_t done[MORAN_RING] = {};   // behind the finalise that last read it
};

struct PermPipe;   // a generator job in flight (sc_permgen.h, sc_perm.hip; begun by sc_moran_seeded_begin, consumed by _finish)

// A problem kept on the device between a _begin and an _end (annotation training, PCA, Louvain, Harmony).  Its type is
// complete only in its own file; the context owns it through this base.
struct Resident {
    virtual ~Resident() = default;
};
template <class T> T *resident(const std::unique_ptr<Resident> &r) { return static_cast<T *>(r.get()); }

// Teardown (sc_ctx_destroy, then the members in reverse declaration order) relies on that order in three places:
// `mem` is declared before every DBuf, since each takes its bytes off it when it dies; `streams` and `timers` are
// declared before `pg`, every DBuf and the resident problems, so that the buffers go first, then the generator (which
// waits for its streams and drops its events), then the timer events, and the streams last.  sc_ctx_destroy has waited
// for the work in flight before any of this runs.  A new DBuf member needs no line anywhere else.
struct sc_ctx {
    int device = 0;
    int64_t mem = 0;  // bytes allocated through DBuf
    std::unique_ptr<PermPipe> pipe;  // the generator / consumer pipeline begun by sc_moran_seeded_begin, until _finish
    StreamTable streams;            // every stream of the context, by role; the names below are its entries
    hipStream_t &stream = streams.s[SR_SCORE];
    hipStream_t &stream2 = streams.s[SR_CHAIN];   // fused permutation/Moran pipeline: rejection scan runs ahead here
    hipStream_t &stream3 = streams.s[SR_SWAP_A];  // ... and the Fisher-Yates swaps of the scanned chunk here
    hipStream_t &stream4 = streams.s[SR_SWAP_B];  // ... alternating with this one
    hipStream_t &stream_out = streams.s[SR_FINALISE];  // r04: what leaves a pipeline beside it: result copies issued by a helper thread (sc_local_moran_seeded,
                                                       // sc_local_stat_seeded); Moran's finalise launches, beside the next chunk's scoring (sc_moran.hip: MoranRing)
    hipStream_t &stream_px = streams.s[SR_EXPAND];     // the generator verifies + expands a finished chunk here, beside the next chunk's chain
    hipStream_t *const stream_pg = streams.s + SR_PREP0;   // [4]: its preparation streams
    bool timing = true;
    KTimer timers[SC_K_END_];
    PermGen pg;       // the numpy-exact permutation generator's state
    sc_ctx();         // (sc_api.hip, where PermPipe is complete)
    ~sc_ctx();
    sc_ctx(const sc_ctx &) = delete;

    // ---- points (kNN / radius) ----
    int64_t pts_n = 0;
    DBuf px, py;        // SoA coordinates in original order
    DBuf sx, sy, sid;   // coordinates / original ids sorted by bin
    DBuf bin_start;     // [nbins + 1]
    DBuf bin_keys, bin_keys2, sid2, cub_tmp;
    int nbx = 0, nby = 0;
    double gx0 = 0, gy0 = 0, gh = 0;
    int64_t knn_n = 0;
    int knn_k = 0;
    DBuf knn_idx, knn_rd;  // [n][k] device result of the last sc_knn_2d
    hipEvent_t knn_done = nullptr;      // ... recorded behind a search whose result was not fetched (sc_knn_fetch)
    DBuf knn_hd, knn_hi;   // k > 32: the per-query candidate heaps, [slot][query]
    // the pending radius count: > 0 from a sc_radius_count_2d until the next sc_bin_points (any neighbour search), since
    // the fill pass walks the bins the rows were counted on
    double radius = -1.0;
    DBuf rad_indptr;  // [n+1] int64 of that count
    long long rad_nnz = 0;   // ... and its last entry
    // ---- Ripley's K pair list (sc_labelperm.hip): the unordered pairs within the largest radius, kept BESIDE the graph ----
    // Positions are those of the bin-sorted order of the points (sid: position -> cell), so the list is valid exactly as
    // long as the bins are those it was built from: sc_bin_points clears rp_valid, and every neighbour search goes through it.
    bool rp_valid = false;
    int64_t rp_n = 0, rp_pairs = 0;   // cells, stored pairs (each unordered pair once: row position < column position)
    int rp_radii = 0;
    DBuf rp_cnt, rp_indptr, rp_row, rp_col, rp_bin, rp_rank;   // per-position counts / offsets, pair ends, radius bin (1 byte), cell -> position
    // ---- Ripley's G neighbour lists (sc_ripley_g.hip): the ORDERED pairs within the largest radius as one row per position,
    // kept beside the graph and beside the pair list above, valid exactly as long as the bins are (sc_bin_points clears rg_valid)
    bool rg_valid = false;
    int64_t rg_n = 0, rg_entries = 0;   // cells, stored entries (every ordered pair once)
    int rg_radii = 0;
    DBuf rg_cnt, rg_indptr, rg_col, rg_bin, rg_rank;   // per-position counts / row offsets, column position, radius bin (1 byte, non-decreasing within a row), cell -> position
    // ---- spatial domains (sc_domains.hip): union-find parents by target index, per-query component and clearance ----
    DBuf dm_parent, dm_qcomp, dm_clear;
    // ---- rank sums (sc_ranksum.hip): group-sorted cell order in pieces, per-piece partials, the pair arrays (double
    // buffered for the sort), per-gene offsets / negative counts / flags, the result tables ----
    DBuf rs_order, rs_pstart, rs_pgroup, rs_gpiece, rs_groupn, rs_psum, rs_pnnz, rs_poff, rs_goff, rs_neg, rs_flag;
    DBuf rs_keys, rs_keys2, rs_pay, rs_pay2, rs_gkey, rs_gkey2, rs_idx, rs_idx2, rs_tmp;
    DBuf rs_rank2, rs_tie, rs_nnz, rs_sum;
    // ---- thresholds (sc_threshold.hip): the sorted fp64 scores of the last sc_ks_prepare, for sc_ks_argmax ----
    DBuf th_sorted;
    int64_t th_n = 0;
    // ---- the dense search (sc_neighbors.hip): the fp64 features and neighbour lists of the last sc_knn_dense[_gram].  Written
    // by sc_neighbors.hip alone; read by lg_build_union (idx), sc_diffmap_graph (X, d2, d) and sc_fuzzy_graph (idx, d2, k).
    // What invalidates what among knn.valid, lg.valid and lz.valid: the functions of sc_list_graph.h.
    // sc_knn_cross uses the same buffers for the lists of nq query rows (Q) among the n reference rows (X): it leaves
    // `cross` set and `valid` clear, so that no reader of a self graph takes them; sc_cross_vote and sc_cross_regress
    // (sc_ingest.hip) read idx, d2, n, nq and k under `cross`.  Every search clears both flags when it begins ----
    struct DenseKnn {
        int64_t n = 0;      // rows of the lists; after a cross search: the reference rows, the lists' indices are below it
        int d = 0, k = 0;   // columns of X (the features padded to a multiple of 8), list length
        bool valid = false;
        DBuf X, raw, idx, d2, pidx, pd2;        // [n][d] fp64, the upload, [n][k] result, [split][query][k] partial lists
        DBuf gnorm, gkept, gcnt, glo, grows;    // the Gram filter: row norms, kept candidates [n][L], their counts, the L-th keys, [count | uncertified rows]
        int64_t nq = 0;     // a cross search: rows of the lists
        bool cross = false;
        DBuf Q, qraw, qnorm;                    // ... its queries [nq][d] fp64, their upload, their norms
    } knn;
    // ---- ingest (sc_ingest.hip): the codes or the values of the reference rows that the cross lists gather from ----
    DBuf ig_ref, ig_raw, ig_label, ig_conf, ig_out;
    // ---- the resident weighted graph (sc_list_graph.h).  Written by sc_list_graph.hip (the union, the upload, the finish;
    // `valid` by its validity functions alone) and by the two kernels that fill `w` between the union and the finish
    // (sc_diffmap_graph, sc_fuzzy_graph, which also set nnz); read by Lanczos, sc_umap_layout and Louvain through lg_resident ----
    struct ListGraph {
        int64_t n = 0, nnz = 0;   // vertices (lg_build_union: knn.n; sc_diffmap_graph_csr: its n) and stored entries
        bool valid = false;
        DBuf indptr, indices, w;            // CSR, rows sorted by column; the weights
        DBuf T, q, parent, flag;            // lg_finish: transition matrix, [row sums | density], union-find, root count
        DBuf keys, keys2, pay, pay2, cnt, off;   // lg_build_union: (row << 32 | column) keys, the sort's payload, first-of-run flags and offsets
    } lg;
    // ---- diffusion's own (sc_diffusion.hip writes and reads it; `valid` through lz_open / lz_close of sc_list_graph.h): the
    // local scales of sc_diffmap_graph, and the Lanczos run on lg's transition matrix ----
    struct Lanczos {
        int64_t m = 0, max_basis = 0;   // steps taken, basis size
        bool valid = false;
        DBuf s2;                        // sc_diffmap_graph's local scales
        DBuf V, wv, part, coef, ab, Y, S, res;   // basis [max_basis + 1][n], work vector, chunk partials, coefficients, alpha | beta, Ritz vectors, their coefficients, residuals
    } lz;
    // ---- UMAP's work buffers (sc_umap.hip writes and reads them; nothing else does) ----
    struct UmapWork {
        DBuf rho, sigma, dsum;                  // sc_fuzzy_graph: first non-zero distance, bandwidth, [row sums of the distances | chunk sums | their total]
        DBuf lip, lix, lw, ly0, ly1, lmax;      // sc_umap_layout: a caller's CSR, the two position buffers, the bits of w_max
    } um;
    // ---- annotation (sc_annotate.hip): the training problem kept on the device between sc_annot_train_begin and _end ----
    std::unique_ptr<Resident> an;        // AnnotTrain
    // ---- PCA (sc_pca.hip): the matrix kept on the device between sc_pca_begin and sc_pca_end ----
    std::unique_ptr<Resident> pca;       // PcaState
    // ---- Louvain (sc_louvain.hip): the level graphs and the partition kept on the device between sc_louvain_begin and _end ----
    std::unique_ptr<Resident> louvain;   // LouvainState
    // ---- Harmony (sc_harmony.hip): the embedding, the assignments and the block tables between sc_harmony_begin and _end ----
    std::unique_ptr<Resident> harmony;   // HarmonyState
    // ---- neighbourhood shells (sc_hops.hip): the pattern, the shells so far and X between sc_hop_begin and _end ----
    std::unique_ptr<Resident> hops;      // HopState

    // ---- graph (CSR, rows sorted by column) + transpose ----
    int64_t g_n = 0, g_nnz = 0;
    DBuf g_indptr, g_indices, g_data;
    double g_uniform_w = 0.0;   // > 0: every stored weight equals this value (kNN graphs: 1 / k); 0: weights differ
    int64_t g_deg_max = 0;      // longest row
    bool g_regular = false;     // every row has g_deg_max entries
    bool gt_valid = false;
    DBuf gt_indptr, gt_indices, gt_data, gt_cursor;
    // the full moments (transpose + reverse-edge search: 6 ms at 1M x 15) may be in flight on a side stream, begun by the
    // scoring's set-up so that they leave its serial prelude (sc_graph.hip: graph_moments_begin / graph_moments)
    hipStream_t &stream_m = streams.s[SR_MOMENTS];
    hipEvent_t mom_ready = nullptr, mom_done = nullptr;
    bool mom_pending = false;
    double *mom_host = nullptr;      // pinned: per-block partials of k_moments
    int mom_blocks = 0;
    DBuf gt_tmp, mom_dev;            // the transpose's own scan scratch (cub_tmp belongs to the neighbour search); k_moments' partials
    bool s0_valid = false, s0_only_valid = false;   // all three moments / s0 alone (k_weight_sum) are those of the active graph
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;  // graph moments (valid with s0_valid)
    // a processing order with spatial locality for kernels that read neighbours' rows (local Moran): the bin-sorted
    // order of the points the graph was built from (identity for a graph of unknown geometry).  Results never depend on it.
    DBuf g_order, g_rank, g_indices_r, g_w32, g_erow_r;   // [n] sorted position -> cell, [n] cell -> position, [nnz] rank of the column, float weights, [nnz] rank of the row
    bool g_order_captured = false, g_order_ready = false;

    // ---- expression tiles ----
    int64_t e_n = 0, e_genes = 0, e_tiles = 0;
    int e_dtype = SC_F64;  // dtype of the matrix the tiles were loaded from (the reference's float32 paths depend on it)
    DBuf X, Z, Lag;      // [tile][cell][16] fp64: raw, centred/standardised, lagged
    DBuf X32;            // the raw values again in the narrowest exact type, one 128-byte row per cell and gene group:
                         // 32 float (float32-exact values), 64 uint16 (counts < 65536) or 128 uint8 (counts < 256) per row
    int nib_groups = 0;         // > 0: the last moran_prepare built the 4-bit source (256 nibble slots per row) with this many row groups
    DBuf nib_map;               // ... its slot map: [padded genes] slot of the gene's high nibble (-1: none) | the genes that have one
    bool lag_u16 = false;       // the last moran_prepare left Lag as 16-bit neighbour sums ([group][cell][64 words]; uint8 source only)
    int narrow_bits = 64;       // element width of the narrow copy the last moran_prepare built: 8, 16, 32 (64: none, the fp64 Z tiles are gathered)
    int n_cus = 0;              // compute units of the device (filled on first use)
    int score_leave_cus = 0;    // compute units the persistent scoring kernel leaves empty (> 0 only while a generator runs beside it)
    int source_bits_min = 8;    // (4: the nibble source, opt-in -- measured slower at the step level) narrowest source the scoring kernels may gather (sc_ctx_set_moran_source_bits)
    int last_source_bits = 0;   // ... and what the last scoring launch gathered (64 = fp64 kernel)
    DBuf e_tmp_indptr, e_tmp_indices, e_tmp_data, e_colmap;
    DBuf g_mean, g_var, g_z2, g_scale, g_Inum, g_I, red_tmp;  // per padded gene
    DBuf g_slag;         // sum_j lag_g[j] per padded gene (lattice genes: the exact integer sum of the neighbour sums)
    // Integer-lattice genes (DESIGN.md "Ties"): integer counts on a graph whose weights are all equal.  Their statistic
    // is scored as the exact integer T_p = sum_j S_j x[inv_p(j)] (S = unweighted neighbour sums; every product and partial
    // sum is an integer < 2^53, so the fp64 arithmetic is exact in any order) and #{T_p >= T_obs} is decided on integers.
    DBuf g_xsum, g_flags, g_xmax;      // per padded gene: raw column sum, value-class bits (k_gene_stats), largest count
    DBuf g_lat, g_meanc, g_seff, g_corr, g_thr;  // lattice flag (0 / 1), mean used for centring (0 for lattice genes),
                                                 // sims = seff * (sum - corr), threshold the count compares against
    DBuf sims_raw;                     // the sums themselves (lattice genes: T_p), same layout as sims
    bool lat_any = false;

    // ---- permutation table ----
    int64_t p_n = 0, p_count = 0, p_stride = 0;  // row stride in elements (multiple of 32)
    DBuf perm;
    DBuf perm_flag;
    DBuf inv;                      // inverse permutations, same layout as perm (rows valid on demand)
    int64_t inv_rows_valid = 0;    // leading rows of c->inv known to be the inverses of the active table's rows
    bool perm_forward_valid = true; // c->perm holds the active table (false: only its inverse, c->inv, was generated)
    bool perm_bijective = false;   // the active table is known to hold true permutations
    bool perm_checked = false;     // ... or was checked and is not

    // ---- Moran / Lee work buffers ----
    DBuf partial, sims, counts, sim_sum, sim_sumsq;   // partial: MORAN_RING slices
    MoranRing ring;
    // everybody's scratch (Lee, the label-permutation tests, the graph builders, the per-cell statistics): an entry point
    // lays them out as it likes, and their contents are not kept from one entry point to the next
    DBuf scratch_a, scratch_b, scratch_out, scratch_idx;
    DBuf lee_U, lee_Zc, lee_Uc, lee_part, lee_obs, lee_cnt, lee_rowmap, lee_lperm;  // Lee's own (sc_lee*.hip)
    // the per-cell (LISA) statistics (sc_local_prepare.hip, sc_local_stats.hip)
    bool lm_valid = false;   // z / lag / statistic / count words of the last sc_local_moran* or sc_local_stat* are still resident
    int64_t lm_perms = 0;    // ... with this many permutations
    int lm_stat = 0;         // ... and belong to this statistic: 0 local Moran, SC_LOCAL_GETIS / SC_LOCAL_GEARY
    bool lm_star = false;    // ... Getis-Ord: Gi* (the graph holds the self edges)
    DBuf lm_out;             // row-major staging of one output array for the helper thread's device-to-host copies (the _seeded calls)
    DBuf lm_ys;              // the permuted z rows (or uint8 code rows) of a batch of permutations, in the graph's processing order (also sc_lee_local*)
    DBuf lm_tab;             // code rows: z and w z per (gene, value)
    // first half of the Moran preparation, enqueued ahead of the generator by sc_moran_seeded_begin (sc_moran.hip)
    bool prep_early = false;         // ... is in flight / done for the resident expression and graph
    void *prep_host = nullptr;       // pinned: [weight-sum partials | xsum | flags | xmax]
    size_t prep_host_cap = 0;
    int prep_s0_blocks = 0;
    DBuf s0_tmp;
    DBuf np_cnt, np_comp, np_leaves, np_leafsum;  // numpy-order column sums: block counts, compacted values, leaf table, leaf sums
};

// Drops a resident problem, if there is one: waits for the context stream, whose work may still use its buffers and host
// vectors, then frees it.  The one way out for an _end, a new _begin, a _begin that fails half-way and a failed level.
inline void sc_resident_drop(sc_ctx *c, std::unique_ptr<Resident> &r)
{
    if (!r) return;
    (void)hipStreamSynchronize(c->stream);
    r.reset();
}

struct KernelTimerScope {
    sc_ctx *c;
    int id;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    KernelTimerScope(sc_ctx *ctx, int kid, hipStream_t on = nullptr);
    ~KernelTimerScope();
};

// generator / consumer pipeline (sc_perm.hip): table 0 = permutation rows, 1 = inverse rows only, 2 = both
constexpr int PIPE_AHEAD = 3;                      // launch units the generator's preparation runs ahead of its chain inside the pipeline
constexpr int64_t PIPE_TAIL[] = {96, 48, 24};      // permutations of the tapering last chunks (sc_perm.hip: pipe_begin)
constexpr int64_t PIPE_TAIL_TOTAL = 96 + 48 + 24;
int pipe_begin(sc_ctx *c, const uint64_t *state6, int64_t n, int64_t n_perm, int table, int units_ahead, PermPipe &pp,
               int64_t chunks_ahead, const std::function<int()> &after_first_chunk = nullptr);
// the consumer's set-up in two callbacks (either may be empty): `enqueue` must not wait for the device, `complete` may
int pipe_consume(sc_ctx *c, PermPipe &pp, uint64_t *state6, const std::function<int()> &enqueue,
                 const std::function<int()> &complete, const std::function<int(int64_t, int64_t)> &score);
void pipe_drain(sc_ctx *c, PermPipe &pp);
void sc_perm_pipe_abort(sc_ctx *c);    // drain and drop c->pipe (no results)
int sc_perm_pipeline(sc_ctx *c, uint64_t *state6, int64_t n, int64_t n_perm, int table, int units_ahead,
                     const std::function<int()> &enqueue, const std::function<int()> &complete,
                     const std::function<int(int64_t, int64_t)> &score);
// Runs attempt(); if the block-parallel scan failed its verification, runs undo() (may be empty) and then attempt() once
// more with the sequential scan.  The generator's mode is the caller's again on return, on every path.
int permgen_rerun_on_failure(sc_ctx *c, const std::function<int()> &attempt, const std::function<int()> &undo);
int sc_perm_forward_ensure(sc_ctx *c);  // materialise c->perm from c->inv after a pipeline that only made the inverse
int sc_perm_table_is_bijective(sc_ctx *c, int64_t n_perm, bool *bijective);   // inverse rows of an uploaded table + the check
int invert_rows(sc_ctx *c, int64_t p0, int64_t p1, hipStream_t s);   // inverse rows [p0, p1) of the active table on stream s
int sc_perm_alloc(sc_ctx *c, int64_t n, int64_t n_perm);
// rows [0, n_perm) of the allocated table <- counter-based permutations p_first .. (sc_perm_counter.hip), on stream s
int sc_perm_counter_rows(sc_ctx *c, uint64_t seed, int64_t n, int64_t p_first, int64_t n_perm, hipStream_t s);

int sc_timer_collect(sc_ctx *c);
// ---- expression tiles (sc_expr.hip), all enqueued on c->stream ----
enum { OP_ID = 0, OP_SQ = 1, OP_MUL = 2, OP_NZ = 3, OP_SQC = 4 };   // what expr_colsum adds up (k_colsum_partial)
int expr_colsum(sc_ctx *c, int op, const double *A, const double *B, double *out, double div, double *out_raw = nullptr);
int expr_colsum_chunks(sc_ctx *c, const double *partial, int chunks, double *out, double div = 1.0, double *out_raw = nullptr);
int expr_moments(sc_ctx *c);                       // mean (+ raw column sums), z2 = sum (X - mean)^2, var = z2 / n
int expr_write_z(sc_ctx *c, const double *centre);   // Z = X - centre (per gene)
int sc_expr_zscores(sc_ctx *c);  // Z = (X - mean) / population sd per gene (0 for zero variance), variances in g_var
int expr_gene_stats(sc_ctx *c);  // value classes and largest counts of the loaded genes into c->g_flags / c->g_xmax
int expr_pack_narrow(sc_ctx *c, int bits);   // c->X32 = the raw values as uint8 / uint16 / float32 rows
// Lag = W Z on any CSR over the cells; unit[gene] != 0 (optional): that gene's rows are summed with weight 1
int sc_lag_tiles(sc_ctx *c, const DBuf &indptr, const DBuf &indices, const DBuf &data, const double *Z, double *out,
                 const double *unit = nullptr);

// 64-bit masks and per-lane variable shifts built from 32-bit instructions whose shift amounts are IN RANGE by
// construction.  r02 finding (ISA diff in r03): the one instruction that produced wrong values
// next to kernels of other hardware queues was a v_lshlrev_b64 whose per-lane amount register held 0 - r (the compiler's
// form of (64 - r) & 63, legal only through the instruction's implicit 6-bit masking of the amount); the right shift by
// r itself, in the same kernel, never failed.  Device code therefore keeps per-lane 64-bit shifts out of the ISA: these
// helpers compile to v_lshlrev_b32 / v_lshrrev_b32 / v_alignbit_b32 with amounts masked to [0, 31] in the source.
#if defined(__HIPCC__)
__device__ __forceinline__ uint64_t sc_low_mask64(uint32_t d)   // the d low bits set, d in [0, 64]
{
    const uint32_t part = (1u << (d & 31u)) - 1u;
    const uint32_t lo = d >= 32u ? 0xffffffffu : part;
    const uint32_t hi = d >= 64u ? 0xffffffffu : (d > 32u ? part : 0u);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t sc_bit64(uint32_t pos)      // 1 << pos, pos in [0, 63]
{
    const uint32_t b = 1u << (pos & 31u);
    const uint32_t lo = (pos & 32u) ? 0u : b, hi = (pos & 32u) ? b : 0u;
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t sc_shr64(uint64_t x, uint32_t pos)   // x >> pos, pos in [0, 63]
{
    uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32);
    if (pos & 32u) { xl = xh; xh = 0u; }
    const uint32_t k = pos & 31u;
    return ((uint64_t)(xh >> k) << 32) | __builtin_amdgcn_alignbit(xh, xl, k);
}
#endif

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t align_up64(int64_t a, int64_t b) { return ceil_div64(a, b) * b; }
// the graph's processing order for kernels that walk n cells (nullptr: none captured for a graph of this size, input order)
static inline const int32_t *sc_processing_order(const sc_ctx *c, int64_t n)
{
    return (c->g_order_captured && c->g_n == n && c->g_order.p) ? c->g_order.as<int32_t>() : nullptr;
}

// ---- implemented across translation units ----
// ---- neighbour searches (sc_search.hip) ----
// bins the points for a neighbour search (sx / sy / sid / bin_start; bins of side >= min_h, about target_per_bin points each).
// The only function that replaces the bins, so it invalidates what is only meaningful on the bins it replaces: the pending
// radius count (radius, rad_indptr), the Ripley pair list (rp_valid) and the Ripley's G neighbour lists (rg_valid).
int sc_bin_points(sc_ctx *c, const double *xy, int64_t n, double target_per_bin, double min_h);
struct BinGrid;                         // sc_search.h
BinGrid sc_bin_grid(const sc_ctx *c);   // the bins of the last sc_bin_points, as kernels take them
int sc_window_rings(const sc_ctx *c, double radius);   // rings of bins around a point's own bin that cover its closed ball (window_walk)
// offsets[0 .. n] = exclusive sums of counts[0 .. n] (counts[n] = 0), and *total = offsets[n]: enqueued on c->stream, the caller waits
int sc_counts_to_offsets(sc_ctx *c, long long *counts, long long *offsets, int64_t n, long long *total);
// the all-pairs entry points' host check (sc_pairwise_2d, sc_pair_table_2d, sc_cooccurrence_2d): SC_ERR_INVALID naming
// the entry point, the point set and the index of the first coordinate that is not finite
int require_finite_points(const char *who, const char *set, const double *xy, int64_t n);
// ---- active graph (sc_graph.hip) ----
void sc_graph_drop(sc_ctx *c);          // the active graph is gone (before its arrays are replaced or overwritten)
int sc_graph_ensure_transpose(sc_ctx *c);
int sc_graph_ensure_s0(sc_ctx *c);
int sc_graph_weight_sum_blocks(const sc_ctx *c);
int sc_graph_weight_sum_launch(sc_ctx *c, double *pinned_out);                 // s0 without a host wait: launch + copy ...
void sc_graph_weight_sum_collect(sc_ctx *c, const double *partial, int blocks);  // ... and the addition after the caller's synchronisation
int sc_graph_moments_begin(sc_ctx *c);   // start the full moments on the side stream (no host wait); collected by sc_graph_moments
void sc_graph_moments_drain(sc_ctx *c);  // wait for a begun computation (before the graph's arrays are replaced)
int sc_graph_capture_order(sc_ctx *c, int64_t n);  // called by the graph setters
int sc_graph_ensure_order(sc_ctx *c);           // rank / relabelled columns / float weights, built on first use
int sc_perm_generate_device(sc_ctx *c, uint64_t *state6, int64_t n, int64_t n_perm);
// sc_kmeans_fit's seeding and Lloyd passes for n_init runs (same arguments), keeping EVERY run's final labels:
// labels_dev[n_init][n] is a device array, written on c->stream (sc_kmeans.hip)
int sc_kmeans_run_labels(sc_ctx *c, const void *X, int dtype, int64_t n, int32_t C, int32_t K, int32_t n_init,
                         int32_t max_iter, double tol, const void *x_mean, const double *uniforms, int32_t *labels_dev);
void sc_launch_spmv_vec(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const double *w,
                        const double *x, double *y, int64_t n);
