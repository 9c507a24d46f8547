// The resident weighted graph (sc_ctx::ListGraph, c->lg) and its one owner, sc_list_graph.hip: the symmetric union of the
// dense search's lists as a CSR pattern, a caller's CSR (sc_diffmap_graph_csr), the finish that makes either the resident
// graph, and the rule for what stays valid.  Writers of the weights between the union and the finish: sc_diffmap_graph
// (sc_diffusion.hip) and sc_fuzzy_graph (sc_umap.hip).  Readers: Lanczos (sc_diffusion.hip, with its own refusal) and, through
// lg_resident, sc_diffmap_graph_get, sc_umap_layout, sc_louvain_resident_weights and sc_louvain_begin_resident.  DESIGN.md 4.6u.
#pragma once

#include "sc_ctx.h"

// the row of stored entry e: the last i with indptr[i] <= e (no row is empty)
__device__ __forceinline__ int64_t df_row_of(const int64_t *__restrict__ indptr, int64_t n, int64_t e)
{
    int64_t lo = 0, hi = n;   // indptr[lo] <= e < indptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (indptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- what invalidates what: knn.valid (the lists), lg.valid (the graph), lz.valid (the Lanczos run on it) ----
// A new search (lists_too; sc_neighbors.hip sets knn.valid itself when the search has finished), a graph from the lists
// (the lists stay) and an uploaded graph (lists_too: its vertices are not the lists' rows): nothing that stood on the old
// graph stays, and with lists_too nothing that stood on the old lists.  A cross search (sc_knn_cross) is a new search that
// never sets knn.valid: its lists (knn.cross) have query rows, not vertices, and no graph is ever built on them.
void lg_invalidate(sc_ctx *c, bool lists_too);
void lg_mark_finished(sc_ctx *c);   // lg_finish has run: the graph is the resident one; no Lanczos run is open on it
void lz_open(sc_ctx *c);            // sc_lanczos_begin has its start vector
void lz_close(sc_ctx *c);           // sc_lanczos_begin before it touches the basis, a breakdown, sc_lanczos_end

// the resident graph for a reader, or SC_ERR_STATE "<who>: no graph is resident<hint>"
int lg_resident(const sc_ctx *c, const char *who, const char *hint, const sc_ctx::ListGraph **g);

// the symmetric union of the resident lists (c->knn) as indptr / indices on the device (rows sorted by column): both
// directions of every entry as keys, one device-wide sort, the first of every run kept.  *nnz_out = its stored entries
// (after the caller's wait); lg.n becomes the lists' row count.
int lg_build_union(sc_ctx *c, long long *nnz_out);
// on the resident CSR with its weights w in place: row sums q, density D, transition matrix T and the connected
// components; then lg_mark_finished
int lg_finish(sc_ctx *c, int64_t *n_components_out);
