"""The Wilcoxon rank-sum tables of rank_genes_groups restated with scipy.stats.rankdata: the yardstick of sc_ranksum and of
wilcoxon_tables.  Nothing here shares code with the package: ranks come from rankdata over ALL ranked cells (zeros
included), tie sums from np.unique over all values, the adjustment from a plain loop."""
import numpy as np
from scipy import stats
from scipy.stats import rankdata


def dense(X):
    return np.asarray(X.todense()) if hasattr(X, "todense") else np.asarray(X)


def integer_tables(X, code, n_groups):
    """What sc_ranksum returns for the (n, G) matrix X and the codes (-1: not ranked), with Python ints for the tie sums."""
    X = dense(X).astype(np.float64)
    code = np.asarray(code)
    ranked = code >= 0
    Xr, cr = X[ranked], code[ranked]
    G = X.shape[1]
    rank2 = np.zeros((G, n_groups), dtype=np.int64)
    nnz = np.zeros((G, n_groups), dtype=np.int64)
    sums = np.zeros((G, n_groups), dtype=np.float64)
    tie_nonzero, tie_all = [], []
    for g in range(G):
        x = Xr[:, g]
        r2 = 2.0 * rankdata(x) if x.size else np.zeros(0)
        assert (r2 == np.rint(r2)).all()
        for k in range(n_groups):
            sel = cr == k
            rank2[g, k] = int(r2[sel].sum())          # integers below 2^53: exact in any order
            nnz[g, k] = int((x[sel] != 0).sum())
            sums[g, k] = x[sel].sum()
        vals, counts = np.unique(x, return_counts=True)
        tie_all.append(sum(int(t) ** 3 - int(t) for t in counts))
        tie_nonzero.append(sum(int(t) ** 3 - int(t) for v, t in zip(vals, counts) if v != 0))
    return {"rank2": rank2, "tie_nonzero": np.array(tie_nonzero, dtype=object), "tie_all": tie_all, "nnz": nnz, "sums": sums,
            "n_neg": (Xr < 0).sum(axis=0).astype(np.int64), "group_n": np.bincount(cr, minlength=n_groups).astype(np.int64)}


def integer_tables_bincount(X, code, n_groups):
    """integer_tables for many groups: the same dict, one np.bincount per gene and table instead of a mask per (gene,
    group).  The weights of ``rank2`` are the integers 2 * rank, and every partial sum of them stays below
    N (N + 1) < 2^53, so the float64 accumulator of bincount is exact.  ``sums`` is not taken with bincount: its running
    sum in cell order is up to n_k * eps * sum |x| away from the pairwise x[sel].sum() of integer_tables, which is no
    relative bound at all once a group's values cancel.  The cells are sorted by group once (stably: cell order inside a
    group) and every occupied group's slice is summed as integer_tables sums it."""
    X = dense(X).astype(np.float64)
    code = np.asarray(code)
    ranked = code >= 0
    Xr, cr = X[ranked], code[ranked].astype(np.int64)
    N, G = Xr.shape
    assert N * (N + 1) < 2 ** 53
    group_n = np.bincount(cr, minlength=n_groups).astype(np.int64)
    by_group = np.argsort(cr, kind="stable")
    ends = np.cumsum(group_n)
    occupied = [(k, int(ends[k] - group_n[k]), int(ends[k])) for k in np.flatnonzero(group_n)]
    rank2 = np.zeros((G, n_groups), dtype=np.int64)
    nnz = np.zeros((G, n_groups), dtype=np.int64)
    sums = np.zeros((G, n_groups), dtype=np.float64)
    tie_nonzero, tie_all = [], []
    for g in range(G):
        x = Xr[:, g]
        r2 = 2.0 * rankdata(x) if x.size else np.zeros(0)
        assert (r2 == np.rint(r2)).all()
        rank2[g] = np.bincount(cr, weights=r2, minlength=n_groups).astype(np.int64)
        nnz[g] = np.bincount(cr[x != 0], minlength=n_groups)
        xs = x[by_group]
        for k, a, b in occupied:
            sums[g, k] = xs[a:b].sum()
        vals, counts = np.unique(x, return_counts=True)
        tie_all.append(sum(int(t) ** 3 - int(t) for t in counts))
        tie_nonzero.append(sum(int(t) ** 3 - int(t) for v, t in zip(vals, counts) if v != 0))
    return {"rank2": rank2, "tie_nonzero": np.array(tie_nonzero, dtype=object), "tie_all": tie_all, "nnz": nnz, "sums": sums,
            "n_neg": (Xr < 0).sum(axis=0).astype(np.int64), "group_n": group_n}


def benjamini_hochberg(p):
    m = len(p)
    order = sorted(range(m), key=lambda i: (p[i], i))
    adj = [0.0] * m
    running = 1.0
    for rank in range(m, 0, -1):
        i = order[rank - 1]
        running = min(running, p[i] * m / rank)
        adj[i] = min(running, 1.0)
    return np.array(adj)


def group_table(X, code, k, *, tie_correct=False, corr_method="benjamini-hochberg", rankby_abs=False, n_genes=None,
                log1p_base=None):
    """Rows of group k against all other ranked cells: (order, scores float32, logfoldchanges float32, pvals, pvals_adj,
    pts, pts_rest); score = (R - n1 (N + 1) / 2) / sqrt(c n1 m (N + 1) / 12)."""
    X = dense(X).astype(np.float64)
    code = np.asarray(code)
    ranked = code >= 0
    Xr, own = X[ranked], code[ranked] == k
    N, G = Xr.shape
    n1 = int(own.sum())
    m = N - n1
    score, lfc, pts, pts_rest = np.zeros(G), np.zeros(G), np.zeros(G), np.zeros(G)
    scale = 1.0 if log1p_base is None else np.log(log1p_base)
    with np.errstate(divide="ignore", invalid="ignore"):
        for g in range(G):
            x = Xr[:, g]
            R = rankdata(x)[own].sum()
            c = 1.0
            if tie_correct:
                _, counts = np.unique(x, return_counts=True)
                T = sum(int(t) ** 3 - int(t) for t in counts)
                c = 1.0 - T / (N ** 3 - N)
            sd = np.sqrt(c * (n1 * m * (N + 1) / 12.0))
            z = (R - n1 * (N + 1) / 2.0) / sd
            score[g] = 0.0 if np.isnan(z) else z
            lfc[g] = np.log2((np.expm1(x[own].mean() * scale) + 1e-9) / (np.expm1(x[~own].mean() * scale) + 1e-9))
            pts[g] = (x[own] != 0).mean()
            pts_rest[g] = (x[~own] != 0).mean()
    pvals = 2.0 * stats.norm.sf(np.abs(score))
    pvals[np.isnan(pvals)] = 1.0
    padj = np.minimum(pvals * G, 1.0) if corr_method == "bonferroni" else benjamini_hochberg(list(pvals))
    key = np.abs(score) if rankby_abs else score
    order = np.array(sorted(range(G), key=lambda i: (-key[i], i)), dtype=np.int64)[: (G if n_genes is None else n_genes)]
    return {"order": order, "scores": score[order].astype(np.float32), "logfoldchanges": lfc[order].astype(np.float32),
            "pvals": pvals[order], "pvals_adj": padj[order], "pts": pts, "pts_rest": pts_rest,
            "score64": score, "pvals_all": pvals}
