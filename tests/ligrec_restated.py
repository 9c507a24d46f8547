"""Plain numpy / Python-int restatement of the ligand-receptor permutation test (include/spatialcore_hip.h, N10).

Definition.  Gene g carries a shift s_g: 0 when every value is an integer in [0, 2^32), else 32 - e_g with e_g the smallest
integer such that max |x| < 2^e_g.  A value x enters as the integer q = rint(x * 2^s_g).  S[c][g] = sum of q over the
cells of cluster c, N[c][g] = #{cells of c with x > 0}, n_c = cells of c.  Under the labels labels[perm_p] the table is
S_p.  For interaction (L, R) and the ordered cluster pair (a, b) permutation p counts when

    2^s_R * n_b * (S_p[a][L] - S[a][L])  +  2^s_L * n_a * (S_p[b][R] - S[b][R])  >=  0,

decided here with Python integers (both powers of two divided by the smaller one, which keeps the sign).
means = (m_L,a + m_R,b) / 2 with m = float(S) * 2^-s / n_c in float64 (0 for an empty cluster), 0 where either mean is <= 0;
pvalues = count_ge / n_perms, NaN where N[a][L] / n_a < threshold or N[b][R] / n_b < threshold (float64 division).
"""
import math

import numpy as np


def shifts(X):
    """s_g of every column of the dense matrix X, by the definition above."""
    out = []
    for g in range(X.shape[1]):
        col = [float(v) for v in X[:, g]]
        top = max((abs(v) for v in col), default=0.0)
        if all(v >= 0 and v < 2.0 ** 32 and v == math.floor(v) for v in col):
            out.append(0)
            continue
        e = math.frexp(top)[1]          # top = m * 2^e with 0.5 <= m < 1: the smallest e with top < 2^e
        assert top < 2.0 ** e and not top < 2.0 ** (e - 1)
        out.append(32 - e)
    return np.array(out, dtype=np.int32)


def quantise(X, s):
    """q = rint(x * 2^s_g) as int64 (round half to even; every |q| must stay below 2^32)."""
    q = np.rint(np.ldexp(np.asarray(X, dtype=np.float64), np.asarray(s, dtype=np.int64)[None, :]))
    assert np.all(np.abs(q) < 2.0 ** 32)
    return q.astype(np.int64)


def group_sums(Q, labels, K):
    """S[c][g] = sum of Q over the cells with label c (int64: the test sizes stay far from 2^63)."""
    S = np.zeros((K, Q.shape[1]), dtype=np.int64)
    np.add.at(S, np.asarray(labels), Q)
    return S


def tables(X, codes, K, s):
    """(S, N, n_c) under the observed labels."""
    Q = quantise(X, s)
    S = group_sums(Q, codes, K)
    N = group_sums((np.asarray(X) > 0).astype(np.int64), codes, K)
    return S, N, np.bincount(codes, minlength=K).astype(np.int64)


def null_sums(X, codes, K, s, perms):
    """S_p for every row of the permutation table: the labels of the cells are codes[perm_p]."""
    Q = quantise(X, s)
    return np.stack([group_sums(Q, np.asarray(codes)[p], K) for p in perms]) if len(perms) else np.zeros((0, K, X.shape[1]), np.int64)


def count_ge(S, Sp, n_c, s, pairs):
    """count_ge[i][a][b] = #{p : the comparison above holds}; object arrays: every product and sum is a Python integer."""
    K = S.shape[0]
    So, Spo, no = S.astype(object), Sp.astype(object), n_c.astype(object)
    out = np.zeros((len(pairs), K, K), dtype=np.int64)
    for i, (L, R) in enumerate(pairs):
        low = min(int(s[L]), int(s[R]))
        wl, wr = 2 ** (int(s[R]) - low), 2 ** (int(s[L]) - low)
        dl = Spo[:, :, L] - So[None, :, L]                      # [p][a]
        dr = Spo[:, :, R] - So[None, :, R]                      # [p][b]
        v = dl[:, :, None] * (wl * no)[None, None, :] + dr[:, None, :] * (wr * no)[None, :, None]
        out[i] = np.asarray(v >= 0, dtype=np.int64).sum(axis=0) if len(Sp) else 0
    return out


def means_pvalues(S, N, n_c, s, pairs, cluster_pairs, ge, n_perms, threshold):
    """(means, pvalues) over interactions x the listed ordered cluster pairs, one Python float at a time; ge is
    count_ge[i][a][b] for all clusters.  pvalues is None for n_perms = 0."""
    means = np.zeros((len(pairs), len(cluster_pairs)))
    pvals = np.full((len(pairs), len(cluster_pairs)), np.nan)

    def mean(c, g):
        return math.ldexp(float(int(S[c, g])), -int(s[g])) / float(n_c[c]) if n_c[c] else 0.0

    def kept(c, g):
        return bool(n_c[c]) and float(N[c, g]) / float(n_c[c]) >= threshold

    for i, (L, R) in enumerate(pairs):
        for j, (a, b) in enumerate(cluster_pairs):
            ml, mr = mean(a, L), mean(b, R)
            means[i, j] = (ml + mr) / 2 if (ml > 0 and mr > 0) else 0.0
            if n_perms > 0 and kept(a, L) and kept(b, R):
                pvals[i, j] = int(ge[i, a, b]) / n_perms
    return means, (pvals if n_perms > 0 else None)


def adjust(pvals, method, axis):
    """Bonferroni / Benjamini-Hochberg over the non-NaN entries of every column (axis "clusters": one cluster pair, its
    interactions) or every row (axis "interactions"), one family at a time."""
    p = np.array(pvals, dtype=np.float64)
    if method is None:
        return p
    families = [(slice(None), j) for j in range(p.shape[1])] if axis == "clusters" else [(i, slice(None)) for i in range(p.shape[0])]
    for fam in families:
        v = p[fam].copy()
        idx = [k for k in range(v.size) if not math.isnan(v[k])]
        m = len(idx)
        if method == "bonferroni":
            for k in idx:
                v[k] = min(v[k] * m, 1.0)
        else:
            ranked = sorted(idx, key=lambda k: v[k])
            running = math.inf
            adj = {}
            for rank in range(m, 0, -1):
                k = ranked[rank - 1]
                running = min(running, v[k] * m / rank)
                adj[k] = min(running, 1.0)
            for k in idx:
                v[k] = adj[k]
        p[fam] = v
    return p


def restated(X, codes, K, pairs, perms, threshold=0.01, cluster_pairs=None):
    """Everything at once on a dense matrix X (cells x genes), integer labels, interactions as pairs of column numbers and
    a permutation table (rows of cell indices)."""
    X = np.asarray(X)
    s = shifts(X)
    S, N, n_c = tables(X, codes, K, s)
    Sp = null_sums(X, codes, K, s, perms)
    ge = count_ge(S, Sp, n_c, s, pairs)
    if cluster_pairs is None:
        cluster_pairs = [(a, b) for a in range(K) for b in range(K)]
    means, pvals = means_pvalues(S, N, n_c, s, pairs, cluster_pairs, ge, len(perms), threshold)
    return {"shift": s, "sum": S, "nnz": N, "group_n": n_c, "null_sums": Sp, "count_ge": ge, "means": means, "pvalues": pvals}
