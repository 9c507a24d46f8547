"""Buffer-union-shrink domains over discs, restated in numpy / scipy independently of the device code (test
infrastructure; the definition is DESIGN.md 4.6e and include/spatialcore_hip.h, N7).

T = target points, d = buffer radius, s = d - m the shrink.  U = union of the closed discs of radius d about T.

* ``components``: connected components of the graph on T with an edge iff ``fl(fl(dx dx) + fl(dy dy)) <= fl((2d)(2d))``
  (``cKDTree.query_pairs`` with a slightly larger radius proposes, the project's own distance expression decides),
  each labelled by the smallest target index in it.
* ``clearance``: per query ``min(s, dist(p, boundary of U))``, or -1 outside U, from the finite candidate set -- foot
  points on the circles that contain p and the intersection points of circle pairs, each counted only if no other
  disc holds it strictly inside.  Written for any numpy float type, so that the formula's own rounding noise can be
  measured (float64 against longdouble).
* ``boundary_sample_clearance``: the same quantity from a dense sampling of the boundary, which shares nothing with
  the candidate formula but the input.
* ``assign`` / ``reduce_and_number``: the region test, the small-domain rule (``<=``) and the numbering.
"""
import numpy as np


def make_input(name):
    """The three shared inputs of the domain tests: (coordinates, target mask, d, m).  One recipe -- n uniform points on
    a square of side 10 sqrt(n), the target draw next on the same generator.  A: sparse targets, many small
    components.  B: six blobs of dense targets, the case with a long rim.  C: a denser scatter with a thin margin."""
    n, seed, d, m = {"A": (2000, 1, 12.0, 5.0), "B": (2000, 2, 15.0, 6.0), "C": (1500, 3, 8.0, 2.0)}[name]
    rng = np.random.default_rng(seed)
    L = np.sqrt(n) * 10
    xy = rng.uniform(0, L, (n, 2))
    if name == "A":
        target = rng.random(n) < 0.15
    elif name == "C":
        target = rng.random(n) < 0.3
    else:
        cen = rng.uniform(0, L, (6, 2))
        rad = rng.uniform(.08, .2, 6) * L
        in_blob = (np.linalg.norm(xy[:, None, :] - cen[None, :, :], axis=2) < rad[None, :]).any(axis=1)
        dense, sparse = rng.random(n) < 0.6, rng.random(n) < 0.01
        target = np.where(in_blob, dense, sparse)
    return xy, target, d, m


def _d2(ax, ay, bx, by):
    dx, dy = ax - bx, ay - by
    return dx * dx + dy * dy          # numpy rounds the products and the sum separately


def components(xy_t, d):
    """int32[n_t]: smallest target index of each target's component."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    xy = np.ascontiguousarray(xy_t, dtype=np.float64)
    n = xy.shape[0]
    two_d = 2.0 * d
    pairs = cKDTree(xy).query_pairs(two_d * (1.0 + 1e-9), output_type="ndarray")
    if pairs.size:
        i, j = pairs[:, 0], pairs[:, 1]
        keep = _d2(xy[i, 0], xy[i, 1], xy[j, 0], xy[j, 1]) <= two_d * two_d
        i, j = i[keep], j[keep]
    else:
        i = j = np.zeros(0, dtype=np.int64)
    g = coo_matrix((np.ones(i.size, dtype=np.int8), (i, j)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    first = np.full(lab.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return first[lab].astype(np.int32)


def _clearance_one(p, P, d, s, one):
    """p: (2,), P: (K, 2) targets within d + s of p (any superset), all in one float type; ``one`` = 1 in that type."""
    r2 = _d2(p[0], p[1], P[:, 0], P[:, 1])
    if not (r2 <= d * d).any():
        return -one
    K = P.shape[0]
    same = (P[:, None, 0] == P[None, :, 0]) & (P[:, None, 1] == P[None, :, 1])     # coincident targets: one circle
    cand, dist, gi, gj = [], [], [], []
    # foot points on the circles that contain p
    r = np.sqrt(r2)
    foot = np.flatnonzero((r > 0) & (r2 <= d * d))
    if foot.size:
        sc = d / r[foot]
        cand.append(np.stack([P[foot, 0] + sc * (p[0] - P[foot, 0]), P[foot, 1] + sc * (p[1] - P[foot, 1])], axis=1))
        dist.append(d - r[foot])
        gi.append(foot)
        gj.append(foot)
    # the two intersection points of every pair of circles
    i, j = np.triu_indices(K, 1)
    D2 = _d2(P[i, 0], P[i, 1], P[j, 0], P[j, 1])
    ok = (D2 > 0) & (D2 <= (d + d) * (d + d))
    i, j, D2 = i[ok], j[ok], D2[ok]
    if i.size:
        D = np.sqrt(D2)
        half = D / 2
        h2 = d * d - half * half
        h = np.sqrt(np.where(h2 > 0, h2, 0 * one))
        ux, uy = (P[j, 0] - P[i, 0]) / D, (P[j, 1] - P[i, 1]) / D
        mx, my = (P[i, 0] + P[j, 0]) / 2, (P[i, 1] + P[j, 1]) / 2
        for sign in (one, -one):
            v = np.stack([mx - sign * h * uy, my + sign * h * ux], axis=1)
            cand.append(v)
            dist.append(np.sqrt(_d2(p[0], p[1], v[:, 0], v[:, 1])))
            gi.append(i)
            gj.append(j)
    if not cand:
        return s
    cand, dist = np.concatenate(cand), np.concatenate(dist)
    gi, gj = np.concatenate(gi), np.concatenate(gj)
    near = dist < s
    cand, dist, gi, gj = cand[near], dist[near], gi[near], gj[near]
    if not dist.size:
        return s
    inside = _d2(cand[:, None, 0], cand[:, None, 1], P[None, :, 0], P[None, :, 1]) < d * d
    inside &= ~(same[gi] | same[gj])
    valid = ~inside.any(axis=1)
    return dist[valid].min() if valid.any() else s


def clearance(xy_t, xy_q, d, s, dtype=np.float64):
    """[n_q] in ``dtype``: min(s, distance to the boundary of U) for queries in U, -1 outside."""
    from scipy.spatial import cKDTree

    t64 = np.ascontiguousarray(xy_t, dtype=np.float64)
    q64 = np.ascontiguousarray(xy_q, dtype=np.float64)
    T, Q = t64.astype(dtype), q64.astype(dtype)
    dd, ss, one = dtype(d), dtype(s), dtype(1)
    out = np.full(Q.shape[0], -one, dtype=dtype)
    if not Q.shape[0]:
        return out
    near = cKDTree(t64).query_ball_point(q64, (d + s) * (1.0 + 1e-9))
    for k, idx in enumerate(near):
        if idx:
            out[k] = _clearance_one(Q[k], T[np.sort(idx)], dd, ss, one)
    return out


def boundary_sample_clearance(xy_t, xy_q, d, s, nang=4000):
    """The same quantity from ``nang`` points per circle, those kept that no disc holds strictly inside; a query's
    distance to the nearest kept point overestimates the true one by at most the arc spacing 2 pi d / nang."""
    from scipy.spatial import cKDTree

    T = np.ascontiguousarray(xy_t, dtype=np.float64)
    Q = np.ascontiguousarray(xy_q, dtype=np.float64)
    ang = 2.0 * np.pi * np.arange(nang) / nang
    ring = d * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    tree = cKDTree(T)
    kept = []
    for i0 in range(0, T.shape[0], 64):
        B = (T[i0:i0 + 64, None, :] + ring[None, :, :]).reshape(-1, 2)
        covered = tree.query_ball_point(B, d * (1.0 - 1e-12), return_length=True)
        kept.append(B[covered == 0])
    kept = np.concatenate(kept)
    in_u = tree.query(Q, k=1)[0] <= d
    out = np.full(Q.shape[0], -1.0)
    out[in_u] = np.minimum(s, cKDTree(kept).query(Q[in_u], k=1)[0])
    return out


def assign(xy_t, xy_q, d, s, comp_t=None, clear=None):
    """(target component ids, query component ids or -1, clearance): a query belongs to the component of a target
    within d of it iff its clearance is >= s."""
    from scipy.spatial import cKDTree

    T = np.ascontiguousarray(xy_t, dtype=np.float64)
    Q = np.ascontiguousarray(xy_q, dtype=np.float64).reshape(-1, 2)
    comp_t = components(T, d) if comp_t is None else comp_t
    clear = clearance(T, Q, d, s) if clear is None else clear
    comp_q = np.full(Q.shape[0], -1, dtype=np.int32)
    if Q.shape[0]:
        _, hit = cKDTree(T).query(Q, k=1)
        inside = clear >= s
        comp_q[inside] = comp_t[hit[inside]]
    return comp_t, comp_q, clear


def reduce_and_number(comp_t, comp_q, min_target, min_total=None):
    """(rank per target, rank per query): 1-based domain numbers, 0 = unassigned.  A component with
    n_target <= min_target (or n_total <= min_total) is dropped; the rest are numbered by assigned-cell count,
    largest first, ties to the smaller component id."""
    comp_t, comp_q = np.asarray(comp_t, dtype=np.int64), np.asarray(comp_q, dtype=np.int64)
    n = comp_t.size
    n_target = np.bincount(comp_t, minlength=n)
    n_total = n_target + np.bincount(comp_q[comp_q >= 0], minlength=n)
    keep = n_target > min_target
    if min_total is not None:
        keep &= n_total > min_total
    ids = np.flatnonzero(keep)
    order = ids[np.lexsort((ids, -n_total[ids]))]
    rank = np.zeros(n + 1, dtype=np.int64)           # (slot n serves the -1 of unassigned queries)
    rank[order] = np.arange(1, order.size + 1)
    return rank[comp_t], rank[comp_q]
