"""ingest restated in numpy, in the device's order (sc_knn_cross in sc_neighbors.hip; sc_cross_vote and sc_cross_regress in
sc_ingest.hip).  numpy alone: every function here runs without the library.

  cross_knn   the k reference rows smallest in (d2, j) for every query row, d2 added in column order from the c = 0 term --
              diffusion_restated.knn without its diagonal mask
  weights     uniform 1; "distance" 1 / sqrt(d2), and in a row that holds a zero distance 1 for the zero-distance entries
              and 0 for the rest
  vote        class sums and the total in list order, proba = class sum / total, the largest proba, the lowest code on ties
  regress     (sum_t w_t Y[j_t]) / (sum_t w_t), both sums in list order, the first term starting each
"""
import numpy as np


def cross_knn(Q, R, k, block=512):
    """(indices int32, d2) of the k smallest (d2, j) among the rows j of R, for every row of Q.  Each array is widened to
    float64 on its own."""
    Q = np.asarray(Q).astype(np.float64)
    R = np.asarray(R).astype(np.float64)
    nq = Q.shape[0]
    idx = np.empty((nq, k), dtype=np.int32)
    d2 = np.empty((nq, k), dtype=np.float64)
    for b in range(0, nq, block):
        q = Q[b:b + block]
        f = q[:, None, 0] - R[None, :, 0]
        acc = f * f
        for c in range(1, R.shape[1]):
            f = q[:, None, c] - R[None, :, c]
            acc = acc + f * f
        order = np.argsort(acc, axis=1, kind="stable")[:, :k]    # stable: equal distances keep index order
        idx[b:b + block] = order
        d2[b:b + block] = np.take_along_axis(acc, order, axis=1)
    return idx, d2


def weights(d2, weighting):
    """w[q][t] of the lists' entries."""
    d2 = np.asarray(d2, dtype=np.float64)
    if weighting == "uniform":
        return np.ones_like(d2)
    assert weighting == "distance"
    zero = d2 == 0.0
    with np.errstate(divide="ignore"):
        w = 1.0 / np.sqrt(d2)
    has_zero = zero.any(axis=1)
    w[has_zero] = zero[has_zero].astype(np.float64)
    return w


def vote(idx, d2, codes_ref, n_classes, weighting):
    """(label int32, conf, proba (n_query, n_classes)) of the lists."""
    codes_ref = np.asarray(codes_ref)
    nq, k = idx.shape
    w = weights(d2, weighting)
    cls = codes_ref[idx]
    total = w[:, 0].copy()
    for t in range(1, k):
        total = total + w[:, t]
    label = np.empty(nq, dtype=np.int32)
    conf = np.empty(nq, dtype=np.float64)
    proba = np.zeros((nq, n_classes), dtype=np.float64)
    for q in range(nq):
        sums = {}
        for t in range(k):
            c = int(cls[q, t])
            sums[c] = sums[c] + w[q, t] if c in sums else w[q, t]
        best, best_p = None, -1.0
        for c in sorted(sums):                     # ascending codes: a tie keeps the lowest
            p = sums[c] / total[q]
            proba[q, c] = p
            if p > best_p:
                best, best_p = c, p
        label[q], conf[q] = best, best_p
    return label, conf, proba


def regress(idx, d2, Y_ref, weighting):
    """out[q][c] of the lists; Y_ref widened to float64 first."""
    Y = np.asarray(Y_ref).astype(np.float64)
    k = idx.shape[1]
    w = weights(d2, weighting)
    num = w[:, 0, None] * Y[idx[:, 0]]
    den = w[:, 0].copy()
    for t in range(1, k):
        num = num + w[:, t, None] * Y[idx[:, t]]
        den = den + w[:, t]
    return num / den[:, None]


def uniform_count_vote(idx, codes_ref, n_classes):
    """The uniform vote from its definition: integer counts, the largest, the lowest code on ties; conf = count / k."""
    cls = np.asarray(codes_ref)[idx]
    counts = np.stack([np.bincount(row, minlength=n_classes) for row in cls])
    label = counts.argmax(axis=1).astype(np.int32)          # argmax returns the first of equal maxima
    return label, counts[np.arange(len(label)), label] / float(idx.shape[1]), counts


def kth_gap(Q, R, k):
    """Per query row: the relative gap (d2_(k+1) - d2_(k)) / d2_(k+1) between the k-th and the (k + 1)-th squared distance."""
    _, d2 = cross_knn(Q, R, k + 1)
    return (d2[:, k] - d2[:, k - 1]) / d2[:, k]
