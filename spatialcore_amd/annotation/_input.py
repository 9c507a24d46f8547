"""What both annotation functions do to the expression matrix on the host: decide its state (counts or log1p(10k), the
reference's test) and hand the library a canonical CSR over the genes in use.  No value is transformed here: the
normalisation itself runs on the device."""

from __future__ import annotations

from typing import Tuple

import numpy as np
from scipy import sparse

from spatialcore_amd._sparse_input import as_csr, float_storage


def matrix_state(Xc) -> str:
    """``"counts"`` for an integer-valued matrix; otherwise the reference's log1p(10k) test (core/utils.py:
    check_normalization_status, _estimate_target_sum) on every cell instead of a sample: values in [0, 25) whose
    ``expm1`` row sums have a median in (8000, 12000) over the non-empty cells give ``"log1p"``.  Anything else raises
    the reference's ValueError."""
    data = Xc.data
    if data.size and not np.all(np.isfinite(data)):
        raise ValueError("the expression matrix contains NaN or infinite values")
    if data.size and data.min() < 0:
        raise ValueError("the expression matrix contains negative values: neither counts nor log1p(10k) data")
    if data.size == 0:
        raise ValueError("the expression matrix is all zero: there is nothing to annotate")
    if np.issubdtype(Xc.dtype, np.integer) or Xc.dtype == bool or np.array_equal(data, np.rint(data)):
        return "counts"
    target = None
    if data.max() < 25:
        E = Xc.astype(np.float64)
        E.data = np.expm1(E.data)
        sums = np.asarray(E.sum(axis=1)).ravel()
        sums = sums[sums > 0]
        target = float(np.median(sums)) if sums.size else 0.0
        if 8_000 < target < 12_000:
            return "log1p"
    raise ValueError(
        "Cannot prepare data for CellTypist.\n"
        f"  Estimated target_sum: {target if target is not None else 'N/A'}\n"
        "Provide data with:\n"
        "  1. Raw counts in .X\n"
        "  2. Or log1p(10k) normalized data in .X")


def prepare(X, cols: np.ndarray) -> Tuple[sparse.csr_matrix, str]:
    """The matrix restricted to the columns ``cols`` (ascending) as a canonical CSR without stored zeros (float32 stays
    float32, everything else becomes float64) and the library's mode: ``"counts"``, ``"log1p"`` (taken as it is) or
    ``"log1p_renorm"`` (the gene set shrank: expm1, renormalise, log1p, as the reference's annotate.py:464-514)."""
    Xc = as_csr(X)
    state = matrix_state(Xc)
    shrunk = cols.size != Xc.shape[1]
    if shrunk:
        Xc = Xc[:, cols]
    Xc = float_storage(Xc)
    Xc.eliminate_zeros()
    Xc.sort_indices()
    if Xc.shape[0] > 2**31 - 1 or Xc.nnz > 2**32 - 1:
        raise ValueError("at most 2^31 - 1 cells and 2^32 - 1 stored entries are supported")
    mode = "counts" if state == "counts" else ("log1p_renorm" if shrunk else "log1p")
    return Xc, mode
