"""What nmf, pca and annotation do to the expression matrix on the host before the library sees it: resolve the genes and
hand over a canonical CSR (sorted columns, no duplicates, no stored zeros) over them.  No value is transformed here."""

from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
from scipy import sparse


def gene_columns(adata, genes) -> Tuple[List[str], np.ndarray]:
    """Names as morans_i resolves them (None: every gene, a string: that gene) and their columns, in the order given."""
    if genes is None:
        names = list(adata.var_names)
    elif isinstance(genes, str):
        names = [genes]
    else:
        names = [str(g) for g in genes]
    if not names:
        raise ValueError("genes must name at least one gene")
    missing = set(names) - set(adata.var_names)
    if missing:
        raise ValueError(f"Genes not found in adata.var_names: {sorted(missing)[:10]}")
    if len(set(names)) != len(names):
        raise ValueError("genes must not repeat a gene")
    if len(names) > 32768:
        raise ValueError(f"at most 32768 genes are supported, got {len(names)}")
    return names, np.asarray([adata.var_names.get_loc(g) for g in names], dtype=np.intp)


def as_csr(X, cols: Optional[np.ndarray] = None, real: bool = False):
    """The 2-D matrix (scipy sparse of any format, or dense) as a CSR that shares nothing with the caller's, restricted to
    ``cols`` if given.  A dense matrix must be numeric or, with ``real``, real."""
    if sparse.issparse(X):
        if X.ndim != 2:
            raise ValueError("the expression matrix must be 2-D")
        Xc = X.tocsr()
        if cols is not None:
            Xc = Xc[:, cols]
        return Xc.copy() if Xc is X or Xc.data is getattr(X, "data", None) else Xc
    A = np.asarray(X)
    if A.ndim != 2:
        raise ValueError("the expression matrix must be 2-D")
    if not (np.issubdtype(A.dtype, np.number) or A.dtype == bool) or (real and np.issubdtype(A.dtype, np.complexfloating)):
        raise ValueError(f"the expression matrix must be {'real' if real else 'numeric'}, got {A.dtype}")
    return sparse.csr_matrix(A if cols is None else A[:, cols])


def float_storage(Xc):
    """float32 stays float32, every other type becomes float64; duplicates are summed, which sorts every row's columns."""
    dtype = np.float32 if Xc.dtype == np.float32 else np.float64
    if Xc.dtype != dtype:
        Xc = Xc.astype(dtype)
    Xc.sum_duplicates()
    return Xc


def canonical_csr(X, cols: np.ndarray, n_vars: int, *, negative: Optional[str] = None, all_zero: Optional[str] = None,
                  real: bool = False):
    """The matrix restricted to ``cols`` as a canonical CSR without stored zeros, and its dtype (float32 or float64).  It
    must be finite; ``negative`` and ``all_zero`` are the messages that refuse a negative value and a matrix without a
    non-zero (None: legal).  The caller's matrix is never modified."""
    identity = cols.size == n_vars and np.array_equal(cols, np.arange(n_vars))
    Xc = float_storage(as_csr(X, None if identity else cols, real))
    if Xc.nnz and not np.all(np.isfinite(Xc.data)):
        raise ValueError("the expression matrix contains NaN or infinite values")
    if negative is not None and Xc.nnz and Xc.data.min() < 0:
        raise ValueError(negative)
    Xc.eliminate_zeros()
    if all_zero is not None and Xc.nnz == 0:
        raise ValueError(all_zero)
    return Xc, Xc.dtype.type
