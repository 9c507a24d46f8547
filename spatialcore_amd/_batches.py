"""The batches of an ``obs`` column, as highly_variable_genes(batch_key=...) and harmony_integrate(key=...) take them."""

from __future__ import annotations

import numpy as np
import pandas as pd


def batch_groups(adata, key, argument: str = "batch_key"):
    """[(category, its rows ascending)] in sorted category order; no missing values, at least 2 cells each."""
    if not isinstance(key, str) or key not in adata.obs:
        raise ValueError(f"{argument}={key!r} is not a column of adata.obs")
    values = np.asarray(adata.obs[key])
    if pd.isna(values).any():
        raise ValueError(f"adata.obs[{key!r}] has missing values")
    try:
        cats, codes = np.unique(values, return_inverse=True)
    except TypeError:
        raise ValueError(f"adata.obs[{key!r}] mixes values that cannot be sorted") from None
    out = []
    for b, cat in enumerate(cats):
        rows = np.flatnonzero(codes == b)
        if rows.size < 2:
            raise ValueError(f"batch {cat!r} of adata.obs[{key!r}] has {rows.size} cell; every batch needs at least 2")
        out.append((cat.item() if hasattr(cat, "item") else cat, rows))
    return out
