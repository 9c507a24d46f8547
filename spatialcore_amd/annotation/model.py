"""CellTypeModel: the arrays of a CellTypist-style model (a StandardScaler, a clip at 10, one-vs-rest logistic
regression) as plain float64 fields, stored as an ``.npz`` that is read with ``allow_pickle=False``."""

from __future__ import annotations

import os
from typing import Sequence

import numpy as np

T_MAX = 256
G_MAX = 32768


class CellTypeModel:
    """``features`` (G gene names), ``cell_types`` (T label names, sorted), ``coef`` (T x G), ``intercept`` (T),
    ``scaler_mean`` (G) and ``scaler_scale`` (G), all float64.  The decision score of a cell is
    ``intercept + coef @ min((x - scaler_mean) / scaler_scale, 10)`` on its log1p(10k) expression ``x``."""

    __slots__ = ("features", "cell_types", "coef", "intercept", "scaler_mean", "scaler_scale")

    def __init__(self, features: Sequence[str], cell_types: Sequence[str], coef, intercept, scaler_mean, scaler_scale):
        self.features = np.asarray([str(f) for f in features], dtype=str)
        self.cell_types = np.asarray([str(c) for c in cell_types], dtype=str)
        arrays = {}
        for name, a in (("coef", coef), ("intercept", intercept), ("scaler_mean", scaler_mean), ("scaler_scale", scaler_scale)):
            a = np.asarray(a)
            if a.dtype == object or not np.issubdtype(a.dtype, np.number):
                raise ValueError(f"{name} must be numeric")
            arrays[name] = np.ascontiguousarray(a, dtype=np.float64)
        G, T = self.features.size, self.cell_types.size
        if not 2 <= T <= T_MAX:
            raise ValueError(f"a model needs 2 to {T_MAX} cell types, got {T}")
        if not 1 <= G <= G_MAX:
            raise ValueError(f"a model needs 1 to {G_MAX} genes, got {G}")
        if len(set(self.features.tolist())) != G:
            raise ValueError("features must not repeat a gene")
        if len(set(self.cell_types.tolist())) != T:
            raise ValueError("cell_types must not repeat a label")
        if T == 2 and arrays["coef"].shape == (1, G):
            raise ValueError("a binary sklearn classifier stores one row of coefficients; pass one row per cell type "
                             "(np.vstack([-coef, coef]) and the intercepts likewise)")
        want = {"coef": (T, G), "intercept": (T,), "scaler_mean": (G,), "scaler_scale": (G,)}
        for name, shape in want.items():
            if arrays[name].shape != shape:
                raise ValueError(f"{name} must have shape {shape}, got {arrays[name].shape}")
            if not np.all(np.isfinite(arrays[name])):
                raise ValueError(f"{name} contains NaN or infinite values")
        if np.any(arrays["scaler_scale"] <= 0):
            raise ValueError("scaler_scale must be > 0")
        if np.any(arrays["scaler_mean"] < 0):
            raise ValueError("scaler_mean must be >= 0 (the mean of non-negative expression)")
        self.coef, self.intercept = arrays["coef"], arrays["intercept"]
        self.scaler_mean, self.scaler_scale = arrays["scaler_mean"], arrays["scaler_scale"]

    @classmethod
    def from_arrays(cls, features, cell_types, coef, intercept, scaler_mean, scaler_scale) -> "CellTypeModel":
        """From the arrays of a trained celltypist model: ``model.features``, ``model.cell_types``,
        ``model.classifier.coef_`` / ``.intercept_``, ``model.scaler.mean_`` / ``.scale_``."""
        return cls(features, cell_types, coef, intercept, scaler_mean, scaler_scale)

    def write(self, path) -> str:
        path = os.fspath(path)
        if not path.endswith(".npz"):
            raise ValueError(f"a CellTypeModel is written as .npz, got {path!r}")
        parent = os.path.dirname(path)
        if parent:
            os.makedirs(parent, exist_ok=True)
        np.savez(path, features=self.features, cell_types=self.cell_types, coef=self.coef, intercept=self.intercept,
                 scaler_mean=self.scaler_mean, scaler_scale=self.scaler_scale)
        return path

    @classmethod
    def load(cls, path) -> "CellTypeModel":
        path = os.fspath(path)
        if path.endswith((".pkl", ".pickle")):
            raise ValueError(
                f"{path!r} is a pickle: celltypist stores its models pickled, and unpickling runs whatever code the file "
                "names, so this package never does it.  Export the arrays where celltypist is installed with "
                "CellTypeModel.from_arrays(model.features, model.cell_types, model.classifier.coef_, "
                "model.classifier.intercept_, model.scaler.mean_, model.scaler.scale_).write('model.npz').")
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in cls.__slots__ if k not in z.files]
            if missing:
                raise ValueError(f"{path!r} is not a CellTypeModel file: missing {missing}")
            return cls(*(z[k] for k in cls.__slots__))

    def __repr__(self) -> str:
        return f"CellTypeModel({self.cell_types.size} cell types x {self.features.size} genes)"
