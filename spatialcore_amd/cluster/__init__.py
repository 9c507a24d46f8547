"""Unsupervised clustering of the cells on the GPU: graph communities and Gaussian mixtures (4.6y)."""

from .communities import louvain
from .mixture import gaussian_mixture, gaussian_mixture_autok, predict_gaussian_mixture

__all__ = ["louvain", "gaussian_mixture", "predict_gaussian_mixture", "gaussian_mixture_autok"]
