"""Unsupervised graph clustering of the cells on the GPU."""

from .communities import louvain

__all__ = ["louvain"]
