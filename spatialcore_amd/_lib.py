"""ctypes binding of libspatialcore_hip.so (include/spatialcore_hip.h).

There is no CPU fallback anywhere in this package: if the shared library is missing, or no gfx950
device is visible, the first call that needs the GPU raises.
"""

from __future__ import annotations

import ctypes
import os
import threading
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint64, c_void_p
from typing import Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SPATIALCORE_HIP_LIB: another build of the same library -- the sanitizer build of `make asan`, a build of another commit)
LIB_PATH = os.environ.get("SPATIALCORE_HIP_LIB") or os.path.join(_HERE, "libspatialcore_hip.so")

SC_OK, SC_ERR_INVALID, SC_ERR_STATE, SC_ERR_HIP, SC_ERR_NOMEM, SC_ERR_EMPTY, SC_ERR_ILLDEFINED = 0, 1, 2, 3, 4, 5, 6
SC_F32, SC_F64 = 0, 1
K_MORAN_PERM, K_LAG, K_KNN, K_PERMGEN, K_LEE_PERM, K_PERM_SCAN, K_PERM_SWAP = 0, 1, 2, 3, 4, 5, 6
K_KMEANS_SEED, K_KMEANS_LLOYD = 7, 8
K_RANK_EMIT, K_RANK_SORT, K_RANK_RUNS = 9, 10, 11
K_THRESH_SCORE, K_THRESH_SORT, K_THRESH_KS, K_GMM_EM, K_GMM_POST = 12, 13, 14, 15, 16
K_COOCCUR = 17
K_LIGREC = 18
K_RIPLEY_G_LIST, K_RIPLEY_G_RELABEL, K_RIPLEY_G_COUNT = 19, 20, 21
K_NMF_SETUP, K_NMF_W, K_NMF_H, K_NMF_ERR = 22, 23, 24, 25
K_DIFF_KNN, K_DIFF_GRAPH, K_DIFF_SPMV, K_DIFF_ORTH = 26, 27, 28, 29
K_ANNOT_SETUP, K_ANNOT_ROWS, K_ANNOT_GRAD, K_ANNOT_LINE, K_ANNOT_PREDICT, K_ANNOT_STEP = 30, 31, 32, 33, 34, 35
K_PCA_SETUP, K_PCA_GRAM, K_PCA_PROJECT = 36, 37, 38
K_LOUVAIN_MOVE, K_LOUVAIN_LEVEL = 39, 40
K_NEIGHBORS_GRAM = 41
K_UMAP_GRAPH, K_UMAP_LAYOUT = 42, 43
K_HVG_SETUP, K_HVG_DENSE, K_HVG_SPARSE = 44, 45, 46
K_MIX_ESTEP, K_MIX_MSTEP = 47, 48
K_INGEST = 49
CROSS_WEIGHTINGS = {"uniform": 0, "distance": 1}   # SC_CROSS_UNIFORM / SC_CROSS_DISTANCE
MIX_COVARIANCES = {"full": 0, "diag": 1}   # SC_MIX_FULL / SC_MIX_DIAG
MIX_D_MAX, MIX_K_MAX, MIX_N_INIT_MAX = 256, 64, 10   # sc_mixture_fit's limits
HOP_AGGREGATIONS = {"mean": 1, "var": 2}   # SC_HOP_MEAN / SC_HOP_VAR
HOP_MAX, HOP_WAVE_KEYS, HOP_WG_KEYS = 64, 512, 16384   # SC_HOP_MAX, SC_HOP_WAVE_KEYS, SC_HOP_WG_KEYS
HARMONY_ARRAYS = {"Zcorr": 0, "Zc": 1, "R": 2, "Y": 3, "O": 4, "W": 5, "order": 6, "dist": 7}   # sc_harmony_get's codes
ANNOT_MODES = {"counts": 0, "log1p": 1, "log1p_renorm": 2}   # sc_annot_*'s input states
NMF_LOSSES = {"frobenius": 2, "kullback-leibler": 1}   # sc_nmf_fit's codes (sklearn's beta)
METAGENE_METHODS = ("shifted_geometric_mean", "geometric_mean", "arithmetic_mean", "median", "minimum")   # sc_metagene_score's codes

# every symbol include/spatialcore_hip.h declares: (name, argtypes); restype is always int
LOCAL_STATS = {"getis": 1, "geary": 2}   # SC_LOCAL_GETIS / SC_LOCAL_GEARY
_P = c_void_p
SYMBOLS = {
    "sc_version": [],
    "sc_device_count": [POINTER(c_int)],
    "sc_ctx_create": [c_int, POINTER(c_void_p)],
    "sc_ctx_destroy": [_P],
    "sc_ctx_sync": [_P],
    "sc_ctx_kernel_time": [_P, c_int, POINTER(c_double), POINTER(c_int64)],
    "sc_ctx_reset_timers": [_P],
    "sc_ctx_set_timing": [_P, c_int],
    "sc_ctx_set_permgen_mode": [_P, c_int],
    "sc_ctx_permgen_note": [_P, POINTER(c_char_p)],
    "sc_ctx_probe_streams": [_P, _P, _P],
    "sc_ctx_permgen_form": [_P, c_int64, POINTER(c_char_p)],
    "sc_ctx_set_moran_source_bits": [_P, c_int],
    "sc_ctx_moran_source_bits": [_P, _P],
    "sc_ctx_moran_lag_bits": [_P, _P],
    "sc_ctx_moran_row_groups": [_P, _P],
    "sc_ctx_permgen_stats": [_P, _P, _P, _P, _P, _P],
    "sc_ctx_device_mem": [_P, POINTER(c_int64)],
    "sc_ctx_device_free": [_P, POINTER(c_int64)],
    "sc_debug_copy": [_P, c_int, c_int64, _P, c_int64],   # buffers: 0 J, 1 raw stream, 2 accept masks, 3 entering counts, 4 block states, 5 scan state, 6 table, 7 inverse table
    "sc_knn_2d": [_P, _P, c_int64, c_int, c_int, _P, _P],
    "sc_knn_fetch": [_P, _P, _P],
    "sc_radius_count_2d": [_P, _P, c_int64, c_double, _P],
    "sc_radius_fill_2d": [_P, c_int64, _P],
    "sc_graph_set_csr": [_P, _P, _P, _P, c_int64, c_int64],
    "sc_graph_from_knn": [_P, c_double],
    "sc_graph_get": [_P, _P, _P, _P],
    "sc_graph_shape": [_P, POINTER(c_int64), POINTER(c_int64)],
    "sc_graph_moments": [_P, POINTER(c_double), POINTER(c_double), POINTER(c_double)],
    "sc_expr_set_csr": [_P, _P, _P, _P, c_int, c_int64, c_int64, _P, c_int64],
    "sc_expr_set_dense": [_P, _P, c_int, c_int64, c_int64, _P, c_int64],
    "sc_expr_stats": [_P, _P, _P],
    "sc_perm_numpy_host": [_P, c_int64, c_int64, _P],
    "sc_perm_generate": [_P, _P, c_int64, c_int64, _P],
    "sc_perm_set": [_P, _P, c_int64, c_int64],
    "sc_perm_generate_counter": [_P, ctypes.c_uint64, c_int64, c_int64, c_int64, _P],
    "sc_perm_counter_host": [ctypes.c_uint64, c_int64, c_int64, c_int64, _P],
    "sc_moran": [_P, c_int64, _P, _P, _P, _P, _P],
    "sc_moran_seeded": [_P, _P, c_int64, _P, _P, _P, _P, _P],
    "sc_moran_seeded_begin": [_P, _P, c_int64, c_int64, c_int64],
    "sc_moran_seeded_finish": [_P, _P, _P, _P, _P, _P, _P],
    "sc_moran_seeded_abort": [_P],
    "sc_lee": [_P, _P, _P, _P, c_int64, c_int64, _P, _P, _P],
    "sc_lee_seeded": [_P, _P, _P, _P, c_int64, c_int64, _P, _P, _P],
    "sc_lee_shared": [_P, _P, _P, c_int32, _P, c_int32, c_int64, _P, _P, _P],
    "sc_lee_observed_f32": [_P, _P, _P, c_int64, _P, _P, _P],
    "sc_local_moran": [_P, c_int64, c_int64, _P, _P, _P, _P, _P],
    "sc_local_moran_seeded": [_P, _P, c_int64, _P, _P, _P, _P, _P],
    "sc_local_moran_hist": [_P, _P],
    "sc_local_moran_classify": [_P, _P, _P, _P, c_float, _P, _P, _P],
    "sc_local_stat": [_P, c_int32, c_int32, c_int64, c_int64, _P, _P, _P, _P, _P, _P],
    "sc_local_stat_seeded": [_P, c_int32, c_int32, _P, c_int64, _P, _P, _P, _P, _P, _P],
    "sc_local_stat_hist": [_P, _P],
    "sc_local_stat_classify": [_P, _P, _P, _P, c_float, _P, _P, _P],
    "sc_lee_local": [_P, c_int32, c_int32, c_int64, c_int64, _P, _P, _P, _P],
    "sc_lee_local_seeded": [_P, _P, c_int32, c_int32, c_int64, c_int64, _P, _P, _P, _P, _P, _P],
    "sc_nearest_2d": [_P, _P, c_int64, _P, c_int64, _P, _P],
    "sc_pairwise_2d": [_P, _P, c_int64, _P, c_int64, POINTER(c_double), POINTER(c_double)],
    "sc_nearest_excluding_2d": [_P, _P, _P, c_int64, _P, _P, c_int64, _P, _P],
    "sc_pair_table_2d": [_P, _P, _P, c_int32, _P, _P, c_int32, _P, _P],
    "sc_profile_counts": [_P, _P, c_int64, c_int32, _P, POINTER(c_int64)],
    "sc_enrichment_counts": [_P, _P, c_int64, c_int32, c_int64, c_int64, _P],
    "sc_enrichment_counter": [_P, _P, c_int64, c_int32, ctypes.c_uint64, c_int64, c_int64, c_int64, _P, _P],
    "sc_ripley_build": [_P, _P, c_int64, _P, c_int32, _P],
    "sc_ripley_counts": [_P, _P, c_int64, c_int32, c_int64, c_int64, _P],
    "sc_ripley_counter": [_P, _P, c_int64, c_int32, ctypes.c_uint64, c_int64, c_int64, c_int64, _P, _P],
    "sc_ripley_g_build": [_P, _P, c_int64, _P, c_int32, _P],
    "sc_ripley_g_counts": [_P, _P, c_int64, c_int32, c_int64, c_int64, _P],
    "sc_ripley_g_counter": [_P, _P, c_int64, c_int32, ctypes.c_uint64, c_int64, c_int64, c_int64, _P, _P],
    "sc_cooccurrence_2d": [_P, _P, _P, c_int32, _P, c_int32, _P],
    "sc_ligrec_counts": [_P, _P, c_int64, c_int32, _P, _P, _P, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P],
    "sc_ligrec_counter": [_P, _P, c_int64, c_int32, _P, _P, _P, c_int64, ctypes.c_uint64, c_int64, c_int64, c_int64, _P, _P, _P, _P],
    "sc_domains_2d": [_P, _P, c_int64, _P, c_int64, c_double, c_double, _P, _P, _P],
    "sc_ranksum": [_P, _P, c_int64, c_int32, _P, _P, _P, _P, _P, _P],
    "sc_kmeans_fit": [_P, _P, c_int, c_int64, c_int32, c_int32, c_int32, c_int32, c_double, _P, _P, _P, _P,
                      POINTER(c_double), _P, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)],
    "sc_metagene_score": [_P, _P, c_int, c_int64, c_int32, c_int32, c_double, _P, _P, _P, _P],
    "sc_ks_prepare": [_P, _P, c_int, c_int64, c_double, _P, c_int32, _P, _P, _P],
    "sc_ks_argmax": [_P, c_double, c_double, POINTER(c_int64), POINTER(c_double), POINTER(c_double)],
    "sc_ks_classify": [_P, _P, c_int, c_int64, c_double, c_double, _P, _P, POINTER(c_int64)],
    "sc_gmm_fit": [_P, _P, c_int, c_int64, c_int32, c_int32, c_int32, c_double, _P, _P, c_int32, c_double, c_double,
                   _P, _P, _P, _P, _P, _P, _P, POINTER(c_int32)],
    "sc_gmm_posterior": [_P, _P, c_int, c_int64, c_int32, _P, _P, _P, _P, c_int32, c_double, _P, _P, POINTER(c_int64)],
    "sc_nmf_fit": [_P, _P, _P, _P, c_int, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_double, _P, _P, _P,
                   POINTER(c_int32), POINTER(c_int32), POINTER(c_double)],
    "sc_nmf_fit_graph": [_P, _P, _P, _P, c_int, c_int64, c_int32, c_int32, _P, _P, _P, c_double, c_int32, c_double, _P, _P, _P, _P,
                         POINTER(c_int32), POINTER(c_int32), POINTER(c_double), POINTER(c_double)],
    "sc_knn_dense": [_P, _P, c_int, c_int64, c_int32, c_int32, c_int32, _P, _P],
    "sc_knn_dense_gram": [_P, _P, c_int, c_int64, c_int32, c_int32, c_int32, c_int32, _P, _P, _P],
    "sc_knn_cross": [_P, _P, c_int, c_int64, _P, c_int, c_int64, c_int32, c_int32, c_int32, c_int32, _P, _P, _P],
    "sc_cross_vote": [_P, _P, c_int32, c_int32, _P, _P, _P],
    "sc_cross_regress": [_P, _P, c_int, c_int32, c_int32, _P],
    "sc_diffmap_graph": [_P, _P, POINTER(c_int64), POINTER(c_int64)],
    "sc_diffmap_graph_csr": [_P, _P, _P, _P, c_int64, POINTER(c_int64)],
    "sc_diffmap_graph_get": [_P, _P, _P, _P, _P],
    "sc_fuzzy_graph": [_P, _P, _P, POINTER(c_int64), POINTER(c_int64)],
    "sc_umap_layout": [_P, _P, _P, _P, c_int64, _P, c_int32, c_double, c_double, c_double, c_double, c_int32, c_int32, c_uint64,
                       c_int32, c_int32],
    "sc_lanczos_begin": [_P, _P, c_int64],
    "sc_lanczos_run": [_P, c_int32, _P, _P, POINTER(c_int64)],
    "sc_lanczos_ritz": [_P, _P, c_int64, c_int32, _P, _P, _P],
    "sc_lanczos_end": [_P],
    "sc_annot_predict": [_P, _P, _P, _P, c_int, c_int64, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P],
    "sc_annot_transform": [_P, _P, c_int, c_int64, c_int32, _P],
    "sc_annot_train_begin": [_P, _P, _P, _P, c_int, c_int64, c_int32, c_int32, c_int32, _P, _P, _P, _P],
    "sc_annot_train_forward": [_P, _P, _P, c_int32],
    "sc_annot_train_grad": [_P, _P, _P],
    "sc_annot_train_line": [_P, _P, _P, _P],
    "sc_annot_train_step": [_P, _P],
    "sc_annot_train_end": [_P],
    "sc_pca_begin": [_P, _P, _P, _P, c_int, c_int64, c_int32, c_int32, c_double],
    "sc_pca_values": [_P, _P],
    "sc_pca_gram": [_P, _P, _P],
    "sc_pca_project": [_P, _P, _P, c_int32, c_int, _P],
    "sc_pca_end": [_P],
    "sc_hvg_pearson": [_P, _P, _P, _P, c_int, c_int64, c_int32, c_double, c_double, _P, _P, _P, _P],
    "sc_harmony_begin": [_P, _P, c_int, c_int64, c_int32, _P, c_int32, _P, c_int32, c_int32, c_double, c_double, c_double, _P],
    "sc_harmony_cluster": [_P, c_int32, c_double, _P, _P],
    "sc_harmony_correct": [_P],
    "sc_harmony_get": [_P, c_int32, _P],
    "sc_harmony_end": [_P],
    "sc_hop_begin": [_P, _P, _P, c_int64],
    "sc_hop_next": [_P, POINTER(c_int64), POINTER(c_int32), POINTER(c_int64)],
    "sc_hop_get": [_P, _P, _P],
    "sc_hop_aggregate": [_P, _P, c_int, c_int32, c_int32, _P],
    "sc_hop_times": [_P, _P],
    "sc_hop_end": [_P],
    "sc_mixture_fit": [_P, _P, c_int, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_double, _P, _P, c_int32, c_double,
                       c_double, _P, _P, _P, _P, _P, _P, POINTER(c_int32), _P, _P, POINTER(c_double)],
    "sc_mixture_predict": [_P, _P, c_int, c_int64, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, POINTER(c_double)],
    "sc_mixture_slice_rows": [c_int64, c_int32, c_int32, c_int32, POINTER(c_int64)],
    "sc_louvain_begin": [_P, _P, _P, _P, c_int64, c_int32, c_int32],
    "sc_louvain_resident_weights": [_P, _P, c_int64],
    "sc_louvain_begin_resident": [_P, _P, c_int64, c_int32, c_int32],
    "sc_louvain_level": [_P, _P, _P],
    "sc_louvain_labels": [_P, _P, POINTER(c_int64)],
    "sc_louvain_end": [_P],
    "sc_comm_unique_id": [_P],
    "sc_comm_create": [_P, _P, c_int, c_int, POINTER(c_void_p)],
    "sc_comm_destroy": [_P],
    "sc_allgather": [_P, _P, c_int64, _P],
    "sc_allreduce_max": [_P, _P, c_int64],
    "sc_allreduce_sum_i64": [_P, _P, c_int64],
    "sc_comm_info": [_P, POINTER(c_int), POINTER(c_int), POINTER(c_int)],
}

_lib = None
_lock = threading.Lock()


class SpatialCoreHipError(RuntimeError):
    """HIP runtime / library-state failure reported by libspatialcore_hip.so."""


def load_library() -> ctypes.CDLL:
    """Load the shared library (no GPU needed for loading).  Raises if it has not been built."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "or `make -C spatialcore_amd/csrc`.  There is no CPU fallback.")
            lib = ctypes.CDLL(LIB_PATH)
            for name, argtypes in SYMBOLS.items():
                fn = getattr(lib, name)  # AttributeError if the header and the library diverge
                fn.argtypes = argtypes
                fn.restype = c_int
            lib.sc_last_error.argtypes = []
            lib.sc_last_error.restype = c_char_p
            _lib = lib
    return _lib


def source_hash(names=("sc_moran.hip", "sc_ctx.h")) -> str:
    """sha256 over the native sources that hold the scoring kernels: ties a measured artefact
    (profiles/*_pmc_traffic.json) to the kernel code it was measured on."""
    import hashlib

    h = hashlib.sha256()
    for name in names:
        h.update(name.encode())
        with open(os.path.join(_HERE, "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _check(rc: int) -> None:
    if rc == SC_OK:
        return
    msg = load_library().sc_last_error().decode("utf-8", "replace")
    if rc in (SC_ERR_INVALID, SC_ERR_EMPTY):
        raise ValueError(msg)
    if rc == SC_ERR_ILLDEFINED:   # sklearn's _compute_precision_cholesky message
        raise ValueError("Fitting the mixture model failed because some components have ill-defined empirical covariance "
                         "(for instance caused by singleton or collapsed samples). Try to decrease the number of components, "
                         f"increase reg_covar, or scale the input data. ({msg})")
    if rc == SC_ERR_NOMEM:
        raise MemoryError(msg)
    raise SpatialCoreHipError(msg)


def mixture_slice_rows(n: int, D: int, K: int, covariance_type: str = "full") -> int:
    """sc_mixture_slice_rows: the rows per M-step slice of sc_mixture_fit, a function of the shape alone.  The library
    states the rule once; no device is needed."""
    rows = c_int64(0)
    _check(load_library().sc_mixture_slice_rows(int(n), int(D), int(K), MIX_COVARIANCES[covariance_type], byref(rows)))
    return rows.value


def device_count() -> int:
    n = c_int(0)
    rc = load_library().sc_device_count(byref(n))
    return n.value if rc == SC_OK else 0


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _c(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype)


def rng_state_words(rng: np.random.Generator) -> np.ndarray:
    """PCG64 Generator state as the 6 uint64 words sc_perm_* take.  The seed -> state expansion
    (SeedSequence) stays in numpy; only the stream itself is re-implemented natively."""
    st = rng.bit_generator.state
    if st.get("bit_generator") != "PCG64":
        raise ValueError("only numpy PCG64 generators (np.random.default_rng) are supported")
    s, inc = st["state"]["state"], st["state"]["inc"]
    m = 0xFFFFFFFFFFFFFFFF
    return np.array([s >> 64, s & m, inc >> 64, inc & m, st["has_uint32"], st["uinteger"]], dtype=np.uint64)


def set_rng_state(rng: np.random.Generator, words: np.ndarray) -> None:
    w = [int(x) for x in words]
    rng.bit_generator.state = {"bit_generator": "PCG64",
                               "state": {"state": (w[0] << 64) | w[1], "inc": (w[2] << 64) | w[3]},
                               "has_uint32": w[4], "uinteger": w[5]}


def perm_numpy_host(words: np.ndarray, n: int, n_perm: int) -> np.ndarray:
    """Host-only numpy-exact permutation table (no GPU needed).  `words` is updated in place."""
    out = np.empty((n_perm, n), dtype=np.int32)
    _check(load_library().sc_perm_numpy_host(_ptr(words), n, n_perm, _ptr(out)))
    return out


def perm_counter_host(seed: int, n: int, n_perm: int, p_first: int = 0) -> np.ndarray:
    """Host-only counter-based permutations p_first .. p_first + n_perm - 1 (no GPU needed); see
    Context.generate_permutations_counter."""
    out = np.empty((n_perm, n), dtype=np.int32)
    _check(load_library().sc_perm_counter_host(int(seed) & 0xFFFFFFFFFFFFFFFF, n, int(p_first), n_perm, _ptr(out)))
    return out


class Context:
    """One GPU + one HIP stream + the device-resident operands of the hot path."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        h = c_void_p()
        _check(self._lib.sc_ctx_create(int(device), byref(h)))
        self._h = h
        self.device = int(device)
        self._ripley_radii = 0   # radii of the resident Ripley pair list (shape of ripley_counts / ripley_counter results)
        self._ripley_g_radii = 0   # ... and of the resident Ripley's G neighbour lists
        self._annot_shape = None   # (classes, genes) of the resident training problem (annot_train_begin .. annot_train_end)
        self._pca_shape = None     # (cells, genes) of the resident PCA matrix (pca_begin .. pca_end)
        self._harmony = None       # (n, d, K, B, blocks) of the resident Harmony problem (harmony_begin .. harmony_end)
        self._hop = None           # [n, stored entries of the resident shell, X as uploaded] (hop_begin .. hop_end)
        self._louvain_n = None     # vertices of the next Louvain level (louvain_begin .. louvain_end)
        self._diff_n = self._diff_nnz = self._lanczos_cap = 0   # cells / stored entries of the resident diffusion graph, Lanczos basis cap
        self._cross_nq = self._cross_nref = None                # rows of the last knn_cross's lists, its reference rows

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.sc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- plumbing ---------------------------------------------------------------------------
    def sync(self) -> None:
        _check(self._lib.sc_ctx_sync(self._h))

    def kernel_time(self, kernel_id: int) -> Tuple[float, int]:
        ms, cnt = c_double(0), c_int64(0)
        _check(self._lib.sc_ctx_kernel_time(self._h, kernel_id, byref(ms), byref(cnt)))
        return ms.value, cnt.value

    def reset_timers(self) -> None:
        _check(self._lib.sc_ctx_reset_timers(self._h))

    def set_timing(self, enabled: bool) -> None:
        _check(self._lib.sc_ctx_set_timing(self._h, int(enabled)))

    def set_permgen_mode(self, mode: int) -> None:
        """0 automatic, 1 sequential rejection scan only, 2 fault injection (tests). Results never differ."""
        _check(self._lib.sc_ctx_set_permgen_mode(self._h, int(mode)))

    def set_moran_source_bits(self, min_bits: int) -> None:
        """Narrowest exact source copy the permutation kernels may gather: 4 (opt-in: nibble slots for count data when they
        take fewer rows than uint8), 8 (default: uint8 when every value is an integer count < 256), 16 (uint16, counts <
        65536), 32 (float32) or 64 (the fp64 tiles)."""
        _check(self._lib.sc_ctx_set_moran_source_bits(self._h, int(min_bits)))

    def moran_source_bits(self) -> int:
        """Source width the last scoring call gathered: 4 (nibble slots) / 8 / 16 (uint8 / uint16 counts), 32 (float32 raw
        values) or 64 (fp64 kernel)."""
        v = c_int(0)
        _check(self._lib.sc_ctx_moran_source_bits(self._h, byref(v)))
        return v.value

    def moran_row_groups(self) -> int:
        """128-byte rows the last scoring call gathered per (permutation, cell)."""
        v = c_int(0)
        _check(self._lib.sc_ctx_moran_row_groups(self._h, byref(v)))
        return v.value

    def moran_lag_bits(self) -> int:
        """Element width of the lag rows the last scoring call streamed: 16 (neighbour sums of a count batch) or 64."""
        v = c_int(0)
        _check(self._lib.sc_ctx_moran_lag_bits(self._h, byref(v)))
        return v.value

    def permgen_stats(self) -> Tuple[int, int, int, int, int]:
        """(jobs by the block-parallel scan, jobs by the sequential scan, verification fallbacks,
        blocks resolved by prepared table lookup, blocks computed by the chain workgroup)."""
        v = [c_int64(0) for _ in range(5)]
        _check(self._lib.sc_ctx_permgen_stats(self._h, *[byref(x) for x in v]))
        return tuple(x.value for x in v)

    def permgen_note(self) -> str:
        """Why the permutation generator left its block-parallel form ("" while it is in use); logged once as a warning."""
        msg = c_char_p()
        _check(self._lib.sc_ctx_permgen_note(self._h, byref(msg)))
        note = (msg.value or b"").decode("utf-8", "replace")
        if note and note != getattr(self, "_note_logged", ""):
            self._note_logged = note
            from spatialcore_amd._logging import get_logger

            get_logger("device").warning(note)
        return note

    def probe_streams(self) -> Tuple[bool, int]:
        """(the generator's streams run concurrently, GPU_MAX_HW_QUEUES as this process's environment has it; 0 = unset)."""
        ok, q = c_int(0), c_int(0)
        _check(self._lib.sc_ctx_probe_streams(self._h, byref(ok), byref(q)))
        self.permgen_note()
        return bool(ok.value), q.value

    def permgen_form(self, n: int) -> str:
        """Which scan a permutation job of length n takes right now: "block-parallel", "sequential (...)" or
        "sequential: <reason>" -- recorded in the provenance entry of every drop-in call that draws permutations."""
        msg = c_char_p()
        _check(self._lib.sc_ctx_permgen_form(self._h, int(n), byref(msg)))
        return (msg.value or b"").decode("utf-8", "replace")

    def debug_copy(self, which: int, offset_bytes: int, count: int, dtype) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        _check(self._lib.sc_debug_copy(self._h, int(which), int(offset_bytes), _ptr(out), out.nbytes))
        return out

    def device_mem(self) -> int:
        v = c_int64(0)
        _check(self._lib.sc_ctx_device_mem(self._h, byref(v)))
        return v.value

    def device_mem_free(self) -> int:
        """Free memory of the device right now, in bytes."""
        v = c_int64(0)
        _check(self._lib.sc_ctx_device_free(self._h, byref(v)))
        return v.value

    # ---- A1 / A2 ----------------------------------------------------------------------------
    def knn(self, coords, k: int, include_self: bool = False, return_distance: bool = False,
            fetch: bool = True):
        xy = _c(coords, np.float64)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError(f"coordinates must have shape (n, 2), got {xy.shape}")
        n = xy.shape[0]
        idx = np.empty((n, k), dtype=np.int32) if fetch else None
        rd = np.empty((n, k), dtype=np.float64) if (return_distance and fetch) else None
        self._xy_in_flight = xy      # fetch=False returns without waiting: the upload may still be reading this array
        _check(self._lib.sc_knn_2d(self._h, _ptr(xy), n, int(k), int(include_self), _ptr(idx), _ptr(rd)))
        self._knn_shape = (n, int(k))
        return (idx, rd) if return_distance else idx

    def knn_fetch(self, return_distance: bool = True):
        """Neighbour lists of the last knn(..., fetch=False), copied out on the library's copy stream (callable from a
        second thread while the context's stream works on something else)."""
        n, k = self._knn_shape
        idx = np.empty((n, k), dtype=np.int32)
        rd = np.empty((n, k), dtype=np.float64) if return_distance else None
        _check(self._lib.sc_knn_fetch(self._h, _ptr(idx), _ptr(rd)))
        return (idx, rd) if return_distance else idx

    def radius_graph(self, coords, radius: float):
        xy = _c(coords, np.float64)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError(f"coordinates must have shape (n, 2), got {xy.shape}")
        n = xy.shape[0]
        indptr = np.empty(n + 1, dtype=np.int64)
        _check(self._lib.sc_radius_count_2d(self._h, _ptr(xy), n, float(radius), _ptr(indptr)))
        nnz = int(indptr[-1])
        indices = np.empty(nnz, dtype=np.int32)
        _check(self._lib.sc_radius_fill_2d(self._h, nnz, _ptr(indices)))
        return indptr, indices

    # ---- A3 ---------------------------------------------------------------------------------
    def set_graph_csr(self, indptr, indices, data, n: int) -> None:
        indptr = _c(indptr, np.int64)
        indices = _c(indices, np.int32)
        data = _c(data, np.float64)
        _check(self._lib.sc_graph_set_csr(self._h, _ptr(indptr), _ptr(indices), _ptr(data), int(n), int(indices.size)))

    def graph_from_knn(self, weight: float) -> None:
        _check(self._lib.sc_graph_from_knn(self._h, float(weight)))

    def graph_shape(self) -> Tuple[int, int]:
        n, nnz = c_int64(0), c_int64(0)
        _check(self._lib.sc_graph_shape(self._h, byref(n), byref(nnz)))
        return n.value, nnz.value

    def get_graph(self):
        n, nnz = self.graph_shape()
        indptr = np.empty(n + 1, dtype=np.int64)
        indices = np.empty(nnz, dtype=np.int32)
        data = np.empty(nnz, dtype=np.float64)
        _check(self._lib.sc_graph_get(self._h, _ptr(indptr), _ptr(indices), _ptr(data)))
        return indptr, indices, data

    def graph_moments(self) -> Tuple[float, float, float]:
        a, b, d = c_double(0), c_double(0), c_double(0)
        _check(self._lib.sc_graph_moments(self._h, byref(a), byref(b), byref(d)))
        return a.value, b.value, d.value

    # ---- expression -------------------------------------------------------------------------
    def set_expression(self, X, gene_cols) -> None:
        """X: scipy sparse (any format) or dense (cells x n_vars); gene_cols: distinct column ids."""
        from scipy import sparse

        cols = _c(gene_cols, np.int32)
        if sparse.issparse(X):
            Xc = X.tocsr()
            if not Xc.has_canonical_format:
                Xc = Xc.copy()
                Xc.sum_duplicates()
            dt = SC_F32 if Xc.dtype == np.float32 else SC_F64
            data = _c(Xc.data, np.float32 if dt == SC_F32 else np.float64)
            indptr = _c(Xc.indptr, np.int64)
            indices = _c(Xc.indices, np.int32)
            _check(self._lib.sc_expr_set_csr(self._h, _ptr(indptr), _ptr(indices), _ptr(data), dt, Xc.shape[0],
                                             Xc.shape[1], _ptr(cols), cols.size))
        else:
            A = np.asarray(X)
            if A.ndim != 2:
                raise ValueError("expression matrix must be 2-D")
            # ship only the requested columns when they are a small part of a wide matrix
            if A.shape[1] > 2 * cols.size:
                A = A[:, cols]
                cols = np.arange(cols.size, dtype=np.int32)
            dt = SC_F32 if A.dtype == np.float32 else SC_F64
            A = _c(A, np.float32 if dt == SC_F32 else np.float64)
            _check(self._lib.sc_expr_set_dense(self._h, _ptr(A), dt, A.shape[0], A.shape[1], _ptr(cols), cols.size))
        self._n_genes = int(cols.size)

    def expr_stats(self):
        mean = np.empty(self._n_genes, dtype=np.float64)
        var = np.empty(self._n_genes, dtype=np.float64)
        _check(self._lib.sc_expr_stats(self._h, _ptr(mean), _ptr(var)))
        return mean, var

    # ---- A4 ---------------------------------------------------------------------------------
    def generate_permutations(self, words: np.ndarray, n: int, n_perm: int, fetch: bool = False):
        out = np.empty((n_perm, n), dtype=np.int32) if fetch else None
        _check(self._lib.sc_perm_generate(self._h, _ptr(words), int(n), int(n_perm), _ptr(out)))
        self.permgen_note()
        return out

    def generate_permutations_counter(self, seed: int, n: int, n_perm: int, p_first: int = 0, fetch: bool = False):
        """EXTENSION: counter-based permutations p_first .. p_first + n_perm - 1 as the resident table (rows 0 ..):
        permutation p is a pure function of (seed, p) -- Fisher-Yates with Philox4x32-10 + Lemire draws -- so ranks and
        batches can take disjoint ranges.  For the paths that have no reference seed semantics only."""
        out = np.empty((n_perm, n), dtype=np.int32) if fetch else None
        _check(self._lib.sc_perm_generate_counter(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(n), int(p_first), int(n_perm),
                                                  _ptr(out)))
        return out

    def set_permutations(self, perm) -> None:
        perm = _c(perm, np.int32)
        if perm.ndim != 2:
            raise ValueError("permutation table must have shape (n_perm, n)")
        _check(self._lib.sc_perm_set(self._h, _ptr(perm), perm.shape[1], perm.shape[0]))

    # ---- A5-A8 ------------------------------------------------------------------------------
    def moran(self, n_perm: int, return_sims: bool = True):
        G = self._n_genes
        I = np.empty(G, dtype=np.float64)
        sims = np.empty((n_perm, G), dtype=np.float64) if (n_perm > 0 and return_sims) else None
        cnt = np.zeros(G, dtype=np.int64) if n_perm > 0 else None
        ssum = np.zeros(G, dtype=np.float64) if n_perm > 0 else None
        ssq = np.zeros(G, dtype=np.float64) if n_perm > 0 else None
        _check(self._lib.sc_moran(self._h, int(n_perm), _ptr(I), _ptr(sims), _ptr(cnt), _ptr(ssum), _ptr(ssq)))
        return {"I": I, "sims": sims, "count_ge": cnt, "sim_sum": ssum, "sim_sumsq": ssq}

    def moran_seeded(self, words: np.ndarray, n_perm: int, return_sims: bool = True):
        """sc_perm_generate + sc_moran, pipelined on the device; `words` is advanced in place."""
        G = self._n_genes
        I = np.empty(G, dtype=np.float64)
        sims = np.empty((n_perm, G), dtype=np.float64) if return_sims else None
        cnt = np.zeros(G, dtype=np.int64)
        ssum = np.zeros(G, dtype=np.float64)
        ssq = np.zeros(G, dtype=np.float64)
        _check(self._lib.sc_moran_seeded(self._h, _ptr(words), int(n_perm), _ptr(I), _ptr(sims), _ptr(cnt),
                                         _ptr(ssum), _ptr(ssq)))
        self.permgen_note()
        return {"I": I, "sims": sims, "count_ge": cnt, "sim_sum": ssum, "sim_sumsq": ssq}

    def moran_seeded_begin(self, words: np.ndarray, n_cells: int, n_perm: int, ahead_chunks: int = 0) -> None:
        """First half of moran_seeded: the generator job (it needs only n_cells and the state) starts and runs while the
        caller builds the graph and uploads the expression; moran_seeded_finish scores.  ahead_chunks: generator chunks
        enqueued before this returns (0 = all: for callers with an upload in front of the finish; else >= 2)."""
        _check(self._lib.sc_moran_seeded_begin(self._h, _ptr(words), int(n_cells), int(n_perm), int(ahead_chunks)))
        self._begun_perms = int(n_perm)

    def moran_seeded_abort(self) -> None:
        _check(self._lib.sc_moran_seeded_abort(self._h))
        self._begun_perms = 0

    def moran_seeded_finish(self, words: np.ndarray, return_sims: bool = True):
        n_perm, G = self._begun_perms, self._n_genes
        I = np.empty(G, dtype=np.float64)
        sims = np.empty((n_perm, G), dtype=np.float64) if return_sims else None
        cnt = np.zeros(G, dtype=np.int64)
        ssum = np.zeros(G, dtype=np.float64)
        ssq = np.zeros(G, dtype=np.float64)
        self._begun_perms = 0
        _check(self._lib.sc_moran_seeded_finish(self._h, _ptr(words), _ptr(I), _ptr(sims), _ptr(cnt), _ptr(ssum), _ptr(ssq)))
        self.permgen_note()
        return {"I": I, "sims": sims, "count_ge": cnt, "sim_sum": ssum, "sim_sumsq": ssq}

    def lee(self, pair_x, pair_y, perm_offset, n_perm: int, return_perms: bool = False):
        px, py = _c(pair_x, np.int32), _c(pair_y, np.int32)
        off = _c(perm_offset, np.int64) if perm_offset is not None else None
        q = px.size
        L = np.empty(q, dtype=np.float64)
        cnt = np.zeros(q, dtype=np.int64)
        Lp = np.empty((q, n_perm), dtype=np.float64) if return_perms else None
        _check(self._lib.sc_lee(self._h, _ptr(px), _ptr(py), _ptr(off), q, int(n_perm), _ptr(L), _ptr(cnt), _ptr(Lp)))
        return {"L": L, "count_abs_ge": cnt, "L_perm": Lp}

    def lee_seeded(self, words: np.ndarray, pair_x, pair_y, n_perm: int, return_perms: bool = False):
        """All pairs of a lees_l call: observed L (fp64 matrix cores) + per-pair permutation counts from the one
        numpy-exact stream `words` (advanced in place), generator and scoring pipelined on the device."""
        px, py = _c(pair_x, np.int32), _c(pair_y, np.int32)
        q = px.size
        L = np.empty(q, dtype=np.float64)
        cnt = np.zeros(q, dtype=np.int64)
        Lp = np.empty((q, n_perm), dtype=np.float64) if return_perms else None
        _check(self._lib.sc_lee_seeded(self._h, _ptr(words), _ptr(px), _ptr(py), q, int(n_perm), _ptr(L), _ptr(cnt), _ptr(Lp)))
        return {"L": L, "count_abs_ge": cnt, "L_perm": Lp}

    def lee_shared(self, words, genes_x, genes_y, n_perm: int, return_perms: bool = False):
        """EXTENSION: the full grid genes_x x genes_y under one shared block of permutations (fp64 MFMA contractions)."""
        gx, gy = _c(genes_x, np.int32), _c(genes_y, np.int32)
        L = np.empty((gx.size, gy.size), dtype=np.float64)
        cnt = np.zeros((gx.size, gy.size), dtype=np.int64)
        Lp = np.empty((n_perm, gx.size, gy.size), dtype=np.float64) if return_perms else None
        # words = None: rows [0, n_perm) of the resident table (e.g. generate_permutations_counter's)
        _check(self._lib.sc_lee_shared(self._h, _ptr(words), _ptr(gx), gx.size, _ptr(gy), gy.size, int(n_perm), _ptr(L), _ptr(cnt), _ptr(Lp)))
        return {"L": L, "count_abs_ge": cnt, "L_perm": Lp}

    def lee_observed_f32(self, pair_x, pair_y) -> np.ndarray:
        """Observed L of each pair exactly as the reference's float32 arithmetic yields it (float32 matrices only)."""
        px, py = _c(pair_x, np.int32), _c(pair_y, np.int32)
        out = np.empty(px.size, dtype=np.float32)
        _check(self._lib.sc_lee_observed_f32(self._h, _ptr(px), _ptr(py), px.size, _ptr(out), None, None))
        return out

    # ---- N1 / N2, and Getis-Ord Gi / Gi* and local Geary's C (extension) ------
    def _local_call(self, n_cells: int, value: str, counts, fetch: bool, call):
        """One sc_local_* call: z, lag and the statistic (key ``value``), the int32 count arrays named in ``counts`` (null
        pointers unless ``fetch``) and the zero-variance flags, in the order of the symbol's output arguments."""
        G = self._n_genes
        r = {name: np.empty((n_cells, G), dtype=np.float32) for name in ("z", "lag", value)}
        r.update({name: np.zeros((n_cells, G), dtype=np.int32) if fetch else None for name in counts})
        zero = np.zeros(G, dtype=np.uint8)
        _check(call(*(_ptr(a) for a in r.values()), _ptr(zero)))
        r["zero_var"] = zero.astype(bool)
        return r

    def _local_hist(self, symbol, n_perm: int) -> np.ndarray:
        hist = np.zeros((self._n_genes, n_perm + 1), dtype=np.int64)
        _check(symbol(self._h, _ptr(hist)))
        return hist

    def _local_classify(self, symbol, n_cells: int, p_tab, padj_tab, force_ns, alpha):
        G = self._n_genes
        with_p = p_tab is not None
        p = np.empty((n_cells, G), dtype=np.float32) if with_p else None
        padj = np.empty((n_cells, G), dtype=np.float32) if with_p else None
        q = np.empty((n_cells, G), dtype=np.int8)
        pt = _c(p_tab, np.float32) if with_p else None
        at = _c(padj_tab, np.float32) if with_p else None
        f = _c(np.asarray(force_ns).astype(np.uint8), np.uint8)
        _check(symbol(self._h, _ptr(pt), _ptr(at), _ptr(f), c_float(float(np.float32(alpha))), _ptr(p), _ptr(padj), _ptr(q)))
        return p, padj, q

    def local_moran(self, n_cells: int, n_perm: int, perm_row0: int = 0, fetch_counts: bool = True):
        return self._local_call(n_cells, "I", ("count",), n_perm > 0 and fetch_counts, lambda *out: self._lib.sc_local_moran(
            self._h, int(n_perm), int(perm_row0), *out))

    def local_moran_seeded(self, words: np.ndarray, n_cells: int, n_perm: int, fetch_counts: bool = True):
        """local_moran with its n_perm permutations drawn from `words` (advanced in place) inside the call: generator and
        per-cell counts run as one pipeline."""
        r = self._local_call(n_cells, "I", ("count",), fetch_counts, lambda *out: self._lib.sc_local_moran_seeded(
            self._h, _ptr(words), int(n_perm), *out))
        self.permgen_note()
        return r

    def local_moran_hist(self, n_perm: int) -> np.ndarray:
        """hist[g][c] = cells of gene g whose permutation count is c (of the last local_moran call)."""
        return self._local_hist(self._lib.sc_local_moran_hist, n_perm)

    def local_moran_classify(self, n_cells: int, p_tab, padj_tab, force_ns, alpha):
        """Per-cell p, adjusted p (table lookups by permutation count) and LISA quadrants of the last local_moran."""
        return self._local_classify(self._lib.sc_local_moran_classify, n_cells, p_tab, padj_tab, force_ns, alpha)

    def local_stat(self, stat: str, n_cells: int, n_perm: int, perm_row0: int = 0, star: bool = False,
                   fetch_counts: bool = True):
        """z, lag, the statistic ("getis": G, Gi* with ``star`` on a graph with self edges; "geary": C) and the two-tail
        counts ge / le of rows [perm_row0, perm_row0 + n_perm) of the active permutation table."""
        return self._local_call(n_cells, "stat", ("ge", "le"), n_perm > 0 and fetch_counts, lambda *out: self._lib.sc_local_stat(
            self._h, LOCAL_STATS[stat], int(bool(star)), int(n_perm), int(perm_row0), *out))

    def local_stat_seeded(self, stat: str, words: np.ndarray, n_cells: int, n_perm: int, star: bool = False,
                          fetch_counts: bool = True):
        """local_stat with its n_perm permutations drawn from `words` (advanced in place) inside the call."""
        r = self._local_call(n_cells, "stat", ("ge", "le"), n_perm > 0 and fetch_counts, lambda *out: self._lib.sc_local_stat_seeded(
            self._h, LOCAL_STATS[stat], int(bool(star)), _ptr(words), int(n_perm), *out))
        self.permgen_note()
        return r

    def local_stat_hist(self, n_perm: int) -> np.ndarray:
        """hist[g][m] = cells of gene g whose permutation level min(ge, le) is m (of the last local_stat call)."""
        return self._local_hist(self._lib.sc_local_stat_hist, n_perm)

    def local_stat_classify(self, n_cells: int, p_tab, padj_tab, force_ns, alpha):
        """Per-cell p, adjusted p (table lookups by min(ge, le)) and the classes of the last local_stat."""
        return self._local_classify(self._lib.sc_local_stat_classify, n_cells, p_tab, padj_tab, force_ns, alpha)

    def lee_local(self, n_cells: int, gene_x: int, gene_y: int, n_perm: int = 0, perm_row0: int = 0):
        zx = np.empty(n_cells, dtype=np.float64)
        lag = np.empty(n_cells, dtype=np.float64)
        L = np.empty(n_cells, dtype=np.float64)
        cnt = np.zeros(n_cells, dtype=np.int32) if n_perm > 0 else None
        _check(self._lib.sc_lee_local(self._h, int(gene_x), int(gene_y), int(n_perm), int(perm_row0), _ptr(zx),
                                      _ptr(lag), _ptr(L), _ptr(cnt)))
        return {"zx": zx, "lag": lag, "L_local": L, "count": cnt}

    def lee_local_seeded(self, words: np.ndarray, n_cells: int, gene_x: int, gene_y: int, n_perm_global: int, n_perm_local: int):
        """generate_permutations + lee (rows [0, n_perm_global)) + lee_local (the rows behind) for one pair, as one
        pipeline behind the generator; `words` (numpy generator state) is advanced in place."""
        zx = np.empty(n_cells, dtype=np.float64)
        lag = np.empty(n_cells, dtype=np.float64)
        L_local = np.empty(n_cells, dtype=np.float64)
        cnt = np.zeros(n_cells, dtype=np.int32) if n_perm_local > 0 else None
        L = np.zeros(1, dtype=np.float64)
        ge = np.zeros(1, dtype=np.int64)
        w = _c(words, np.uint64)
        _check(self._lib.sc_lee_local_seeded(self._h, _ptr(w), int(gene_x), int(gene_y), int(n_perm_global), int(n_perm_local),
                                             _ptr(L), _ptr(ge), _ptr(zx), _ptr(lag), _ptr(L_local), _ptr(cnt)))
        if w is not words:
            words[...] = w
        return {"L": float(L[0]), "count_abs_ge": int(ge[0]), "zx": zx, "lag": lag, "L_local": L_local, "count": cnt}

    # ---- N3 ---------------------------------------------------------------------------------
    def nearest(self, targets, queries):
        t, q = _c(targets, np.float64), _c(queries, np.float64)
        idx = np.empty(q.shape[0], dtype=np.int32)
        dist = np.empty(q.shape[0], dtype=np.float64)
        _check(self._lib.sc_nearest_2d(self._h, _ptr(t), t.shape[0], _ptr(q), q.shape[0], _ptr(idx), _ptr(dist)))
        return dist, idx

    def nearest_excluding(self, targets, target_code, queries, query_excluded_code):
        """Nearest target whose group code differs from the query's excluded code; (inf, -1) when none is left."""
        t, q = _c(targets, np.float64), _c(queries, np.float64)
        tc, qc = _c(target_code, np.int32), _c(query_excluded_code, np.int32)
        if tc.size != t.shape[0] or qc.size != q.shape[0]:
            raise ValueError("one group code per target and per query is required")
        idx = np.empty(q.shape[0], dtype=np.int32)
        dist = np.empty(q.shape[0], dtype=np.float64)
        _check(self._lib.sc_nearest_excluding_2d(self._h, _ptr(t), _ptr(tc), t.shape[0], _ptr(q), _ptr(qc), q.shape[0],
                                                 _ptr(idx), _ptr(dist)))
        return dist, idx

    def pair_table(self, a_sorted, a_off, b_sorted, b_off):
        """(sum, min) of the pairwise distances of every (group of a, group of b) block; points sorted by group."""
        a, b = _c(a_sorted, np.float64), _c(b_sorted, np.float64)
        ao, bo = _c(a_off, np.int64), _c(b_off, np.int64)
        ga, gb = ao.size - 1, bo.size - 1
        if ao[-1] != a.shape[0] or bo[-1] != b.shape[0]:
            raise ValueError("group offsets do not cover the point arrays")
        tot = np.empty((ga, gb), dtype=np.float64)
        mn = np.empty((ga, gb), dtype=np.float64)
        _check(self._lib.sc_pair_table_2d(self._h, _ptr(a), _ptr(ao), ga, _ptr(b), _ptr(bo), gb, _ptr(tot), _ptr(mn)))
        return tot, mn

    def pairwise(self, a, b):
        a, b = _c(a, np.float64), _c(b, np.float64)
        mean, mn = c_double(0), c_double(0)
        _check(self._lib.sc_pairwise_2d(self._h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], byref(mean), byref(mn)))
        return mean.value, mn.value

    # ---- N7: spatial domains -----------------------------------------------------------------
    def domains(self, targets, queries, cell_dist: float, shrink: float, return_clearance: bool = True):
        """Buffer - union - shrink over discs (sc_domains_2d): (component id per target = smallest target index of its
        component, component id per query or -1, clearance per query or None).  ``queries`` may be None or empty."""
        t = _c(targets, np.float64)
        if t.ndim != 2 or t.shape[1] != 2:
            raise ValueError(f"targets must have shape (n, 2), got {t.shape}")
        q = _c(queries if queries is not None else np.zeros((0, 2)), np.float64).reshape(-1, 2)
        n_q = q.shape[0]
        comp_t = np.empty(t.shape[0], dtype=np.int32)
        comp_q = np.empty(n_q, dtype=np.int32)
        clear = np.empty(n_q, dtype=np.float64) if return_clearance else None
        _check(self._lib.sc_domains_2d(self._h, _ptr(t), t.shape[0], _ptr(q) if n_q else None, n_q, float(cell_dist),
                                       float(shrink), _ptr(comp_t), _ptr(comp_q) if n_q else None,
                                       _ptr(clear) if (n_q and return_clearance) else None))
        return comp_t, comp_q, clear

    # ---- N8 (extension): rank sums ----------------------------------------------------------
    def ranksum(self, group_code, n_groups: int) -> dict:
        """Wilcoxon rank sums of the loaded genes per group (sc_ranksum): ``rank2`` (G, K) int64 = 2 * sum of the average
        ranks of the group's cells among the cells with a code >= 0 (-1 excludes a cell), ``tie_nonzero`` (G,) Python ints
        = sum of t^3 - t over the tie runs of non-zero values, ``nnz`` (G, K) int64, ``sums`` (G, K) float64, ``n_neg``
        (G,) int64 and ``group_n`` (K,) int64.  Exact integers, identical from run to run."""
        code = _c(group_code, np.int32)
        if code.ndim != 1:
            raise ValueError(f"group codes must be 1-D, got shape {code.shape}")
        # (without a loaded expression the library refuses the call: the arrays only have to exist)
        G, K = max(int(getattr(self, "_n_genes", 0)), 1), int(n_groups)
        shape = (G, max(K, 1))
        rank2 = np.zeros(shape, dtype=np.int64)
        tie = np.zeros((G, 2), dtype=np.uint64)
        nnz = np.zeros(shape, dtype=np.int64)
        sums = np.zeros(shape, dtype=np.float64)
        n_neg = np.zeros(G, dtype=np.int64)
        group_n = np.zeros(max(K, 1), dtype=np.int64)
        _check(self._lib.sc_ranksum(self._h, _ptr(code), code.size, K, _ptr(rank2), _ptr(tie), _ptr(nnz), _ptr(sums),
                                    _ptr(n_neg), _ptr(group_n)))
        tie_nonzero = np.array([(int(hi) << 64) | int(lo) for hi, lo in tie], dtype=object)
        return {"rank2": rank2, "tie_nonzero": tie_nonzero, "nnz": nnz, "sums": sums, "n_neg": n_neg, "group_n": group_n}

    # ---- A9 ---------------------------------------------------------------------------------
    def profile_counts(self, labels, n_types: int) -> np.ndarray:
        lab = _c(labels, np.int32)
        out = np.empty((lab.size, n_types), dtype=np.float32)
        empty = c_int64(0)
        _check(self._lib.sc_profile_counts(self._h, _ptr(lab), lab.size, int(n_types), _ptr(out), byref(empty)))
        return out


    # ---- N5: niches (k-means) ----------------------------------------------------------------
    def kmeans(self, X, n_clusters: int, n_init: int, max_iter: int, tol: float, x_mean, uniforms) -> dict:
        """sc_kmeans_fit on a float32 or float64 (n, C) matrix (see the header for the draws' layout)."""
        X = np.ascontiguousarray(X)
        if X.dtype not in (np.float32, np.float64) or X.ndim != 2:
            raise ValueError(f"kmeans: X must be a 2-D float32 or float64 array, got {X.dtype} {X.shape}")
        n, C = X.shape
        K = int(n_clusters)
        xm = np.ascontiguousarray(x_mean, dtype=X.dtype)
        u = _c(uniforms, np.float64)
        L = 2 + int(np.log(K)) if K >= 1 else 0
        if xm.shape != (C,) or u.size != int(n_init) * (1 + (K - 1) * L):
            raise ValueError("kmeans: x_mean must have C entries and uniforms n_init * (1 + (K - 1) * L)")
        labels = np.empty(n, dtype=np.int32)
        centers = np.empty((K, C), dtype=X.dtype)
        seeds = np.empty((int(n_init), K), dtype=np.int64)
        inertia, n_iter, strict, distinct = c_double(0.0), c_int32(0), c_int32(0), c_int32(0)
        _check(self._lib.sc_kmeans_fit(self._h, _ptr(X), SC_F32 if X.dtype == np.float32 else SC_F64, n, C, K,
                                       int(n_init), int(max_iter), float(tol), _ptr(xm), _ptr(u), _ptr(labels),
                                       _ptr(centers), byref(inertia), _ptr(seeds), byref(n_iter), byref(strict),
                                       byref(distinct)))
        return {"labels": labels, "centers": centers, "inertia": inertia.value, "seeds": seeds,
                "n_iter": n_iter.value, "strict": bool(strict.value), "distinct": distinct.value}

    # ---- T1-T4: classify_by_threshold --------------------------------------------------------
    @staticmethod
    def _scores(a, what: str) -> np.ndarray:
        a = np.ascontiguousarray(a)
        if a.dtype not in (np.float32, np.float64) or a.ndim != 1:
            raise ValueError(f"{what}: scores must be a 1-D float32 or float64 array, got {a.dtype} {a.shape}")
        return a

    def metagene_score(self, features, method: str, pseudocount: float = 0.1) -> dict:
        """sc_metagene_score on a float32 or float64 (n, F) matrix: ``valid`` (n,) bool, ``score`` (n,) in the input type
        (NaN where not valid), ``min`` / ``max`` / ``mean`` of the valid scores, ``n_valid``, ``n_below`` (valid scores
        < 1e-6) and ``n_negative`` (valid rows with a negative feature)."""
        F = np.ascontiguousarray(features)
        if F.dtype not in (np.float32, np.float64) or F.ndim != 2:
            raise ValueError(f"metagene_score: features must be a 2-D float32 or float64 array, got {F.dtype} {F.shape}")
        n, nf = F.shape
        valid = np.empty(n, dtype=np.uint8)
        score = np.empty(n, dtype=F.dtype)
        stats = np.empty(3, dtype=np.float64)
        counts = np.empty(3, dtype=np.int64)
        _check(self._lib.sc_metagene_score(self._h, _ptr(F), SC_F32 if F.dtype == np.float32 else SC_F64, n, nf,
                                           METAGENE_METHODS.index(method), float(pseudocount), _ptr(valid), _ptr(score),
                                           _ptr(stats), _ptr(counts)))
        return {"valid": valid.astype(bool), "score": score, "min": float(stats[0]), "max": float(stats[1]),
                "mean": float(stats[2]), "n_valid": int(counts[0]), "n_below": int(counts[1]),
                "n_negative": int(counts[2])}

    def ks_prepare(self, scores, background_quantile: float, ranks=(), return_sorted: bool = False) -> dict:
        """sc_ks_prepare: sorts the scores on the device (they stay there for ks_argmax); ``bg_mean`` / ``bg_std`` of the
        lowest max(int(n q), 10) of them, ``order`` = the order statistics at ``ranks``, ``sorted`` on request."""
        x = self._scores(scores, "ks_prepare")
        rk = _c(ranks, np.int64)
        vals = np.empty(rk.size, dtype=np.float64)
        bg = np.empty(2, dtype=np.float64)
        srt = np.empty(x.size, dtype=np.float64) if return_sorted else None
        _check(self._lib.sc_ks_prepare(self._h, _ptr(x), SC_F32 if x.dtype == np.float32 else SC_F64, x.size,
                                       float(background_quantile), _ptr(rk) if rk.size else None, rk.size,
                                       _ptr(vals) if rk.size else None, _ptr(bg), _ptr(srt)))
        return {"bg_mean": float(bg[0]), "bg_std": float(bg[1]), "order": vals, "sorted": srt}

    def ks_argmax(self, bg_mean: float, bg_std: float) -> Tuple[int, float, float]:
        """(first index of the largest D, the sorted score there, D) over the scores of the last ks_prepare."""
        i, sc, d = c_int64(0), c_double(0.0), c_double(0.0)
        _check(self._lib.sc_ks_argmax(self._h, float(bg_mean), float(bg_std), byref(i), byref(sc), byref(d)))
        return i.value, sc.value, d.value

    def ks_classify(self, scores, threshold: float, max_score: float):
        """(deviation scores float64, labels int32 = score >= threshold, their number)."""
        x = self._scores(scores, "ks_classify")
        dev = np.empty(x.size, dtype=np.float64)
        lab = np.empty(x.size, dtype=np.int32)
        nh = c_int64(0)
        _check(self._lib.sc_ks_classify(self._h, _ptr(x), SC_F32 if x.dtype == np.float32 else SC_F64, x.size,
                                        float(threshold), float(max_score), _ptr(dev), _ptr(lab), byref(nh)))
        return dev, lab, nh.value

    def gmm_fit(self, scores, n_components: int, n_init: int, km_max_iter: int, km_tol: float, x_mean, uniforms,
                max_iter: int = 100, tol: float = 1e-3, reg_covar: float = 1e-6, return_km_labels: bool = False) -> dict:
        """sc_gmm_fit: every run's ``weights`` / ``means`` / ``variances`` (n_init, K), ``lower_bound``, ``n_iter`` and
        ``converged`` (n_init,), the index ``best``, and on request every run's k-means labels (n_init, n)."""
        x = self._scores(scores, "gmm_fit")
        K, R = int(n_components), int(n_init)
        xm = np.ascontiguousarray(np.asarray(x_mean).reshape(-1), dtype=x.dtype)
        u = _c(uniforms, np.float64)
        L = 2 + int(np.log(K)) if K >= 1 else 0
        if xm.size != 1 or u.size != R * (1 + (K - 1) * L):
            raise ValueError("gmm_fit: x_mean must have one entry and uniforms n_init * (1 + (K - 1) * L)")
        w, mu, var = (np.empty((R, K), dtype=np.float64) for _ in range(3))
        lb = np.empty(R, dtype=np.float64)
        n_iter = np.empty(R, dtype=np.int32)
        conv = np.empty(R, dtype=np.int32)
        km = np.empty((R, x.size), dtype=np.int32) if return_km_labels else None
        best = c_int32(0)
        _check(self._lib.sc_gmm_fit(self._h, _ptr(x), SC_F32 if x.dtype == np.float32 else SC_F64, x.size, K, R,
                                    int(km_max_iter), float(km_tol), _ptr(xm), _ptr(u), int(max_iter), float(tol),
                                    float(reg_covar), _ptr(km), _ptr(w), _ptr(mu), _ptr(var), _ptr(lb), _ptr(n_iter),
                                    _ptr(conv), byref(best)))
        return {"weights": w, "means": mu, "variances": var, "lower_bound": lb, "n_iter": n_iter,
                "converged": conv.astype(bool), "best": best.value, "km_labels": km}

    def gmm_posterior(self, scores, weights, means, variances, high, cutoff: float):
        """(P(high) float64 = the responsibilities of the components ``high`` added in that order, labels int32 = P >
        cutoff, their number) of every score under the given mixture."""
        x = self._scores(scores, "gmm_posterior")
        w, mu, var = _c(weights, np.float64), _c(means, np.float64), _c(variances, np.float64)
        hi = _c(high, np.int32)
        if not (w.size == mu.size == var.size):
            raise ValueError("gmm_posterior: weights, means and variances must have one entry per component")
        prob = np.empty(x.size, dtype=np.float64)
        lab = np.empty(x.size, dtype=np.int32)
        nh = c_int64(0)
        _check(self._lib.sc_gmm_posterior(self._h, _ptr(x), SC_F32 if x.dtype == np.float32 else SC_F64, x.size, w.size,
                                          _ptr(w), _ptr(mu), _ptr(var), _ptr(hi), hi.size, float(cutoff), _ptr(prob),
                                          _ptr(lab), byref(nh)))
        return prob, lab, nh.value

    # ---- Gaussian mixtures (extension) --------------------------------------------------------
    @staticmethod
    def _mixture_input(X, who: str) -> np.ndarray:
        X = np.ascontiguousarray(X)
        if X.dtype not in (np.float32, np.float64) or X.ndim != 2:
            raise ValueError(f"{who}: X must be a 2-D float32 or float64 array, got {X.dtype} {X.shape}")
        return X

    def mixture_fit(self, X, n_components: int, covariance_type: str, n_init: int, km_max_iter: int, km_tol: float, x_mean,
                    uniforms, max_iter: int = 100, tol: float = 1e-3, reg_covar: float = 1e-6, return_proba: bool = False) -> dict:
        """sc_mixture_fit: every run's ``weights`` (n_init, K), ``means`` (n_init, K, D), ``covariances`` (n_init, K, D, D) or
        (n_init, K, D), ``lower_bound``, ``n_iter``, ``converged``; ``best``; the best run's ``labels``, ``loglik`` (the mean log-likelihood
        under its final parameters) and, on request, ``proba`` (n, K)."""
        X = self._mixture_input(X, "mixture_fit")
        n, D = X.shape
        K, R = int(n_components), int(n_init)
        full = MIX_COVARIANCES[covariance_type] == 0
        xm = u = None
        if K > 1:
            xm = _c(np.asarray(x_mean).reshape(-1), np.float64)
            u = _c(uniforms, np.float64)
            L = 2 + int(np.log(K))
            if xm.size != D or u.size != R * (1 + (K - 1) * L):
                raise ValueError("mixture_fit: x_mean must have D entries and uniforms n_init * (1 + (K - 1) * L)")
        R1, K1 = max(R, 1), max(K, 1)
        w = np.empty((R1, K1), dtype=np.float64)
        mu = np.empty((R1, K1, D), dtype=np.float64)
        cov = np.empty((R1, K1, D, D) if full else (R1, K1, D), dtype=np.float64)
        lb = np.empty(R1, dtype=np.float64)
        n_iter = np.empty(R1, dtype=np.int32)
        conv = np.empty(R1, dtype=np.int32)
        labels = np.empty(n, dtype=np.int32)
        proba = np.empty((n, K1), dtype=np.float64) if return_proba else None
        best, ll = c_int32(0), c_double(0.0)
        _check(self._lib.sc_mixture_fit(self._h, _ptr(X), SC_F32 if X.dtype == np.float32 else SC_F64, n, D, K,
                                        MIX_COVARIANCES[covariance_type], R, int(km_max_iter), float(km_tol), _ptr(xm), _ptr(u),
                                        int(max_iter), float(tol), float(reg_covar), _ptr(w), _ptr(mu), _ptr(cov), _ptr(lb),
                                        _ptr(n_iter), _ptr(conv), byref(best), _ptr(labels), _ptr(proba), byref(ll)))
        return {"weights": w, "means": mu, "covariances": cov, "lower_bound": lb, "n_iter": n_iter,
                "converged": conv.astype(bool), "best": best.value, "labels": labels, "proba": proba, "loglik": ll.value}

    def mixture_predict(self, X, covariance_type: str, weights, means, covariances, return_proba: bool = False):
        """sc_mixture_predict: (labels int32, responsibilities (n, K) float64 or None, mean log-likelihood)."""
        X = self._mixture_input(X, "mixture_predict")
        n, D = X.shape
        w, mu, cov = _c(weights, np.float64), _c(means, np.float64), _c(covariances, np.float64)
        K = w.size
        want = (K, D, D) if MIX_COVARIANCES[covariance_type] == 0 else (K, D)
        if w.ndim != 1 or mu.shape != (K, D) or cov.shape != want:
            raise ValueError(f"mixture_predict: need weights (K,), means (K, {D}) and covariances {want}, got {w.shape}, "
                             f"{mu.shape} and {cov.shape}")
        labels = np.empty(n, dtype=np.int32)
        proba = np.empty((n, K), dtype=np.float64) if return_proba else None
        ll = c_double(0.0)
        _check(self._lib.sc_mixture_predict(self._h, _ptr(X), SC_F32 if X.dtype == np.float32 else SC_F64, n, D, K,
                                            MIX_COVARIANCES[covariance_type], _ptr(w), _ptr(mu), _ptr(cov), _ptr(labels),
                                            _ptr(proba), byref(ll)))
        return labels, proba, ll.value

    # ---- N12 (extension): NMF ---------------------------------------------------------------
    def nmf_fit(self, indptr, indices, data, n_genes: int, W0, H0, loss: str, update_H: bool = True, max_iter: int = 200,
                tol: float = 1e-4) -> dict:
        """sc_nmf_fit on a canonical CSR (values float32 or float64) from the starting factors ``W0`` (n, K) and ``H0``
        (K, n_genes): ``W`` / ``H`` float64, ``n_iter``, ``reconstruction_err`` and ``error_trace`` (the error at the start
        and at every check)."""
        data = np.ascontiguousarray(data)
        if data.dtype not in (np.float32, np.float64):
            raise ValueError(f"nmf_fit: values must be float32 or float64, got {data.dtype}")
        indptr, indices = _c(indptr, np.int64), _c(indices, np.int32)
        W, H = np.array(W0, dtype=np.float64, order="C"), np.array(H0, dtype=np.float64, order="C")
        n, G = indptr.size - 1, int(n_genes)
        if W.ndim != 2 or H.ndim != 2 or W.shape[0] != n or H.shape != (W.shape[1], G):
            raise ValueError(f"nmf_fit: W0 must be (n, K) and H0 (K, n_genes), got {W.shape} and {H.shape}")
        if indices.size != data.size or n < 1 or indptr[-1] != data.size:
            raise ValueError("nmf_fit: indptr, indices and values do not describe one CSR matrix")
        trace = np.zeros(2 + max(int(max_iter), 0) // 10, dtype=np.float64)
        checks, n_iter, err = c_int32(0), c_int32(0), c_double(0.0)
        _check(self._lib.sc_nmf_fit(self._h, _ptr(indptr), _ptr(indices), _ptr(data),
                                    SC_F32 if data.dtype == np.float32 else SC_F64, n, G, W.shape[1], NMF_LOSSES[loss],
                                    int(bool(update_H)), int(max_iter), float(tol), _ptr(W), _ptr(H), _ptr(trace),
                                    byref(checks), byref(n_iter), byref(err)))
        return {"W": W, "H": H, "n_iter": n_iter.value, "reconstruction_err": err.value,
                "error_trace": trace[:checks.value].copy()}

    def nmf_fit_graph(self, indptr, indices, data, n_genes: int, gptr, gidx, gval, spatial_alpha: float, W0, H0,
                      max_iter: int = 200, tol: float = 1e-4) -> dict:
        """sc_nmf_fit_graph: graph-regularised NMF (Frobenius loss) of a canonical CSR over the symmetric graph
        (``gptr``, ``gidx``, ``gval``), n x n canonical CSR without a diagonal.  The keys of ``nmf_fit`` plus
        ``objective_trace`` (sqrt(2 max(F, 0)) at the start and at every check) and ``penalty`` = tr(W^T L W)."""
        data = np.ascontiguousarray(data)
        if data.dtype not in (np.float32, np.float64):
            raise ValueError(f"nmf_fit_graph: values must be float32 or float64, got {data.dtype}")
        indptr, indices = _c(indptr, np.int64), _c(indices, np.int32)
        gptr, gidx, gval = _c(gptr, np.int64), _c(gidx, np.int32), _c(gval, np.float64)
        W, H = np.array(W0, dtype=np.float64, order="C"), np.array(H0, dtype=np.float64, order="C")
        n, G = indptr.size - 1, int(n_genes)
        if W.ndim != 2 or H.ndim != 2 or W.shape[0] != n or H.shape != (W.shape[1], G):
            raise ValueError(f"nmf_fit_graph: W0 must be (n, K) and H0 (K, n_genes), got {W.shape} and {H.shape}")
        if indices.size != data.size or n < 1 or indptr[-1] != data.size:
            raise ValueError("nmf_fit_graph: indptr, indices and values do not describe one CSR matrix")
        if gptr.size != n + 1 or gidx.size != gval.size or gptr[-1] != gval.size:
            raise ValueError("nmf_fit_graph: gptr, gidx and gval do not describe one n x n CSR matrix")
        slots = 2 + max(int(max_iter), 0) // 10
        obj, trace = np.zeros(slots, dtype=np.float64), np.zeros(slots, dtype=np.float64)
        checks, n_iter, err, pen = c_int32(0), c_int32(0), c_double(0.0), c_double(0.0)
        _check(self._lib.sc_nmf_fit_graph(self._h, _ptr(indptr), _ptr(indices), _ptr(data),
                                          SC_F32 if data.dtype == np.float32 else SC_F64, n, G, W.shape[1], _ptr(gptr),
                                          _ptr(gidx), _ptr(gval), float(spatial_alpha), int(max_iter), float(tol), _ptr(W),
                                          _ptr(H), _ptr(obj), _ptr(trace), byref(checks), byref(n_iter), byref(err), byref(pen)))
        return {"W": W, "H": H, "n_iter": n_iter.value, "reconstruction_err": err.value, "penalty": pen.value,
                "error_trace": trace[:checks.value].copy(), "objective_trace": obj[:checks.value].copy()}

    # ---- N14 (extension): annotation ----------------------------------------------------------
    @staticmethod
    def _annot_csr(indptr, indices, data, who: str):
        data = np.ascontiguousarray(data)
        if data.dtype not in (np.float32, np.float64):
            raise ValueError(f"{who}: values must be float32 or float64, got {data.dtype}")
        indptr, indices = _c(indptr, np.int64), _c(indices, np.int32)
        n = indptr.size - 1
        if indices.size != data.size or n < 1 or indptr[-1] != data.size:
            raise ValueError(f"{who}: indptr, indices and values do not describe one CSR matrix")
        return indptr, indices, data, n

    def annot_predict(self, indptr, indices, data, mode: str, coef, intercept, mean, scale, scores: bool = True) -> dict:
        """sc_annot_predict on a canonical CSR over the model's genes: ``labels`` (int32, first argmax of the fp64
        scores), ``confidence_raw`` = expit(max score), ``raw`` / ``zscore`` / ``softmax`` / ``minmax`` (the reference's
        transforms of the float32-rounded row) and, with ``scores``, the float32 ``scores`` (n, T)."""
        indptr, indices, data, n = self._annot_csr(indptr, indices, data, "annot_predict")
        coef, b = _c(coef, np.float64), _c(intercept, np.float64)
        mean, scale = _c(mean, np.float64), _c(scale, np.float64)
        if coef.ndim != 2 or b.shape != (coef.shape[0],) or mean.shape != (coef.shape[1],) or scale.shape != mean.shape:
            raise ValueError("annot_predict: coef must be (T, G), intercept (T,), mean and scale (G,)")
        T, G = coef.shape
        out = np.empty((n, T), dtype=np.float32) if scores else None
        lab = np.empty(n, dtype=np.int32)
        conf = np.empty((5, n), dtype=np.float64)
        _check(self._lib.sc_annot_predict(self._h, _ptr(indptr), _ptr(indices), _ptr(data),
                                          SC_F32 if data.dtype == np.float32 else SC_F64, n, G, ANNOT_MODES[mode], T, _ptr(coef),
                                          _ptr(b), _ptr(mean), _ptr(scale), _ptr(out), _ptr(lab), _ptr(conf)))
        return {"labels": lab, "confidence_raw": conf[0], "raw": conf[1], "zscore": conf[2], "softmax": conf[3],
                "minmax": conf[4], "scores": out}

    def annot_transform(self, scores) -> dict:
        """sc_annot_transform: the four confidence transforms of an (n, T) float32 or float64 matrix."""
        S = np.ascontiguousarray(scores)
        if S.dtype not in (np.float32, np.float64) or S.ndim != 2:
            raise ValueError("annot_transform: scores must be a 2-D float32 or float64 matrix")
        n, T = S.shape
        conf = np.empty((4, n), dtype=np.float64)
        _check(self._lib.sc_annot_transform(self._h, _ptr(S), SC_F32 if S.dtype == np.float32 else SC_F64, n, T, _ptr(conf)))
        return {"raw": conf[0], "zscore": conf[1], "softmax": conf[2], "minmax": conf[3]}

    def annot_train_begin(self, indptr, indices, data, n_genes: int, mode: str, n_classes: int, labels, weights):
        """sc_annot_train_begin: leaves the training problem on the device; returns the scaler's (mean, scale)."""
        indptr, indices, data, n = self._annot_csr(indptr, indices, data, "annot_train_begin")
        labels, weights = _c(labels, np.int32), _c(weights, np.float64)
        if labels.shape != (n,) or weights.shape != (n,):
            raise ValueError("annot_train_begin: labels and weights must have one entry per cell")
        G, T = int(n_genes), int(n_classes)
        self._annot_shape = None   # until the call succeeds this object vouches for no resident problem
        mean, scale = np.empty(max(G, 1), dtype=np.float64), np.empty(max(G, 1), dtype=np.float64)
        _check(self._lib.sc_annot_train_begin(self._h, _ptr(indptr), _ptr(indices), _ptr(data),
                                              SC_F32 if data.dtype == np.float32 else SC_F64, n, G, ANNOT_MODES[mode], T,
                                              _ptr(labels), _ptr(weights), _ptr(mean), _ptr(scale)))
        self._annot_shape = (T, G)
        return mean[:G], scale[:G]

    def annot_train_forward(self, coef, bias, direction: bool = False) -> None:
        """The resident scores (or, with ``direction``, the direction's product) <- Z coef^T + bias."""
        T, G = self._annot_dims("annot_train_forward")
        coef, bias = _c(coef, np.float64), _c(bias, np.float64)
        if coef.shape != (T, G) or bias.shape != (T,):
            raise ValueError(f"annot_train_forward: coef must be ({T}, {G}) and bias ({T},)")
        _check(self._lib.sc_annot_train_forward(self._h, _ptr(coef), _ptr(bias), int(bool(direction))))

    def annot_train_grad(self):
        """(gradient of the data term at the resident scores, (T, G + 1) with the intercept last; data loss per class)."""
        T, G = self._annot_dims("annot_train_grad")
        grad, loss = np.empty((T, G + 1), dtype=np.float64), np.empty(T, dtype=np.float64)
        _check(self._lib.sc_annot_train_grad(self._h, _ptr(grad), _ptr(loss)))
        return grad, loss

    def annot_train_line(self, alpha):
        """First and second derivative of the data term along the resident direction at the step lengths ``alpha``."""
        T, _ = self._annot_dims("annot_train_line")
        alpha = _c(alpha, np.float64)
        if alpha.shape != (T,):
            raise ValueError(f"annot_train_line: alpha must be ({T},)")
        d1, d2 = np.empty(T, dtype=np.float64), np.empty(T, dtype=np.float64)
        _check(self._lib.sc_annot_train_line(self._h, _ptr(alpha), _ptr(d1), _ptr(d2)))
        return d1, d2

    def annot_train_step(self, alpha) -> None:
        T, _ = self._annot_dims("annot_train_step")
        alpha = _c(alpha, np.float64)
        if alpha.shape != (T,):
            raise ValueError(f"annot_train_step: alpha must be ({T},)")
        _check(self._lib.sc_annot_train_step(self._h, _ptr(alpha)))

    def annot_train_end(self) -> None:
        self._annot_shape = None
        _check(self._lib.sc_annot_train_end(self._h))

    def _annot_dims(self, who: str):
        """(classes, genes) of the resident training problem; without one, the library's own state error."""
        if self._annot_shape is None:
            raise SpatialCoreHipError(f"{who}: no training problem is resident (annot_train_begin)")
        return self._annot_shape

    # ---- N15 (extension): PCA ------------------------------------------------------------------
    def pca_begin(self, indptr, indices, data, n_genes: int, normalize: bool = False, target_sum: float = 1e4) -> None:
        """sc_pca_begin: validates a canonical CSR over the genes in use and leaves its fp64 values on the device, as they
        are or as ``log1p(x / rowsum * target_sum)``.  A second call replaces the resident matrix."""
        indptr, indices, data, n = self._annot_csr(indptr, indices, data, "pca_begin")
        self._pca_shape = None   # until the call succeeds this object vouches for no resident matrix
        _check(self._lib.sc_pca_begin(self._h, _ptr(indptr), _ptr(indices), _ptr(data),
                                      SC_F32 if data.dtype == np.float32 else SC_F64, n, int(n_genes), int(bool(normalize)),
                                      float(target_sum)))
        self._pca_shape = (n, int(n_genes))
        self._pca_nnz = int(data.size)

    def pca_values(self) -> np.ndarray:
        """sc_pca_values: the resident fp64 values, one per stored entry in CSR order (the normalised ones after
        ``normalize``): what sc_pca_gram and sc_pca_project read."""
        self._pca_dims("pca_values")
        out = np.empty(self._pca_nnz, dtype=np.float64)
        _check(self._lib.sc_pca_values(self._h, _ptr(out)))
        return out

    def pca_gram(self):
        """sc_pca_gram: (column sums (G,), Gram matrix X^T X (G, G)) of the resident values, float64."""
        _, G = self._pca_dims("pca_gram")
        colsum, gram = np.empty(G, dtype=np.float64), np.empty((G, G), dtype=np.float64)
        _check(self._lib.sc_pca_gram(self._h, _ptr(colsum), _ptr(gram)))
        return colsum, gram

    def pca_project(self, V, offset, dtype=np.float64) -> np.ndarray:
        """sc_pca_project: ``X V^T - offset`` of the resident values, (n, K) in ``dtype`` (float64, or float32 = the
        float64 result rounded once).  ``V`` is (K, G), ``offset`` (K,)."""
        n, G = self._pca_dims("pca_project")
        V, offset = _c(V, np.float64), _c(offset, np.float64)
        if V.ndim != 2 or V.shape[1] != G or offset.shape != (V.shape[0],):
            raise ValueError(f"pca_project: V must be (K, {G}) and offset (K,)")
        dtype = np.dtype(dtype)
        if dtype not in (np.float32, np.float64):
            raise ValueError(f"pca_project: dtype must be float32 or float64, got {dtype}")
        out = np.empty((n, V.shape[0]), dtype=dtype)
        _check(self._lib.sc_pca_project(self._h, _ptr(V), _ptr(offset), V.shape[0], SC_F32 if dtype == np.float32 else SC_F64,
                                        _ptr(out)))
        return out

    def pca_end(self) -> None:
        self._pca_shape = None
        _check(self._lib.sc_pca_end(self._h))

    def _pca_dims(self, who: str):
        """(cells, genes) of the resident matrix; without one, the library's own state error."""
        if self._pca_shape is None:
            raise SpatialCoreHipError(f"{who}: no matrix is resident (pca_begin)")
        return self._pca_shape

    # ---- N18 (extension): Pearson-residual gene selection ------------------------------------
    def hvg_pearson(self, indptr, indices, data, n_genes: int, theta: float, clip: float):
        """sc_hvg_pearson on a canonical CSR of counts: per gene (sum x, sum x^2, mean of the clipped Pearson residuals,
        their population variance over all cells), float64.  Validated on the host before the device is touched."""
        indptr, indices, data, n = self._annot_csr(indptr, indices, data, "hvg_pearson")
        G = int(n_genes)
        if not 1 <= G <= 32768:
            raise ValueError(f"hvg_pearson: need 1 <= n_genes <= 32768, got {G}")
        out = np.empty((4, G), dtype=np.float64)
        _check(self._lib.sc_hvg_pearson(self._h, _ptr(indptr), _ptr(indices), _ptr(data),
                                        SC_F32 if data.dtype == np.float32 else SC_F64, n, G, float(theta), float(clip),
                                        _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3])))
        return out[0], out[1], out[2], out[3]


    # ---- N19: harmony_integrate ----------------------------------------------------------------
    def harmony_begin(self, Z, batch, n_batches: int, Y, n_blocks: int, sigma: float, theta: float, lamb: float) -> float:
        """sc_harmony_begin: leaves Z (n, d; float32 or float64), its unit rows, the assignments from the centres Y (K, d) and
        the per-block tables on the device; returns the objective of that state."""
        Z = np.ascontiguousarray(Z)
        if Z.dtype not in (np.float32, np.float64) or Z.ndim != 2:
            raise ValueError(f"harmony_begin: Z must be a 2-D float32 or float64 array, got {Z.dtype} {Z.shape}")
        batch, Y = _c(batch, np.int32), _c(Y, np.float64)
        n, d = Z.shape
        if batch.shape != (n,) or Y.ndim != 2 or Y.shape[1] != d:
            raise ValueError(f"harmony_begin: batch must have {n} entries and Y {d} columns")
        self._harmony = None   # until the call succeeds this object vouches for no resident problem
        obj = c_double(0.0)
        _check(self._lib.sc_harmony_begin(self._h, _ptr(Z), SC_F32 if Z.dtype == np.float32 else SC_F64, n, d, _ptr(batch),
                                          int(n_batches), _ptr(Y), Y.shape[0], int(n_blocks), float(sigma), float(theta),
                                          float(lamb), byref(obj)))
        self._harmony = (n, d, Y.shape[0], int(n_batches), int(n_blocks))
        return obj.value

    def _harmony_dims(self, who: str):
        if self._harmony is None:
            raise SpatialCoreHipError(f"{who}: no problem is resident (harmony_begin)")
        return self._harmony

    def harmony_cluster(self, max_iter: int, epsilon: float) -> np.ndarray:
        """sc_harmony_cluster: the objective after every clustering round done (at most ``max_iter``; ``epsilon`` < 0 runs
        them all)."""
        self._harmony_dims("harmony_cluster")
        if not 1 <= int(max_iter) <= 4096:
            raise ValueError(f"harmony_cluster: need 1 <= max_iter <= 4096, got {max_iter}")
        out = np.empty(int(max_iter), dtype=np.float64)
        rounds = c_int32(0)
        _check(self._lib.sc_harmony_cluster(self._h, int(max_iter), float(epsilon), byref(rounds), _ptr(out)))
        return out[:rounds.value].copy()

    def harmony_correct(self) -> None:
        """sc_harmony_correct: the ridge correction from the resident assignments; Zcorr, Zc and W change."""
        self._harmony_dims("harmony_correct")
        _check(self._lib.sc_harmony_correct(self._h))

    def harmony_get(self, name: str) -> np.ndarray:
        """sc_harmony_get: "Zcorr" / "Zc" (n, d), "R" / "dist" (n, K), "Y" (K, d), "O" (blocks, K, B), "W" (K, B, d) as
        float64 in the caller's cell order; "order" (n,) int64, the cell at every position of the device's sort."""
        n, d, K, B, nb = self._harmony_dims("harmony_get")
        if name not in HARMONY_ARRAYS:
            raise ValueError(f"harmony_get: unknown array {name!r}; one of {sorted(HARMONY_ARRAYS)}")
        shape = {"Zcorr": (n, d), "Zc": (n, d), "R": (n, K), "dist": (n, K), "Y": (K, d), "O": (nb, K, B), "W": (K, B, d),
                 "order": (n,)}[name]
        out = np.empty(shape, dtype=np.int64 if name == "order" else np.float64)
        _check(self._lib.sc_harmony_get(self._h, HARMONY_ARRAYS[name], _ptr(out)))
        return out

    def harmony_end(self) -> None:
        self._harmony = None
        _check(self._lib.sc_harmony_end(self._h))

    # ---- N20: aggregate_neighbors --------------------------------------------------------------
    def hop_begin(self, indptr, indices, n: int) -> None:
        """sc_hop_begin: leaves the pattern (canonical CSR without a diagonal, n x n) resident as shell 1."""
        indptr, indices = _c(indptr, np.int64), _c(indices, np.int32)
        if indptr.ndim != 1 or indptr.size != int(n) + 1 or indices.ndim != 1 or (indptr.size and indices.size != int(indptr[-1])):
            raise ValueError(f"hop_begin: indptr must have {int(n) + 1} entries and indices indptr[-1], got {indptr.shape} and {indices.shape}")
        self._hop = None   # until the call succeeds this object vouches for no resident graph
        _check(self._lib.sc_hop_begin(self._h, _ptr(indptr), _ptr(indices), int(n)))
        self._hop = [int(n), int(indices.size), None]

    def _hop_state(self, who: str):
        if self._hop is None:
            raise SpatialCoreHipError(f"{who}: no graph is resident (hop_begin)")
        return self._hop

    def hop_next(self) -> Tuple[int, int, int]:
        """sc_hop_next: the next shell becomes resident; (its stored entries, its longest row, its empty rows)."""
        st = self._hop_state("hop_next")
        nnz, longest, empty = c_int64(0), c_int32(0), c_int64(0)
        _check(self._lib.sc_hop_next(self._h, byref(nnz), byref(longest), byref(empty)))
        st[1] = nnz.value
        return nnz.value, longest.value, empty.value

    def hop_get(self) -> Tuple[np.ndarray, np.ndarray]:
        """sc_hop_get: the resident shell as canonical CSR (int64 indptr, int32 indices)."""
        n, nnz, _ = self._hop_state("hop_get")
        indptr, indices = np.empty(n + 1, dtype=np.int64), np.empty(nnz, dtype=np.int32)
        _check(self._lib.sc_hop_get(self._h, _ptr(indptr), _ptr(indices)))
        return indptr, indices

    def hop_aggregate(self, X, what: str) -> np.ndarray:
        """sc_hop_aggregate: "mean" or "var" of X (n, d; float32 or float64) over the resident shell, (n, d) float64.  X goes
        to the device once per hop_begin as long as the same array is handed in."""
        st = self._hop_state("hop_aggregate")
        if what not in HOP_AGGREGATIONS:
            raise ValueError(f"hop_aggregate: unknown aggregation {what!r}; one of {sorted(HOP_AGGREGATIONS)}")
        if st[2] is None or st[2][0] is not X:
            if not isinstance(X, np.ndarray) or X.ndim != 2 or X.shape[0] != st[0] or X.dtype not in (np.float32, np.float64):
                raise ValueError(f"hop_aggregate: X must be a float32 or float64 array with {st[0]} rows, got {getattr(X, 'dtype', None)} "
                                 f"{getattr(X, 'shape', None)}")
            st[2] = (X, np.ascontiguousarray(X))   # the contiguous array is the one the library saw: kept, so its address stays
        Xc = st[2][1]
        out = np.empty(Xc.shape, dtype=np.float64)
        _check(self._lib.sc_hop_aggregate(self._h, _ptr(Xc), SC_F32 if Xc.dtype == np.float32 else SC_F64, Xc.shape[1],
                                          HOP_AGGREGATIONS[what], _ptr(out)))
        return out

    def hop_times(self) -> dict:
        """sc_hop_times: milliseconds of the last hop_next's count, fill and sort and of the last hop_aggregate's kernel."""
        self._hop_state("hop_times")
        ms = np.zeros(4)
        _check(self._lib.sc_hop_times(self._h, _ptr(ms)))
        return dict(zip(("count", "fill", "sort", "aggregate"), ms.tolist()))

    def hop_end(self) -> None:
        self._hop = None
        _check(self._lib.sc_hop_end(self._h))

    # ---- N16 (extension): Louvain communities ---------------------------------------------------
    def louvain_begin(self, indptr, indices, q, g: int, max_rounds: int) -> None:
        """sc_louvain_begin: a symmetric canonical CSR with integer weights in [1, 65535] becomes level 0 of a new
        hierarchy; ``g`` = rint(resolution 2^16).  Everything is validated on the host before the device is touched."""
        indptr, indices, q = _c(indptr, np.int64), _c(indices, np.int32), _c(q, np.uint16)
        n = indptr.size - 1
        if indptr.ndim != 1 or n < 1 or indices.shape != q.shape or indices.ndim != 1 or indptr[-1] != q.size:
            raise ValueError("louvain_begin: indptr, indices and weights do not describe one CSR matrix")
        self._louvain_n = None
        _check(self._lib.sc_louvain_begin(self._h, _ptr(indptr), _ptr(indices), _ptr(q), n, int(g), int(max_rounds)))
        self._louvain_n = n

    def louvain_resident_weights(self) -> np.ndarray:
        """sc_louvain_resident_weights: the fp64 kernel weights of the graph ``diffmap_graph`` left on the device, in CSR
        order (its structure stays where it is)."""
        w = np.empty(self._diff_nnz, dtype=np.float64)
        _check(self._lib.sc_louvain_resident_weights(self._h, _ptr(w), int(w.size)))
        return w

    def louvain_begin_resident(self, q, g: int, max_rounds: int) -> None:
        """sc_louvain_begin_resident: level 0 = the structure of the resident ``diffmap_graph`` with the integer weights
        ``q`` in CSR order (None: 1 per edge); the symmetry is checked on the device."""
        if q is not None:
            q = _c(q, np.uint16)
            if q.shape != (self._diff_nnz,):
                raise ValueError(f"louvain_begin_resident: need {self._diff_nnz} weights, got shape {q.shape}")
        self._louvain_n = None
        _check(self._lib.sc_louvain_begin_resident(self._h, _ptr(q), int(self._diff_nnz), int(g), int(max_rounds)))
        self._louvain_n = int(self._diff_n)

    def louvain_level(self, labels: bool = True) -> dict:
        """sc_louvain_level: runs the next level and returns its record; ``qnum`` is the exact Python integer."""
        if self._louvain_n is None:
            raise SpatialCoreHipError("louvain_level: no graph is resident (louvain_begin)")
        info = np.zeros(12, dtype=np.int64)
        lab = np.empty(self._louvain_n, dtype=np.int32) if labels else None
        _check(self._lib.sc_louvain_level(self._h, _ptr(info), _ptr(lab)))
        self._louvain_n = int(info[3])
        return {"n_vertices": int(info[0]), "rounds": int(info[1]), "n_best": int(info[2]), "n_communities": int(info[3]),
                "qnum": (int(info[4]) << 64) + (int(info[5]) & 0xFFFFFFFFFFFFFFFF), "finished": bool(info[6]),
                "hit_max_rounds": bool(info[7]), "rows_wavefront": int(info[8]), "rows_workgroup": int(info[9]),
                "rows_global": int(info[10]), "nnz": int(info[11]), "labels": lab}

    def louvain_labels(self, n: int) -> np.ndarray:
        """sc_louvain_labels: the labels of the ``n`` input vertices after the levels run so far, clusters numbered by
        descending size (ties: the smaller smallest member)."""
        out = np.empty(int(n), dtype=np.int32)
        nc = c_int64(0)
        _check(self._lib.sc_louvain_labels(self._h, _ptr(out), byref(nc)))
        return out

    def louvain_end(self) -> None:
        self._louvain_n = None
        _check(self._lib.sc_louvain_end(self._h))

    # ---- N13 (extension): diffusion maps ------------------------------------------------------
    @staticmethod
    def _dense_features(who, X, k, fetch):
        """``knn_dense`` / ``knn_dense_gram`` before the call: (features, dtype code, indices, squared distances or None)."""
        X = np.ascontiguousarray(X)
        if X.dtype not in (np.float32, np.float64):
            raise ValueError(f"{who}: features must be float32 or float64, got {X.dtype}")
        if X.ndim != 2:
            raise ValueError(f"{who}: features must have shape (n, d), got {X.shape}")
        n = X.shape[0]
        idx = np.empty((n, int(k)), dtype=np.int32) if fetch else None
        d2 = np.empty((n, int(k)), dtype=np.float64) if fetch else None
        return X, SC_F32 if X.dtype == np.float32 else SC_F64, idx, d2

    def knn_dense(self, X, k: int, fetch: bool = True, splits: int = 0):
        """sc_knn_dense: the exact k nearest neighbours of every row of ``X`` (n, d), float32 or float64, by (squared
        distance, index).  The lists stay on the device for ``diffmap_graph``; ``fetch`` also returns (indices, squared
        distances).  ``splits`` forces a number of candidate splits (0: the library's choice; the result never differs)."""
        X, dtype, idx, d2 = self._dense_features("knn_dense", X, k, fetch)
        n, d = X.shape
        _check(self._lib.sc_knn_dense(self._h, _ptr(X), dtype, n, d, int(k), int(splits), _ptr(idx), _ptr(d2)))
        self._diff_n = n
        return (idx, d2) if fetch else None

    def knn_dense_gram(self, X, k: int, fetch: bool = True, path: int = 0, slack: int = 0):
        """sc_knn_dense_gram: the lists of ``knn_dense``, bit for bit, through the certified Gram-form filter on the fp64
        matrix cores.  ``path``: 0 the library's choice, 1 the direct kernels, 2 the filter; ``slack``: list entries the
        filter keeps beyond ``k`` (0: the library's choice).  Returns (indices, squared distances, info) -- the first two
        None without ``fetch`` -- with ``info`` = {``path``, ``list_length``, ``rows_certified``, ``rows_fallback``}."""
        X, dtype, idx, d2 = self._dense_features("knn_dense_gram", X, k, fetch)
        n, d = X.shape
        info = np.zeros(4, dtype=np.int64)
        _check(self._lib.sc_knn_dense_gram(self._h, _ptr(X), dtype, n, d, int(k), int(path), int(slack), _ptr(idx), _ptr(d2),
                                           _ptr(info)))
        self._diff_n = n
        return idx, d2, {"path": int(info[0]), "list_length": int(info[1]), "rows_certified": int(info[2]),
                         "rows_fallback": int(info[3])}

    def knn_cross(self, R, Q, k: int, fetch: bool = True, path: int = 0, slack: int = 0):
        """sc_knn_cross: for every row of ``Q`` (n_query, d) the ``k`` rows of ``R`` (n_ref, d) smallest in (squared
        distance, index); nothing is excluded.  Either array float32 or float64.  ``path`` and ``slack`` as
        ``knn_dense_gram``; the lists are the same bytes whatever they are.  The lists stay on the device for
        ``cross_vote`` and ``cross_regress``, and no self lists or graph stay resident.  Returns (indices, squared
        distances, info) as ``knn_dense_gram``."""
        R, dtype_r, _, _ = self._dense_features("knn_cross", R, k, False)
        Q, dtype_q, idx, d2 = self._dense_features("knn_cross", Q, k, fetch)
        if R.shape[1] != Q.shape[1]:
            raise ValueError(f"knn_cross: the reference has {R.shape[1]} columns and the queries have {Q.shape[1]}")
        info = np.zeros(4, dtype=np.int64)
        self._cross_nq = None
        _check(self._lib.sc_knn_cross(self._h, _ptr(R), dtype_r, R.shape[0], _ptr(Q), dtype_q, Q.shape[0], R.shape[1], int(k),
                                      int(path), int(slack), _ptr(idx), _ptr(d2), _ptr(info)))
        self._cross_nq, self._cross_nref = Q.shape[0], R.shape[0]
        return idx, d2, {"path": int(info[0]), "list_length": int(info[1]), "rows_certified": int(info[2]),
                         "rows_fallback": int(info[3])}

    def _cross_shape(self, who):
        if self._cross_nq is None:
            raise SpatialCoreHipError(f"{who}: no cross lists are resident (call knn_cross first)")
        return self._cross_nq, self._cross_nref

    def cross_vote(self, codes_ref, n_classes: int, weighting: str = "uniform", proba: bool = False):
        """sc_cross_vote on the lists of the last ``knn_cross``: ``codes_ref`` (n_ref,) integer codes in [0, n_classes).
        ``weighting`` "uniform" or "distance" (sklearn's).  Returns (labels int32, confidence float64, probabilities
        (n_query, n_classes) or None); ties go to the lowest code."""
        nq, nref = self._cross_shape("cross_vote")
        if weighting not in CROSS_WEIGHTINGS:
            raise ValueError(f"cross_vote: weighting must be one of {sorted(CROSS_WEIGHTINGS)}, got {weighting!r}")
        codes = np.ascontiguousarray(codes_ref, dtype=np.int32)
        if codes.shape != (nref,):
            raise ValueError(f"cross_vote: codes_ref must have shape ({nref},), got {codes.shape}")
        label = np.empty(nq, dtype=np.int32)
        conf = np.empty(nq, dtype=np.float64)
        P = np.empty((nq, int(n_classes)), dtype=np.float64) if proba else None
        _check(self._lib.sc_cross_vote(self._h, _ptr(codes), int(n_classes), CROSS_WEIGHTINGS[weighting], _ptr(label), _ptr(conf),
                                       _ptr(P)))
        return label, conf, P

    def cross_regress(self, Y_ref, weighting: str = "uniform") -> np.ndarray:
        """sc_cross_regress on the lists of the last ``knn_cross``: the weighted average of the neighbours' rows of
        ``Y_ref`` (n_ref, C), float32 or float64, C <= 64, in list order; float64 (n_query, C)."""
        nq, nref = self._cross_shape("cross_regress")
        if weighting not in CROSS_WEIGHTINGS:
            raise ValueError(f"cross_regress: weighting must be one of {sorted(CROSS_WEIGHTINGS)}, got {weighting!r}")
        Y = np.ascontiguousarray(Y_ref)
        if Y.dtype not in (np.float32, np.float64):
            Y = Y.astype(np.float64)
        if Y.ndim != 2 or Y.shape[0] != nref:
            raise ValueError(f"cross_regress: Y_ref must have shape ({nref}, C), got {Y.shape}")
        out = np.empty((nq, Y.shape[1]), dtype=np.float64)
        _check(self._lib.sc_cross_regress(self._h, _ptr(Y), SC_F32 if Y.dtype == np.float32 else SC_F64, Y.shape[1],
                                          CROSS_WEIGHTINGS[weighting], _ptr(out)))
        return out

    def diffmap_graph(self) -> dict:
        """sc_diffmap_graph on the lists of the last ``knn_dense``: ``s2`` (local scales), ``n_edges`` (stored entries of
        the symmetric kernel matrix), ``n_components``.  A zero scale raises ValueError."""
        s2 = np.empty(self._diff_n, dtype=np.float64)
        ne, nc = c_int64(0), c_int64(0)
        _check(self._lib.sc_diffmap_graph(self._h, _ptr(s2), byref(ne), byref(nc)))
        self._diff_nnz = ne.value
        return {"s2": s2, "n_edges": ne.value, "n_components": nc.value}

    def fuzzy_graph(self) -> dict:
        """sc_fuzzy_graph on the lists of the last ``knn_dense``: UMAP's fuzzy simplicial set becomes the resident graph.
        ``rho`` (first non-zero distances), ``sigma`` (bandwidths), ``n_edges``, ``n_components``."""
        rho = np.empty(self._diff_n, dtype=np.float64)
        sigma = np.empty(self._diff_n, dtype=np.float64)
        ne, nc = c_int64(0), c_int64(0)
        _check(self._lib.sc_fuzzy_graph(self._h, _ptr(rho), _ptr(sigma), byref(ne), byref(nc)))
        self._diff_nnz = ne.value
        return {"rho": rho, "sigma": sigma, "n_edges": ne.value, "n_components": nc.value}

    def umap_layout(self, graph, Y, a: float, b: float, gamma: float, alpha0: float, neg: int, n_epochs: int, seed: int,
                    e0: int = 0, e1: Optional[int] = None) -> np.ndarray:
        """sc_umap_layout: epochs [e0, e1) (default: all) of the deterministic layout on ``graph`` = (indptr, indices, w)
        of a symmetric canonical CSR, or None for the graph resident on the device.  ``Y`` (n, 2 or 3) is the start;
        returns the new positions (float64), ``Y`` itself is not written."""
        Y = np.array(Y, dtype=np.float64, order="C", copy=True)
        if Y.ndim != 2:
            raise ValueError(f"umap_layout: positions must have shape (n, components), got {Y.shape}")
        n = Y.shape[0]
        if graph is None:
            indptr = indices = w = None
        else:
            indptr, indices, w = _c(graph[0], np.int64), _c(graph[1], np.int32), _c(graph[2], np.float64)
            if indptr.size != n + 1 or indices.size != w.size or indptr[-1] != w.size:
                raise ValueError("umap_layout: indptr, indices and values do not describe one CSR matrix of the positions' rows")
        _check(self._lib.sc_umap_layout(self._h, _ptr(indptr), _ptr(indices), _ptr(w), n, _ptr(Y), int(Y.shape[1]), float(a),
                                        float(b), float(gamma), float(alpha0), int(neg), int(n_epochs),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(e0), int(n_epochs if e1 is None else e1)))
        return Y

    def diffmap_graph_csr(self, indptr, indices, w) -> int:
        """sc_diffmap_graph_csr: a caller's symmetric kernel matrix (canonical CSR) becomes the resident graph; returns
        the number of connected components."""
        indptr, indices, w = _c(indptr, np.int64), _c(indices, np.int32), _c(w, np.float64)
        n = indptr.size - 1
        if n < 1 or indices.size != w.size or indptr[-1] != w.size:
            raise ValueError("diffmap_graph_csr: indptr, indices and values do not describe one CSR matrix")
        nc = c_int64(0)
        _check(self._lib.sc_diffmap_graph_csr(self._h, _ptr(indptr), _ptr(indices), _ptr(w), n, byref(nc)))
        self._diff_n, self._diff_nnz = n, int(w.size)
        return nc.value

    def diffmap_graph_get(self, transition: bool = False):
        """(indptr, indices, w) of the resident kernel matrix, rows sorted by column; with ``transition`` also T."""
        indptr = np.empty(self._diff_n + 1, dtype=np.int64)
        indices = np.empty(self._diff_nnz, dtype=np.int32)
        w = np.empty(self._diff_nnz, dtype=np.float64)
        T = np.empty(self._diff_nnz, dtype=np.float64) if transition else None
        _check(self._lib.sc_diffmap_graph_get(self._h, _ptr(indptr), _ptr(indices), _ptr(w), _ptr(T)))
        return (indptr, indices, w, T) if transition else (indptr, indices, w)

    def lanczos_begin(self, start, max_basis: int) -> None:
        v = _c(start, np.float64)
        if v.shape != (self._diff_n,):
            raise ValueError(f"lanczos_begin: the start vector must have shape ({self._diff_n},), got {v.shape}")
        _check(self._lib.sc_lanczos_begin(self._h, _ptr(v), int(max_basis)))
        self._lanczos_cap = int(max_basis)

    def lanczos_run(self, steps: int):
        """``steps`` more Lanczos steps; returns (alpha[m], beta[m + 1]) of all m steps so far (beta[0] = the start
        vector's norm).  A Krylov breakdown raises RuntimeError."""
        alpha = np.zeros(self._lanczos_cap, dtype=np.float64)
        beta = np.zeros(self._lanczos_cap + 1, dtype=np.float64)
        m = c_int64(0)
        _check(self._lib.sc_lanczos_run(self._h, int(steps), _ptr(alpha), _ptr(beta), byref(m)))
        return alpha[:m.value].copy(), beta[:m.value + 1].copy()

    def lanczos_ritz(self, S, lam):
        """Ritz vectors V S (S: m x c) scaled to unit norm, as (n, c), and their true residuals ||T y - lam y||."""
        S, lam = _c(S, np.float64), _c(lam, np.float64)
        if S.ndim != 2 or lam.shape != (S.shape[1],):
            raise ValueError(f"lanczos_ritz: S must be (m, c) and lam (c,), got {S.shape} and {lam.shape}")
        vecs = np.empty((S.shape[1], self._diff_n), dtype=np.float64)
        res = np.empty(S.shape[1], dtype=np.float64)
        _check(self._lib.sc_lanczos_ritz(self._h, _ptr(S), S.shape[0], S.shape[1], _ptr(lam), _ptr(vecs), _ptr(res)))
        return np.ascontiguousarray(vecs.T), res

    def lanczos_end(self) -> None:
        _check(self._lib.sc_lanczos_end(self._h))

    # ---- N4 (extension) ---------------------------------------------------------------------
    def enrichment_counts(self, labels, n_types: int, n_perm: int, perm_row0: int = 0) -> np.ndarray:
        lab = _c(labels, np.int32)
        out = np.empty((n_perm + 1, n_types, n_types), dtype=np.int64)
        _check(self._lib.sc_enrichment_counts(self._h, _ptr(lab), lab.size, int(n_types), int(n_perm), int(perm_row0),
                                              _ptr(out)))
        return out


    def enrichment_counter(self, labels, n_types: int, seed: int, p_first: int, n_perm: int, batch: int = 512):
        """Observed T x T edge counts and the integer sums (deviation, squared deviation, exceedances) over the
        counter-based label permutations p_first .. p_first + n_perm - 1, generation overlapped with counting."""
        lab = _c(labels, np.int32)
        obs = np.empty((n_types, n_types), dtype=np.int64)
        sums = np.empty((3, n_types, n_types), dtype=np.int64)
        _check(self._lib.sc_enrichment_counter(self._h, _ptr(lab), lab.size, int(n_types), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                               int(p_first), int(n_perm), int(batch), _ptr(obs), _ptr(sums)))
        return obs, sums

    # ---- N6 (extension): Ripley's K ---------------------------------------------------------
    def ripley_build(self, coords, radii) -> int:
        """Builds the device-resident list of pairs within radii[-1], each tagged with the smallest radius that contains
        it; returns the number of ORDERED pairs (nnz of the radius graph at radii[-1]).  The active graph is untouched."""
        xy = _c(coords, np.float64)
        r = _c(radii, np.float64)
        n_pairs = c_int64(0)
        _check(self._lib.sc_ripley_build(self._h, _ptr(xy), xy.shape[0], _ptr(r), r.size, byref(n_pairs)))
        self._ripley_radii = int(r.size)
        return n_pairs.value

    def ripley_counts(self, labels, n_types: int, n_perm: int, perm_row0: int = 0) -> np.ndarray:
        """(n_perm + 1, T, T, R) cumulative ordered pair counts under rows [perm_row0, perm_row0 + n_perm) of the
        resident permutation table; the last slice is the observed table."""
        lab = _c(labels, np.int32)
        out = np.empty((n_perm + 1, n_types, n_types, self._ripley_radii), dtype=np.int64)
        _check(self._lib.sc_ripley_counts(self._h, _ptr(lab), lab.size, int(n_types), int(n_perm), int(perm_row0), _ptr(out)))
        return out

    def ripley_counter(self, labels, n_types: int, seed: int, p_first: int, n_perm: int, batch: int = 512):
        """Observed (T, T, R) table and the four integer sum rows (deviation, squared deviation, #{>=}, #{<=}) over the
        counter-based label permutations p_first .. p_first + n_perm - 1, generation overlapped with counting."""
        lab = _c(labels, np.int32)
        obs = np.empty((n_types, n_types, self._ripley_radii), dtype=np.int64)
        sums = np.empty((4, n_types, n_types, self._ripley_radii), dtype=np.int64)
        _check(self._lib.sc_ripley_counter(self._h, _ptr(lab), lab.size, int(n_types), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           int(p_first), int(n_perm), int(batch), _ptr(obs), _ptr(sums)))
        return obs, sums

    # ---- N11 (extension): Ripley's G --------------------------------------------------------
    def ripley_g_build(self, coords, radii) -> int:
        """Builds the device-resident ordered neighbour lists within radii[-1], one row per cell, each entry tagged with
        the smallest radius that contains the pair; returns the number of entries (ORDERED pairs: nnz of the radius graph
        at radii[-1], the value ``ripley_build`` returns).  The active graph and a Ripley pair list are untouched."""
        xy = _c(coords, np.float64)
        r = _c(radii, np.float64)
        n_entries = c_int64(0)
        _check(self._lib.sc_ripley_g_build(self._h, _ptr(xy), xy.shape[0], _ptr(r), r.size, byref(n_entries)))
        self._ripley_g_radii = int(r.size)
        return n_entries.value

    def ripley_g_counts(self, labels, n_types: int, n_perm: int, perm_row0: int = 0) -> np.ndarray:
        """(n_perm + 1, T, T, R) cumulative counts of cells of type a with a cell of type b within r_j, under rows
        [perm_row0, perm_row0 + n_perm) of the resident permutation table; the last slice is the observed table."""
        lab = _c(labels, np.int32)
        out = np.empty((n_perm + 1, n_types, n_types, self._ripley_g_radii), dtype=np.int64)
        _check(self._lib.sc_ripley_g_counts(self._h, _ptr(lab), lab.size, int(n_types), int(n_perm), int(perm_row0), _ptr(out)))
        return out

    def ripley_g_counter(self, labels, n_types: int, seed: int, p_first: int, n_perm: int, batch: int = 512):
        """Observed (T, T, R) table and the four integer sum rows (deviation, squared deviation, #{>=}, #{<=}) over the
        counter-based label permutations p_first .. p_first + n_perm - 1, generation overlapped with counting."""
        lab = _c(labels, np.int32)
        obs = np.empty((n_types, n_types, self._ripley_g_radii), dtype=np.int64)
        sums = np.empty((4, n_types, n_types, self._ripley_g_radii), dtype=np.int64)
        _check(self._lib.sc_ripley_g_counter(self._h, _ptr(lab), lab.size, int(n_types), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                             int(p_first), int(n_perm), int(batch), _ptr(obs), _ptr(sums)))
        return obs, sums

    # ---- N9 (extension): co-occurrence ------------------------------------------------------
    def cooccurrence_counts(self, coords_sorted, type_off, thresholds) -> np.ndarray:
        """(T, T, len(thresholds)) int64 ordered pair counts by type pair and distance bin over ALL pairs of cells
        (sc_cooccurrence_2d): the cells arrive sorted by type with offsets ``type_off`` (T + 1 entries); bin 0 holds the
        pairs within thresholds[0], bin j the annulus (thresholds[j - 1], thresholds[j]], pairs beyond the last threshold
        are dropped.  Leaves the bin grid, the active graph and a built Ripley pair list as they were."""
        xy = _c(coords_sorted, np.float64)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError(f"coordinates must have shape (n, 2), got {xy.shape}")
        off = _c(type_off, np.int64)
        t = _c(thresholds, np.float64)
        if off.ndim != 1 or off.size < 2 or t.ndim != 1:
            raise ValueError("type offsets and thresholds must be 1-D, with at least one type")
        if off[-1] != xy.shape[0]:
            raise ValueError("type offsets do not cover the point array")
        out = np.empty((off.size - 1, off.size - 1, t.size), dtype=np.int64)
        _check(self._lib.sc_cooccurrence_2d(self._h, _ptr(xy), _ptr(off), off.size - 1, _ptr(t), t.size, _ptr(out)))
        return out

    # ---- N10 (extension): ligand-receptor permutation test ----------------------------------
    def _ligrec_args(self, labels, n_types: int, shift, pair_l, pair_r):
        lab, sh = _c(labels, np.int32), _c(shift, np.int32)
        pl, pr = _c(pair_l, np.int32), _c(pair_r, np.int32)
        G = int(getattr(self, "_n_genes", 0))
        if lab.ndim != 1 or pl.ndim != 1 or pl.shape != pr.shape:
            raise ValueError("labels must be 1-D and the two ends of the interactions 1-D arrays of one length")
        if G and sh.shape != (G,):   # (without a loaded expression the library refuses the call: the arrays only have to exist)
            raise ValueError(f"one shift per loaded gene is required: {G} genes, shift has shape {sh.shape}")
        K, Gs = max(int(n_types), 1), max(G, 1)
        out = {"sum": np.zeros((K, Gs), dtype=np.int64), "nnz": np.zeros((K, Gs), dtype=np.int64),
               "group_n": np.zeros(K, dtype=np.int64), "count_ge": np.zeros((max(pl.size, 1), K, K), dtype=np.int64)}
        return lab, sh, pl, pr, out

    def ligrec_counts(self, labels, n_types: int, shift, pair_l, pair_r, n_perm: int, perm_row0: int = 0,
                      return_null_sums: bool = False) -> dict:
        """sc_ligrec_counts on the loaded genes: ``sum`` (K, G) int64 = the quantised expression ``rint(x * 2**shift[g])``
        summed per cluster, ``nnz`` (K, G) = cells with x > 0, ``group_n`` (K,), ``count_ge`` (I, K, K) = permutations (rows
        [perm_row0, perm_row0 + n_perm) of the resident table) whose ligand-in-a plus receptor-in-b mean is >= the observed
        one, decided exactly, and on request ``null_sums`` (n_perm, K, G), the sums under every row."""
        lab, sh, pl, pr, out = self._ligrec_args(labels, n_types, shift, pair_l, pair_r)
        nul = np.zeros((int(n_perm),) + out["sum"].shape, dtype=np.int64) if return_null_sums else None
        _check(self._lib.sc_ligrec_counts(self._h, _ptr(lab), lab.size, int(n_types), _ptr(sh), _ptr(pl), _ptr(pr), pl.size,
                                          int(n_perm), int(perm_row0), _ptr(out["sum"]), _ptr(out["nnz"]), _ptr(out["group_n"]),
                                          _ptr(nul), _ptr(out["count_ge"])))
        out["null_sums"] = nul
        return out

    def ligrec_counter(self, labels, n_types: int, shift, pair_l, pair_r, seed: int, p_first: int, n_perm: int,
                       batch: int = 512) -> dict:
        """ligrec_counts over the counter-based label permutations p_first .. p_first + n_perm - 1 (sc_ligrec_counter),
        generation overlapped with the sums; no ``null_sums``."""
        lab, sh, pl, pr, out = self._ligrec_args(labels, n_types, shift, pair_l, pair_r)
        _check(self._lib.sc_ligrec_counter(self._h, _ptr(lab), lab.size, int(n_types), _ptr(sh), _ptr(pl), _ptr(pr), pl.size,
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(p_first), int(n_perm), int(batch),
                                           _ptr(out["sum"]), _ptr(out["nnz"]), _ptr(out["group_n"]), _ptr(out["count_ge"])))
        return out


class RcclComm:
    """One rank's end of the RCCL communicator (include/spatialcore_hip.h, "multi-GPU")."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = np.zeros(RcclComm.ID_BYTES, dtype=np.uint8)
        _check(load_library().sc_comm_unique_id(_ptr(buf)))
        return buf.tobytes()

    def __init__(self, ctx: Context, unique_id: bytes, world: int, rank: int):
        if len(unique_id) != self.ID_BYTES:
            raise ValueError(f"an RCCL unique id is {self.ID_BYTES} bytes, got {len(unique_id)}")
        self._lib = load_library()
        self._ctx = ctx                     # keeps the context (stream, device) alive
        self.world, self.rank = int(world), int(rank)
        h = c_void_p()
        idb = np.frombuffer(unique_id, dtype=np.uint8).copy()
        _check(self._lib.sc_comm_create(ctx._h, _ptr(idb), self.world, self.rank, byref(h)))
        self._h = h

    def all_gather(self, block: np.ndarray) -> np.ndarray:
        """(world, *block.shape) float64: every rank's equally shaped block, in rank order."""
        mine = _c(block, np.float64)
        out = np.empty((self.world,) + mine.shape, dtype=np.float64)
        if mine.size:
            _check(self._lib.sc_allgather(self._h, _ptr(mine), mine.size, _ptr(out)))
        return out

    def max_over_ranks(self, values) -> np.ndarray:
        v = np.array(values, dtype=np.float64, ndmin=1)
        _check(self._lib.sc_allreduce_max(self._h, _ptr(v), v.size))
        return v

    def sum_over_ranks_i64(self, values) -> np.ndarray:
        """Element-wise integer sum over ranks (exact; used to merge exceedance counts of permutation shards)."""
        v = np.array(values, dtype=np.int64, ndmin=1)
        shape = v.shape
        v = np.ascontiguousarray(v.reshape(-1))
        if v.size:
            _check(self._lib.sc_allreduce_sum_i64(self._h, _ptr(v), v.size))
        return v.reshape(shape)

    def info(self) -> Tuple[int, int, int]:
        """(ranks, this rank, device) as RCCL itself reports them for this communicator."""
        w, r, d = c_int(0), c_int(0), c_int(0)
        _check(self._lib.sc_comm_info(self._h, byref(w), byref(r), byref(d)))
        return w.value, r.value, d.value

    def barrier(self) -> None:
        self.max_over_ranks([0.0])

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.sc_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def release_default_contexts() -> None:
    """Destroy the cached per-device contexts (their device memory and streams); the next default_context() creates anew.
    A process's streams share hardware queues once they outnumber GPU_MAX_HW_QUEUES, so a program that is done with the
    default context and goes on with contexts of its own (the test suite) gives it back."""
    for ctx in list(_default_ctx.values()):
        if ctx is not None and ctx._h is not None:
            ctx.close()
    _default_ctx.clear()


def default_context(device: int = 0) -> Context:
    """Process-wide context per device (created on first use; raises without a gfx950 GPU)."""
    ctx = _default_ctx.get(device)
    if ctx is None or ctx._h is None:
        ctx = Context(device)
        _default_ctx[device] = ctx
    return ctx
