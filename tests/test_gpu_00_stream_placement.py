"""The placement of a context's eleven streams on the runtime's hardware queues (spatialcore_amd/csrc/sc_streams.h,
permgen_place_streams): plain streams where GPU_MAX_HW_QUEUES holds them all, one group per stream priority level
where a launcher holds the process to 4 queues per level, the sequential scan where neither fits.

A process's hardware queues are fixed at its first HIP call and the suite's own process asks for 24, so every GPU case
starts a fresh child with its own environment and compares it with a child that leaves the variable to the library
(plain streams, 24).  Shapes are the smallest that reach the block-parallel form (n >= 131072).  The pure function behind
the choice is tested on the CPU for every limit from 1 to 32 by a stand-alone host program."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SPREAD = "streams spread over three priority levels"

_PRELUDE = r"""
import os, sys, time, logging, io
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
if os.environ.get("SC_TEST_HIP_FIRST") == "1":
    # a host application that touches the GPU before it imports the library: the runtime initialises with ITS default
    import ctypes
    hip = None
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            hip = ctypes.CDLL(name)
            break
        except OSError:
            pass
    assert hip is not None, "libamdhip64.so not found"
    assert hip.hipInit(0) == 0 and hip.hipFree(ctypes.c_void_p(0)) == 0
import spatialcore_amd
from spatialcore_amd import _lib
buf = io.StringIO()
logging.getLogger("spatialcore_amd").addHandler(logging.StreamHandler(buf))
"""

# init() + the public morans_i, as _INIT_WORKER of test_gpu_00_multirank.py, plus the generator's counters
_PUBLIC_WORKER = _PRELUDE + r"""
rep = spatialcore_amd.init()
print("REPORT", rep["hw_queues_requested"], int(rep["streams_concurrent"]), rep["generator"].replace("\n", " "), flush=True)
from conftest import make_adata, synth
from spatialcore_amd.spatial import morans_i
coords, X = synth(140001, 6, 3, dtype=np.float32)
ad = make_adata(coords, X)
morans_i(ad, n_neighbors=6, n_permutations=40, seed=2)
op = ad.uns["spatialcore_metadata"]["operations"][-1]
print("FORM", op["parameters"]["permgen_form"].replace("\n", " "), flush=True)
print("PVAL", " ".join(repr(float(v)) for v in ad.uns["morans_i"]["p_value"].values), flush=True)
print("WARNED", int("sequential scan" in buf.getvalue()), int("priority levels" in buf.getvalue()), flush=True)
print("STATS", *_lib.default_context(0).permgen_stats()[:3], flush=True)
"""

# moran_seeded through the whole pipeline: P = 400 > 3 x 128 (tail chunks, both swap streams, the two-permutation swap
# form, the finalise ring), n = 131072 + 37 -- the shape of the `big` fixture of test_gpu_moran_stream.py
_PIPELINE_WORKER = _PRELUDE + r"""
n, G, P, K = 131072 + 37, 130, 400, 6
rng = np.random.default_rng(4)
coords = rng.uniform(0, np.sqrt(n) * 10, (n, 2))
rng = np.random.default_rng(6)
X = np.minimum(rng.poisson(rng.uniform(0.2, 4.0, G), (n, G)), 15).astype(np.float32)
ctx = _lib.Context(0)
ctx.set_moran_source_bits(8)
ctx.knn(coords, K, fetch=False); ctx.graph_from_knn(1.0 / K)
ctx.set_expression(X, np.arange(G))
w = _lib.rng_state_words(np.random.default_rng(21))
out = ctx.moran_seeded(w, P)
wh = _lib.rng_state_words(np.random.default_rng(21))
_lib.perm_numpy_host(wh, n, P)
print("STATE", int(np.array_equal(w, wh)), flush=True)
print("FORM", ctx.permgen_form(n).replace("\n", " "), flush=True)
print("STATS", *ctx.permgen_stats()[:3], flush=True)
print("WARNED", int("sequential scan" in buf.getvalue()), int("priority levels" in buf.getvalue()), flush=True)
np.savez(sys.argv[1], I=out["I"], sims=out["sims"], count_ge=out["count_ge"])
ctx.close()
"""

_TWO_CONTEXT_WORKER = _PRELUDE + r"""
n, P = 140001, 6
want = _lib.perm_numpy_host(_lib.rng_state_words(np.random.default_rng(12)), n, P)
ctxs = [_lib.Context(0), _lib.Context(0)]
for i, c in enumerate(ctxs):
    t0 = time.perf_counter()
    got = c.generate_permutations(_lib.rng_state_words(np.random.default_rng(12)), n, P, fetch=True)
    wall = time.perf_counter() - t0
    print(f"CTX{{i}}", int(np.array_equal(got, want)), *c.permgen_stats()[:3], repr(wall), flush=True)
    print(f"FORM{{i}}", c.permgen_form(n).replace("\n", " "), flush=True)
    print(f"NOTE{{i}}", c.permgen_note().replace("\n", " "), flush=True)
for c in ctxs:
    c.close()
"""


def _run(tmp_path, text, name, queues, *args, hip_first=False):
    """One fresh child: GPU_MAX_HW_QUEUES exported as `queues`, or left to the library (None)."""
    script = tmp_path / f"{name}.py"
    script.write_text(text.format(root=ROOT))
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "SC_TEST_HIP_FIRST")}
    if queues is not None:
        env["GPU_MAX_HW_QUEUES"] = str(queues)
    if hip_first:
        env["SC_TEST_HIP_FIRST"] = "1"
    run = subprocess.run([sys.executable, str(script), *map(str, args)], env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    print(run.stdout)
    return {ln.split()[0]: ln.split(None, 1)[1] if len(ln.split(None, 1)) > 1 else "" for ln in run.stdout.splitlines() if ln.split()}


@pytest.fixture(scope="module")
def plain_public(tmp_path_factory):
    """The public call in a child that leaves the variable to the library: plain streams, 24 queues."""
    out = _run(tmp_path_factory.mktemp("plain_public"), _PUBLIC_WORKER, "public", None)
    q, ok, gen = out["REPORT"].split(None, 2)
    assert int(q) == 24 and int(ok) == 1 and gen == "block-parallel" and out["FORM"] == "block-parallel", out
    return out


@pytest.fixture(scope="module")
def plain_pipeline(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain_pipeline")
    out = _run(d, _PIPELINE_WORKER, "pipeline", None, d / "plain.npz")
    assert out["FORM"] == "block-parallel" and out["STATS"].split() == ["1", "0", "0"] and out["STATE"] == "1", out
    return dict(np.load(d / "plain.npz"))


@pytest.mark.gpu
def test_exported_4_public_call_is_block_parallel_on_spread_streams(tmp_path, plain_public):
    out = _run(tmp_path, _PUBLIC_WORKER, "public", 4)
    q, ok, gen = out["REPORT"].split(None, 2)
    assert int(q) == 4 and int(ok) == 1, out                              # 4 requested, streams concurrent
    assert gen == f"block-parallel; {SPREAD} (GPU_MAX_HW_QUEUES=4)", out
    assert out["FORM"] == gen, out
    assert out["WARNED"] == "0 0", out                                    # no "sequential scan" warning, and the placement is not logged as one
    assert out["STATS"].split() == ["1", "0", "0"], out
    assert out["PVAL"] == plain_public["PVAL"]


@pytest.mark.gpu
def test_exported_4_whole_pipeline_equals_plain_byte_for_byte(tmp_path, plain_pipeline):
    out = _run(tmp_path, _PIPELINE_WORKER, "pipeline", 4, tmp_path / "spread.npz")
    assert out["FORM"].startswith("block-parallel") and SPREAD in out["FORM"], out
    assert out["STATS"].split() == ["1", "0", "0"], out                   # one block-parallel job, 0 fallbacks
    assert out["STATE"] == "1" and out["WARNED"] == "0 0", out            # the generator's final state is perm_numpy_host's
    got = np.load(tmp_path / "spread.npz")
    for key in ("I", "sims", "count_ge"):
        assert got[key].dtype == plain_pipeline[key].dtype and got[key].shape == plain_pipeline[key].shape, key
        assert got[key].tobytes() == plain_pipeline[key].tobytes(), key


@pytest.mark.gpu
def test_hip_initialised_before_the_library_is_loaded(tmp_path, plain_public):
    """The runtime initialised with its own default before the library could ask for 24: the environment shows 24, the
    plain probe finds shared queues, the spread placement takes over.  (A runtime that honours the late request passes
    the plain probe: exactly "block-parallel".)  Which of the two happened is printed; when the test was written
    the runtime did not honour the late request: the spread placement, reported with GPU_MAX_HW_QUEUES=24."""
    out = _run(tmp_path, _PUBLIC_WORKER, "public", None, hip_first=True)
    q, ok, gen = out["REPORT"].split(None, 2)
    print("HIP first:", out["REPORT"])
    assert int(ok) == 1, out
    assert gen == "block-parallel" or (gen.startswith("block-parallel; ") and SPREAD in gen), out
    assert out["FORM"] == gen and out["WARNED"] == "0 0", out
    assert out["STATS"].split() == ["1", "0", "0"], out
    assert out["PVAL"] == plain_public["PVAL"]


@pytest.mark.gpu
def test_exported_4_two_live_contexts(tmp_path):
    """The spread placement fills its queue pools exactly, so a second live context cannot have queues of its own: its
    all-role probe must notice (no repeated 1-second give-ups inside jobs) and say which form it took."""
    out = _run(tmp_path, _TWO_CONTEXT_WORKER, "two", 4)
    for i in (0, 1):
        same, par, seq, fallbacks, wall = out[f"CTX{i}"].split()
        assert same == "1", out                                           # both tables are perm_numpy_host's
        assert float(wall) < 6.0, out
        form = out[f"FORM{i}"]
        if i == 0:
            assert form.startswith("block-parallel") and (par, seq, fallbacks) == ("1", "0", "0"), out
        elif form.startswith("block-parallel"):
            assert (par, seq, fallbacks) == ("1", "0", "0"), out
        else:
            assert form.startswith("sequential: ") and out[f"NOTE{i}"] and (par, seq) == ("0", "1"), out


@pytest.mark.gpu
def test_exported_3_takes_the_sequential_scan_with_the_note(tmp_path, plain_public):
    """Nine queues cannot hold eleven streams: today's behaviour."""
    out = _run(tmp_path, _PUBLIC_WORKER, "public", 3)
    q, ok, gen = out["REPORT"].split(None, 2)
    if int(ok) == 1:
        pytest.skip("the runtime ran the streams concurrently on three hardware queues: nothing to fall back from")
    assert int(q) == 3 and gen.startswith("sequential: ") and "GPU_MAX_HW_QUEUES=3" in gen and "sequential scan" in gen, out
    assert out["FORM"].startswith("sequential: ") and out["WARNED"] == "1 0", out
    assert out["STATS"].split() == ["0", "1", "0"], out
    assert out["PVAL"] == plain_public["PVAL"]


def test_placement_function_for_limits_1_to_32(tmp_path):
    """sc_place_streams on the CPU (tests/stream_placement_checks.cpp: its own main, no HIP): plain from 11 up, spread
    from 4 to 10 and after a failed plain probe, "does not fit" below 4, the tables it must refuse."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path / "stream_placement_checks"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-x", "c++", os.path.join(ROOT, "tests", "stream_placement_checks.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=120)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "stream placement: ok" in run.stdout, run.stdout[-3000:]
