"""The device generator alone (no scoring): time of sc_perm_generate at bench size, and its block statistics."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from spatialcore_amd import _lib
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
P = int(sys.argv[2]) if len(sys.argv) > 2 else 300
if os.environ.get("SC_LIB"):   # another build of the library
    _lib.LIB_PATH = os.environ["SC_LIB"]
ctx = _lib.Context(0)
for rep in range(3):
    w = _lib.rng_state_words(np.random.default_rng(0))
    ctx.sync(); t0 = time.perf_counter()
    ctx.generate_permutations(w, N, P)
    ctx.sync(); dt = time.perf_counter() - t0
    print(f"{P} x {N}: {dt * 1e3:.1f} ms, stats {ctx.permgen_stats()}, state {w[:2]}", flush=True)
st = ctx.debug_copy(5, 0, 8, np.uint64)
print(f"last job: {int(st[4])} blocks by lookup in {int(st[6])} segment lookups, {int(st[7]) & 0xffffffff} segments block by block (window missed); {int(st[5])} computed")
