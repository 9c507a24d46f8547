"""Development: run bench.py against another build of the library, e.g. one built from another commit (A/B on the
same box in the same call).  usage: python scripts/bench_variant.py path/to/libspatialcore_hip.so [bench.py flags]"""
import sys, runpy
sys.path.insert(0, ".")
from spatialcore_amd import _lib
_lib.LIB_PATH = sys.argv[1]
sys.argv = ["bench.py"] + sys.argv[2:]
runpy.run_path("bench.py", run_name="__main__")
