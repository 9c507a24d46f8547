"""csrc/sc_search.h on the host: the two walks over the bin grid visit exactly the positions, in exactly the order, of
the loops the search kernels used to write out themselves (tests/search_walks_restated.cpp).  No GPU: the helpers are
plain C++ once __device__ is empty, so the host compiler builds them with the rounding of the device build
(-ffp-contract=off)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walks_match_written_out_loops(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    # any host C++ compiler; the one hipcc drives is there wherever the library itself can be built
    cxx = shutil.which(os.environ.get("CXX", "g++")) or os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    exe = str(tmp_path / "search_walks")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "spatialcore_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "search_walks_restated.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.startswith("walks ok"), out.stdout
