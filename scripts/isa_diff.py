"""Compare the gfx950 device code of two source trees kernel by kernel (no GPU needed).

    python scripts/isa_diff.py OLD_CSRC [NEW_CSRC] [--keep DIR] [--rename OLD_SYMBOL=NEW_SYMBOL ...]

Every *.hip of both directories (NEW_CSRC defaults to spatialcore_amd/csrc; OLD_CSRC is e.g. the csrc/ of a
`git worktree add` of the parent commit) is compiled to device assembly with the Makefile's code-generation flags,
the assembly is cut per kernel symbol -- code, .amdhsa_kernel block and resource summary -- and the kernels are
matched BY NAME across all units, so a kernel that moved to another file compares equal.  Reported: kernels that
are missing, new or defined twice, and for every kernel whose text differs its resources, old -> new.
--rename (repeatable) compares kernel OLD_SYMBOL of the old tree with kernel NEW_SYMBOL of the new one, the symbols as
this tool prints them, with the symbol's own name replaced in both texts; between such a pair the section directive that
differs only because a plain function became a template instantiation (.text vs its comdat .section) does not count.
Exit status 0 only if both trees hold the same kernels with identical text.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-device-only", "-S",
         "-Wno-unused-command-line-argument"]
BEGIN = re.compile(r"; -- Begin function (\S+)")
LOCAL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp|LJTI)\d+")   # labels numbered by position in the unit
SECTION = re.compile(r'(?m)^\t(\.text|\.section\t\.text\.\S+,"axG",@progbits,\S+,comdat)$')
FIELDS = (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size",
          ".amdhsa_private_segment_fixed_size", "; Occupancy:", "; codeLenInByte")


def kernels(src_dir, out_dir):
    """{kernel symbol: [normalised text, ...]} over every unit of src_dir"""
    units = sorted(glob.glob(os.path.join(src_dir, "*.hip")))
    os.makedirs(out_dir, exist_ok=True)

    def compile_unit(u):
        s = os.path.join(out_dir, os.path.basename(u)[:-4] + ".s")
        subprocess.check_call([HIPCC, *FLAGS, u, "-o", s])
        return s

    found = {}
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for s in pool.map(compile_unit, units):
            text = open(s).read().split("\t.amdgpu_metadata")[0]
            blocks = re.split(r"(?m)^(?=.*; -- Begin function )", text)
            for b in blocks[1:]:
                name = BEGIN.search(b).group(1)
                if ".amdhsa_kernel " + name not in b:   # (a device function that was not inlined is not a kernel)
                    continue
                # ends with the resource comments of its .AMDGPU.csdata section; what follows belongs to the next symbol
                head, _, tail = b.partition("\t.section\t.AMDGPU.csdata")
                stats = [ln for ln in tail.split("\n")[1:] if ln.startswith(";")]
                code = re.sub(r"(?m)[ \t]*;.*$", "", LOCAL.sub(r".\1", head))   # (comments name blocks by their number in the unit)
                found.setdefault(name, []).append(code + "\n".join(stats))
    return found


def resources(block):
    out = []
    for f in FIELDS:
        m = re.search(re.escape(f) + r"\s*=?\s*(\S+)", block)
        out.append("%s %s" % (f.lstrip(".; ").replace("amdhsa_", "").rstrip(":"), m.group(1) if m else "?"))
    out.append("instructions %d" % len(re.findall(r"(?m)^\t[a-z]\w+_\w+", block)))
    return ", ".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new", nargs="?", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spatialcore_amd", "csrc"))
    ap.add_argument("--keep", help="keep the assembly under this directory")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD_SYMBOL=NEW_SYMBOL",
                    help="compare this kernel of the old tree with that kernel of the new one")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    old, new = kernels(a.old, os.path.join(tmp, "old")), kernels(a.new, os.path.join(tmp, "new"))
    bad = 0
    renamed = [r.split("=", 1) for r in a.rename]
    for o_name, n_name in renamed:
        o, n = old.get(o_name, []), new.get(n_name, [])
        if len(o) != 1 or len(set(n)) != 1:   # (several equal copies after: kernels merged into a header library's one)
            print("COUNT   %s -> %s: %d definition(s) before, %d after" % (o_name, n_name, len(o), len(n)))
            bad += 1
            continue
        o_text, n_text = (SECTION.sub("\t.text", t.replace(name, "KERNEL")) for t, name in ((o[0], o_name), (n[0], n_name)))
        if o_text != n_text:
            print("DIFFERS %s -> %s\n    old: %s\n    new: %s" % (o_name, n_name, resources(o[0]), resources(n[0])))
            bad += 1
    for o_name, n_name in renamed:
        old.pop(o_name, None)
        new.pop(n_name, None)
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name, []), new.get(name, [])
        if len(o) != len(n) or len(set(n)) != 1:   # (several equal copies: a header library's kernel in more than one unit)
            print("COUNT   %s: %d definition(s) before, %d after" % (name, len(o), len(n)))
            bad += 1
        elif o[0] != n[0]:
            print("DIFFERS %s\n    old: %s\n    new: %s" % (name, resources(o[0]), resources(n[0])))
            bad += 1
    print("%d kernels before, %d after, %d not identical" % (len(old), len(new), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
