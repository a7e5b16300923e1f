#!/usr/bin/env python3
"""Is the device code of two source trees the same, function by function?  Needs no GPU.

    python tools/device_code_diff.py PARENT_TREE [THIS_TREE] [--jobs N]

Every HIP source of the build is compiled in both trees with the build's own flags plus `--cuda-device-only -S`.  Per
function symbol the lines between `name:` and `.Lfunc_endN:` are taken, comments after `;` stripped, directive lines
(starting with `.`) dropped and the labels `.LBBn_m` rewritten to `.LBB_m`; what is left is hashed.  Every symbol of the
parent must exist with the same hash and none may be added.  Prints one line per file and exits 1 on any difference.
(A parent tree: `git archive REV | tar -x -C DIR`.)"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from __graft_entry__ import HIP_FLAGS, HIP_SOURCES  # noqa: E402

LABEL = re.compile(r"\.LBB\d+_(\d+)")


def functions(asm):
    out, name, body = {}, None, []
    for line in asm.splitlines():
        line = line.split(";", 1)[0].strip()
        if name is None:
            m = re.match(r"^([A-Za-z_$][\w$.]*):$", line)
            if m and not line.startswith("."):
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = hashlib.sha256("\n".join(body).encode()).hexdigest()
            name = None
        elif line and (not line.startswith(".") or line.startswith(".LBB")):
            body.append(LABEL.sub(r".LBB_\1", line))
    return out


def compile_one(tree, src, tmp):
    out = os.path.join(tmp, "%s_%s.s" % (hashlib.sha1(tree.encode()).hexdigest()[:8], src))
    csrc = os.path.join(tree, "pysparse_amd", "csrc")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + HIP_FLAGS +
                          ["-I" + os.path.join(tree, "include"), "-I" + csrc, "--cuda-device-only", "-S", "-Wno-unused-command-line-argument",
                           os.path.join(csrc, src), "-o", out])
    with open(out) as f:
        return functions(f.read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this", nargs="?", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        jobs = {(t, s): pool.submit(compile_one, os.path.abspath(t), s, tmp) for s in HIP_SOURCES for t in (a.parent, a.this)}
        for s in HIP_SOURCES:
            p, c = jobs[(a.parent, s)].result(), jobs[(a.this, s)].result()
            changed = sorted(k for k in p if k in c and p[k] != c[k])
            missing, added = sorted(set(p) - set(c)), sorted(set(c) - set(p))
            print("%-18s %4d device functions: %d changed, %d missing, %d added" % (s, len(p), len(changed), len(missing), len(added)))
            for k in changed + missing + added:
                print("    " + k)
            bad += len(changed) + len(missing) + len(added)
    print("device code identical in every translation unit" if not bad else "%d device functions differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
