#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_kfdb_query and of the adapter's whole DetectRelocalizationCandidates
(pli_slam_amd/adapters/orbslam_keyframe_database.hpp) against a plain host inverted-file implementation of our own on the same box,
for databases of 100, 1000 and 10000 keyframes of about 1000 words.  Builds tools/kfdb_query_timing.cpp against the product library
into a temporary directory and runs it once per size; the program fails if the two paths disagree on a candidate list.
Prints ONE JSON line: medians over --calls queries after --warmup.

  python tools/kfdb_query_timing.py [--n 100,1000,10000] [--calls 30] [--warmup 5]

(A kernel trace, if wanted, in a run of its own: rocprofv3 --kernel-trace --stats -- <the built program> 10000.)
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="100,1000,10000")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    out = {"tool": "kfdb_query_timing", "runs": []}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "kfdb_query_timing")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I", ROOT, os.path.join(ROOT, "tools", "kfdb_query_timing.cpp"), LIB,
                               "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        for n in a.n.split(","):
            r = subprocess.run([exe, n, str(a.calls), str(a.warmup)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("kfdb_query_timing %s: exit %d: %s" % (n, r.returncode, r.stderr[-2000:]))
            out["runs"].append(json.loads(r.stdout))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
