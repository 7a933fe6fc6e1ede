#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_distinctive_descriptors (MapPoint / MapLine::ComputeDistinctiveDescriptors for a batch of
features in one call) on three shapes of synthetic tracks (tests/helpers_distinctive.py: track, flip rate 0.15):

  local_mapping   1000 groups of 3-15 rows    (LocalMapping.cc:267-286: the map points of a new keyframe)
  long_session    1000 groups of 20-80 rows   (long tracks)
  cap             one group of 2048 rows      (PLI_DISTINCTIVE_MAX_OBS)

The C entry is timed on packed tables (upload, launches, download and synchronisation included; the packing is the caller's): the
median of --calls calls per series, --series series, the shapes interleaved within a series; reported is the median of the series'
medians with the smallest and the largest.  The kernels alone come from the library's event timer (pli_prof_enable) over a further
--calls calls.  Next to it stands a plain single-threaded host loop of the same semantics over the same tables
(tests/cpp/distinctive_harness.cpp --time, built here with g++ -O2): NOT the reference's loop (no cv::Mat, no float matrix, no
mutex), so no speed-up over the reference follows from the two numbers.  A sweep over group sizes (1000 groups of n rows each)
names the size from which the batch call is the faster of the two.  Prints ONE JSON line (and writes it to --out).

  python tools/distinctive_timing.py [--calls 50] [--series 5] [--warmup 10] [--out profiles/distinctive_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers_distinctive as H  # noqa: E402
from pli_slam_amd import capi  # noqa: E402
from pli_slam_amd.capi import ptr  # noqa: E402
from pli_slam_amd.frontend import Frontend, pack_keyframes  # noqa: E402

LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")
KERNELS = ("k_distinctive_wave", "k_distinctive_block", "k_distinctive_pick")


def build_harness(outdir):
    exe = os.path.join(outdir, "distinctive_harness")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"),
                    os.path.join(ROOT, "tests", "cpp", "distinctive_harness.cpp"), LIB, "-Wl,-rpath," + os.path.dirname(LIB),
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--series", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sweep", default="3,4,6,8,12,16,24,32,48,64")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    shapes = {
        "local_mapping": [H.track(rng, int(rng.integers(3, 16)), 0.15) for _ in range(1000)],
        "long_session": [H.track(rng, int(rng.integers(20, 81)), 0.15) for _ in range(1000)],
        "cap": [H.track(rng, capi.DISTINCTIVE_MAX_OBS, 0.15)],
    }
    sweep = [int(n) for n in a.sweep.split(",") if n]
    for n in sweep:
        shapes["sweep_%d" % n] = [H.track(rng, n, 0.15) for _ in range(1000)]
    fe = Frontend(capi.default_config(128, 96, orb_nfeatures=100, lsd_nfeatures=0), dev=False)
    packed = {}
    for name, groups in shapes.items():
        off, (desc,) = pack_keyframes([(g,) for g in groups], ((0, np.uint8, (32,)),), "a group is (N, 32) uint8")
        packed[name] = (desc, off, np.zeros(len(groups), np.int32), np.zeros(len(groups), np.int32))

    def call(name):
        desc, off, best, bm = packed[name]
        capi.check(fe.L.pli_distinctive_descriptors(fe.h, ptr(desc), ptr(off), len(best), ptr(best), ptr(bm), None))

    for name in packed:
        for _ in range(a.warmup):
            call(name)
    per_series = {name: [] for name in packed}
    for _ in range(a.series):
        ts = {name: [] for name in packed}
        for _ in range(a.calls):
            for name in packed:                                    # interleaved: a drift of the machine touches every shape alike
                t0 = time.perf_counter()
                call(name)
                ts[name].append((time.perf_counter() - t0) * 1e3)
        for name in packed:
            per_series[name].append(float(np.median(ts[name])))
    out = {"tool": "distinctive_timing", "calls": a.calls, "series": a.series, "shapes": {}}
    fe.prof_enable(True)
    tmp = tempfile.mkdtemp()
    exe = build_harness(tmp)
    for name, (desc, off, best, bm) in packed.items():
        fe.prof_reset()
        for _ in range(a.calls):
            call(name)
        rep = fe.prof_report()
        kernel_ms = sum(rep[k][1] for k in KERNELS if k in rep) / a.calls
        path = os.path.join(tmp, name + ".bin")
        with open(path, "wb") as f:
            f.write(np.int32(len(best)).tobytes() + off.tobytes() + desc.tobytes())
        host_calls = a.calls if off[-1] < 100000 and name != "cap" else 5          # (the cap's host loop takes tenths of a second)
        r = subprocess.run([exe, "--time", path, str(host_calls), str(a.series)], capture_output=True, text=True, check=True)
        host = json.loads(r.stdout)
        want = int(sum(int(b) + 4096 * int(m) for b, m in zip(best, bm)))
        assert host["checksum"] == want, (name, host["checksum"], want)           # the two computed the same winners
        s = sorted(per_series[name])
        out["shapes"][name] = {
            "groups": len(best), "rows": int(off[-1]),
            "batch_call_median_ms": round(s[len(s) // 2], 4), "batch_call_series_min_ms": round(s[0], 4),
            "batch_call_series_max_ms": round(s[-1], 4), "kernels_ms": round(kernel_ms, 4),
            "host_loop_median_ms": host["host_loop_median_ms"], "host_loop_series_min_ms": host["host_loop_min_series_ms"],
            "host_loop_series_max_ms": host["host_loop_max_series_ms"], "host_loop_calls_per_series": host_calls,
        }
    wins = [n for n in sweep
            if out["shapes"]["sweep_%d" % n]["batch_call_series_max_ms"] < out["shapes"]["sweep_%d" % n]["host_loop_series_min_ms"]]
    # the smallest size from which every larger size of the sweep wins too, series ranges apart
    from_n = None
    for n in reversed(sweep):
        if n in wins:
            from_n = n
        else:
            break
    out["batch_wins_from_rows_per_group"] = from_n
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    fe.close()


if __name__ == "__main__":
    main()
