#!/usr/bin/env python3
"""GPU box: latency of the front-end of ONE single-camera Frame (752x480, default config, frames cut from the photographs), monocular
and RGB-D — pli_frame_extract_single against the sequence of per-call entry points that served such a Frame before it:
orb_extract_lapping + line_extract (+ stereo_from_depth), each of which stages, synchronises and reads back on its own.  Both in
the same process, on contexts of their own, alternating frame by frame; wall clock around calls that end in a synchronise.

  python tools/single_camera_frame.py [frames] [rounds] [json out]

Per mode and form: the median over frames of each frame's median over rounds, and the spread (the 10th and 90th percentile of the
per-call times).  Written as JSON (default profiles/single_frame_timing.json) and printed."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pli_slam_amd import capi, realdata
from pli_slam_amd.frontend import Frontend

nframes = int(sys.argv[1]) if len(sys.argv) > 1 else 12
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "single_frame_timing.json")
W, H = 752, 480
TUM = (517.306408 * W / 640, 516.469215, 318.643040 * W / 640, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
frames = [np.ascontiguousarray(f[0]) for f in realdata.frames_752x480(nframes, seed=17)]
ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
depth = (1.5 + 0.004 * xs + 0.002 * ys).astype(np.float32)
cfg = capi.default_config(W, H)
one, seq = Frontend(cfg, dev=False), Frontend(cfg, dev=False)
one.set_pinhole_distortion(TUM)


def fused(img, mode):
    return one.frame_extract_single(img, (0, 1000) if mode == "mono" else (0, 0), None if mode == "mono" else depth)


def sequence(img, mode):
    r = seq.orb_extract_lapping(0, img, (0, 1000) if mode == "mono" else (0, 0))
    l = seq.line_extract(0, img)
    d = seq.stereo_from_depth(depth) if mode == "rgbd" else None
    return r, l, d


def clock(fn, img, mode):
    t0 = time.perf_counter()
    fn(img, mode)                       # (every entry point returns behind its own stream synchronise)
    return (time.perf_counter() - t0) * 1e3


result = {"width": W, "height": H, "frames": nframes, "rounds": rounds, "config": "pli_config_default(752, 480)",
          "clock": "host wall clock around each call (the calls end in a stream synchronise); Python wrapper included in both forms"}
for mode in ("mono", "rgbd"):
    for img in frames[:2]:              # warm-up: code objects, scratch, pinned buffers, the LSD's round plan
        for _ in range(3):
            fused(img, mode); sequence(img, mode)
    # the same answer first
    a, (b, l, d) = fused(frames[0], mode), sequence(frames[0], mode)
    assert a["kpL"].tobytes() == b[2].tobytes() and a["klL"].tobytes() == l[1].tobytes(), "the two forms differ"
    t = {"fused": np.zeros((nframes, rounds)), "sequence": np.zeros((nframes, rounds))}
    for r in range(rounds):
        for i, img in enumerate(frames):
            order = (("fused", fused), ("sequence", sequence)) if (r + i) % 2 == 0 else (("sequence", sequence), ("fused", fused))
            for name, fn in order:
                t[name][i, r] = clock(fn, img, mode)
    res = {}
    for name, v in t.items():
        res[name] = {"median_ms": float(np.median(np.median(v, axis=1))), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)),
                     "per_frame_median_ms": [round(float(x), 3) for x in np.median(v, axis=1)]}
    ratio = np.median(t["sequence"], axis=1) / np.median(t["fused"], axis=1)
    res["sequence_over_fused"] = {"median": float(np.median(ratio)), "min": float(ratio.min()), "max": float(ratio.max())}
    result[mode] = res
    print("%s: frame_extract_single %.3f ms (p10 %.3f, p90 %.3f)  |  separate calls %.3f ms (p10 %.3f, p90 %.3f)  |  ratio %.2f (%.2f .. %.2f)" % (
        mode, res["fused"]["median_ms"], res["fused"]["p10_ms"], res["fused"]["p90_ms"], res["sequence"]["median_ms"], res["sequence"]["p10_ms"],
        res["sequence"]["p90_ms"], res["sequence_over_fused"]["median"], res["sequence_over_fused"]["min"], res["sequence_over_fused"]["max"]), flush=True)
# where the fused call's time goes (HIP events on the context's stream; a run of its own, after the timed ones)
one.prof_enable(True); one.prof_reset()
for img in frames[:4]:
    fused(img, "rgbd")
rep = one.prof_report()
result["fused_kernel_ms_per_frame"] = {k: round(v[1] / 4, 4) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1])[:12]}
print("kernels of the fused call, ms per frame:", result["fused_kernel_ms_per_frame"], flush=True)
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out)
