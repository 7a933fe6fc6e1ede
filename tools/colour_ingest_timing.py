#!/usr/bin/env python3
"""GPU box: what the colour / raw-depth ingest costs or saves on ONE RGB-D Frame of TUM's kind (640x480, TUM's Freiburg-1 camera,
3-channel colour, 16-bit depth with factor 5000, pli_config_default), 200 Frames cut from the photographs.

  (a) pli_frame_extract_single on the colour image and the raw uint16 map (pli_set_image_format RGB8, pli_set_depth_format U16)
  (b) the path before it: the host converts (tools/colour_ingest_host.cpp, plain C++ loops, g++ -O2: RGB -> gray, uint16 -> float x
      scale over the frame), then the same call on the gray image and the float map; conversion and call timed separately
  (c) the gray / float call alone, on inputs converted beforehand

  python tools/colour_ingest_timing.py [distinct frames] [rounds] [json out]

(a), (b), (c) alternate frame by frame in one process; (a) has a context of its own, (b) and (c) share a default one.  Host wall clock
around calls that end in a stream synchronise, the Python wrapper included in all three.  Per leg the median and the 10th / 90th
percentile over all frames x rounds calls; written as JSON (default profiles/colour_ingest_timing.json) and printed."""
import ctypes as C
import json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from pli_slam_amd import capi, realdata
from pli_slam_amd.frontend import Frontend

nframes = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 10
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "colour_ingest_timing.json")
W, H = 640, 480
TUM = (517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
SCALE = np.float32(1) / np.float32(5000)

tmp = tempfile.mkdtemp(prefix="pli_colour_host_")
so = os.path.join(tmp, "libcolour_ingest_host.so")
subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tools", "colour_ingest_host.cpp"), "-o", so])
host = C.CDLL(so)
host.pli_host_rgb_to_gray.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]
host.pli_host_depth_to_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
host.pli_host_rgb_to_gray.restype = host.pli_host_depth_to_f32.restype = None

# colour frames: red the photograph, green the same a pixel down and two across, blue the next photograph's cut, noise on each
rng = np.random.default_rng(23)
cuts = [np.ascontiguousarray(f[0]) for f in realdata.frames_752x480(nframes + 1, seed=17, w=W + 2, h=H + 1)]
colour = []
for i in range(nframes):
    planes = [cuts[i][:H, :W], cuts[i][1:, 2:], cuts[i + 1][:H, :W]]
    colour.append(np.stack([np.clip(p.astype(np.int32) + rng.integers(-4, 5, (H, W)), 0, 255).astype(np.uint8) for p in planes], axis=2))
ys, xs = np.mgrid[0:H, 0:W]
raw_depth = np.clip(5000 * (1.5 + 0.004 * xs + 0.002 * ys), 0, 65535).astype(np.uint16)      # 1.5 .. 5 m, as TUM stores it
raw_depth[200:230] = 0                                                                       # (no measurement)

cfg = capi.default_config(W, H)
fa, fb = Frontend(cfg, dev=False), Frontend(cfg, dev=False)
for fe in (fa, fb):
    fe.set_pinhole_distortion(TUM)
fa.set_image_format(capi.IMAGE_RGB8)
fa.set_depth_format(capi.DEPTH_U16, SCALE)
gray_buf, depth_buf = np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32)


def convert(img):
    host.pli_host_rgb_to_gray(capi.ptr(img), img.strides[0], W, H, 3, capi.ptr(gray_buf))
    host.pli_host_depth_to_f32(capi.ptr(raw_depth), W, H, float(SCALE), capi.ptr(depth_buf))


def leg_a(img):
    t0 = time.perf_counter()
    r = fa.frame_extract_single(img, (0, 0), raw_depth)
    return r, ((time.perf_counter() - t0) * 1e3,)


def leg_b(img):
    t0 = time.perf_counter()
    convert(img)
    t1 = time.perf_counter()
    r = fb.frame_extract_single(gray_buf, (0, 0), depth_buf)
    t2 = time.perf_counter()
    return r, ((t1 - t0) * 1e3, (t2 - t1) * 1e3)


pre = []
for img in colour:
    convert(img)
    pre.append((gray_buf.copy(), depth_buf.copy()))


def leg_c(i):
    t0 = time.perf_counter()
    r = fb.frame_extract_single(pre[i][0], (0, 0), pre[i][1])
    return r, ((time.perf_counter() - t0) * 1e3,)


for i in range(2):                       # warm-up: code objects, scratch, pinned buffers, the LSD's round plan
    for _ in range(3):
        leg_a(colour[i]); leg_b(colour[i]); leg_c(i)
# the same answer first
ra, rb, rc = leg_a(colour[0])[0], leg_b(colour[0])[0], leg_c(0)[0]
for k in ("record", "kp_un", "kl_un", "cell"):
    assert ra["full"][k].tobytes() == rb["full"][k].tobytes() == rc["full"][k].tobytes(), "the legs differ in " + k
assert len(ra["kpL"]) > 500 and (ra["depth"] > 0).sum() > 300

t = {"a": [], "b_convert": [], "b_call": [], "c": []}
for r in range(rounds):
    for i, img in enumerate(colour):
        for leg in ("abc", "bca", "cab")[(r + i) % 3]:
            if leg == "a":
                t["a"].append(leg_a(img)[1][0])
            elif leg == "b":
                conv, call = leg_b(img)[1]
                t["b_convert"].append(conv); t["b_call"].append(call)
            else:
                t["c"].append(leg_c(i)[1][0])
v = {k: np.array(x) for k, x in t.items()}
v["b_total"] = v["b_convert"] + v["b_call"]
stat = lambda x: {"median_ms": round(float(np.median(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4), "p90_ms": round(float(np.percentile(x, 90)), 4)}
result = {"width": W, "height": H, "frames": nframes * rounds, "distinct_frames": nframes, "config": "pli_config_default(640, 480), TUM Freiburg-1 camera",
          "clock": "host wall clock around each call (the calls end in a stream synchronise); Python wrapper included in every leg",
          "upload_bytes_per_frame": {"a_rgb8_u16": W * H * 3 + W * H * 2, "b_c_gray8_f32": W * H + W * H * 4},
          "a_frame_extract_single_rgb8_u16": stat(v["a"]),
          "b_host_conversion": stat(v["b_convert"]), "b_gray_f32_call": stat(v["b_call"]), "b_total": stat(v["b_total"]),
          "c_gray_f32_call_alone": stat(v["c"]),
          "a_minus_b_total_median_ms": round(float(np.median(v["a"]) - np.median(v["b_total"])), 4),
          "a_minus_c_median_ms": round(float(np.median(v["a"]) - np.median(v["c"])), 4)}
for k in ("a_frame_extract_single_rgb8_u16", "b_host_conversion", "b_gray_f32_call", "b_total", "c_gray_f32_call_alone"):
    print("%-34s median %.3f ms  p10 %.3f  p90 %.3f" % (k, result[k]["median_ms"], result[k]["p10_ms"], result[k]["p90_ms"]), flush=True)
print("a - b_total %.3f ms, a - c %.3f ms (medians)" % (result["a_minus_b_total_median_ms"], result["a_minus_c_median_ms"]), flush=True)
# the ingest kernel itself (HIP events on the context's stream; a run of its own, after the timed ones)
for name, fe, fn in (("a", fa, lambda i: leg_a(colour[i])), ("c", fb, leg_c)):
    fe.prof_enable(True); fe.prof_reset()
    for i in range(4):
        fn(i)
    rep = fe.prof_report()
    result["k_ingest_ms_per_frame_" + name] = round(rep["k_ingest"][1] / 4, 5) if "k_ingest" in rep else None
    fe.prof_enable(False)
print("k_ingest per frame: colour %s ms, gray %s ms" % (result["k_ingest_ms_per_frame_a"], result["k_ingest_ms_per_frame_c"]), flush=True)
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out)
