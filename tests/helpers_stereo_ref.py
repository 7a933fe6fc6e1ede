"""The stereo pin's corpus and fixtures: Frame::ComputeStereoMatches, ComputeStereoMatches_Lines (with lineSegmentOverlapStereo and
filterLineSegmentDisparity), matchGrid, matchNNR, match, distance, GetFeaturesInArea and ComputeStereoFromRGBD as the reference's own
text computes them, compiled into oracle/_ref/pli_ref_stereo (oracle/Makefile: ref_stereo; the stand-in it compiles against is
oracle/ref_recipe/stereo_shim), run over the constructed stereo cases of tests/helpers_matchers.py and a few tables of this file.

  build_all(po)         every reference case: name -> (the inputs a fixture stores, the arrays the program is given), and what
                        was removed on the way
  run_reference         one call of pli_ref_stereo as a child process; a call that throws or aborts raises
  save_fixture / load_fixture    tests/golden/stereo_ref/<case>.npz: "in/<array>" and "out/<array>"
  case_of_fixture       a points / lines fixture as a case of helpers_matchers' corpus (images, tables, configuration)
  generate(po)          writes all fixtures and manifest.json (coverage counts, dropped cases), asserts the coverage conditions;
                        or reruns every case through another build of the program and compares

THE REFERENCE ALONE MUST HAVE DEFINED BEHAVIOUR ON EVERY CASE.  This project defines an answer where the reference has none:
a SAD window that rowRange / colRange rejects (labels left_window_outside_level, strip_window_outside_level), an empty vDistIdx
(frame tag survivors_none), matches_[idx][1] with fewer than two train rows, a right keypoint whose row band leaves vRowIndices.
Left rows with those labels, right rows with such a band, and whole cases with survivors_none or short train tables are removed
before a case goes to the reference (UNDEFINED_*), and recorded.  Coverage is counted from helpers_matchers' labels alone.

tools/gen_stereo_ref.py writes the fixtures; tests/test_ref_pin_stereo.py and tests/test_ref_pin_stereo_gpu.py read them.  Nothing
here reads the reference tree; run_reference needs the program oracle/Makefile built from it.
"""
import io
import json
import os
import subprocess
import tempfile
import zipfile
from collections import Counter

import numpy as np

import helpers_matchers as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_DIR = os.path.join(ROOT, "tests", "golden", "stereo_ref")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "pli_ref_stereo")
MANIFEST = os.path.join(GOLD_DIR, "manifest.json")
FUNCTIONS = ("points", "lines", "overlap", "filter", "nnr", "match", "dist", "area", "rgbd")
f32, f64 = np.float32, np.float64
W, H = 752, 480

UNDEFINED_POINT_EXITS = ("left_window_outside_level", "strip_window_outside_level")
UNDEFINED_FRAME_TAG = "survivors_none"
POINT_EXITS = [l for l in hm.POINT_LABELS[:14] if l not in UNDEFINED_POINT_EXITS]
LINE_EXITS = hm.LINE_LABELS[:8]
# (`if (overlap > 1.f)` is not among them: it cannot be taken.  With length = eln - spn > 0.01 and the segments not disjoint, the
# overlap is eln - sln with spn < sln, or min(eln, epn) - max(sln, spn) <= eln - spn: never more than the length.)
OVERLAP_BRANCHES = ["overlap_left_horizontal", "overlap_disjoint", "overlap_right_contains_left", "overlap_partial",
                    "overlap_length_le_0.01"]


# ------------------------------------------------------------------------------------------------------ the reference program
def reference_functions(exe=REF_EXE):
    if not os.path.exists(exe):
        return ()
    return tuple(subprocess.run([exe, "--functions"], check=True, capture_output=True, text=True, timeout=60).stdout.split())


def run_reference(bag, exe=REF_EXE):
    """One call of the reference program: the result arrays by name.  A run that throws (status 3) or aborts raises."""
    from helpers_match_ref import read_bag, write_bag
    with tempfile.TemporaryDirectory() as d:
        req, rsp = os.path.join(d, "case"), os.path.join(d, "result")
        write_bag(req, bag)
        subprocess.run([exe, req, rsp], check=True, timeout=300)
        return read_bag(rsp)


def _fn(name):
    return np.frombuffer(name.encode(), np.uint8)


# ---------------------------------------------------------------------------------------------------------------- fixtures
def fixture_path(name):
    return os.path.join(GOLD_DIR, name + ".npz")


def save_fixture(name, inputs, results):
    """A .npz whose bytes depend on its arrays alone (fixed entry dates, sorted names)."""
    os.makedirs(GOLD_DIR, exist_ok=True)
    flat = {"in/" + k: v for k, v in inputs.items()}
    flat.update({"out/" + k: v for k, v in results.items()})
    with zipfile.ZipFile(fixture_path(name), "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(flat):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(flat[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


_FIX = {}


def load_fixture(name):
    """-> (inputs, results); read once, left unchanged."""
    if name not in _FIX:
        z = np.load(fixture_path(name))
        ins, outs = {}, {}
        for key in z.files:
            kind, rest = key.split("/", 1)
            (ins if kind == "in" else outs)[rest] = z[key]
        for a in list(ins.values()) + list(outs.values()):
            a.setflags(write=False)
        _FIX[name] = (ins, outs)
    return _FIX[name]


def manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def fixture_names():
    return sorted(n[:-4] for n in os.listdir(GOLD_DIR) if n.endswith(".npz"))


def _text(a):
    return bytes(np.asarray(a, np.uint8)).decode()


# ------------------------------------------------------------------------------------------------------------ bags of a case
def _kp3(kp):
    return np.stack([kp["x"], kp["y"], kp["octave"].astype(f32)], 1).astype(f32).reshape(len(kp), 3)


def _kl4(kl):
    return np.stack([kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"]], 1).astype(f32).reshape(len(kl), 4)


def cfg_lines(cfg):
    return np.array([cfg.matching_s_ws, cfg.best_lr_matches, cfg.line_sim_th, cfg.min_ratio_12_l, cfg.min_disp, cfg.line_horiz_th,
                     cfg.stereo_overlap_th, cfg.ls_min_disp_ratio], f64)


def rig_of(cfg):
    """(mb, mbf): mb = mbf / fx in float (Frame.cc:197), or 0 where the case asks for maxD = +inf (mb read before it is set)."""
    bf = f32(cfg.bf)
    return np.array([f32(0) if cfg.stereo_maxd_inf else f32(bf / f32(cfg.fx)), bf], f32)


def points_bag(c):
    cfg = c["cfg"]
    sf, inv = hm.scale_factors(cfg.orb_nlevels, cfg.orb_scale_factor)
    bag = dict(fn=_fn("points"), kpL=_kp3(c["kpL"]), kpR=_kp3(c["kpR"]), descL=c["descL"], descR=c["descR"], sf=sf, inv_sf=inv, rig=rig_of(cfg))
    for e, k in enumerate("LR"):
        for l in range(cfg.orb_nlevels):
            bag["pyr%s%d" % (k, l)] = np.ascontiguousarray(c["pyr"][e][l], np.uint8)
    return bag


def lines_bag(c):
    return dict(fn=_fn("lines"), klL=_kl4(c["klL"]), klR=_kl4(c["klR"]), ldL=c["ldL"], ldR=c["ldR"], cfg=cfg_lines(c["cfg"]),
                inv=np.array([hm.GRID_COLS / float(c["W"]), hm.GRID_ROWS / float(c["H"])], f64))


# ------------------------------------------------------------------------------------------ removing what the reference cannot take
def right_band_outside(c):
    """Right keypoints whose row band floor(y - r) .. ceil(y + r) leaves [0, nRows): vRowIndices[yi] out of range."""
    sf, _ = hm.scale_factors(c["cfg"].orb_nlevels, c["cfg"].orb_scale_factor)
    kp = c["kpR"]
    if not len(kp):
        return np.zeros(0, np.int64)
    r = (f32(2.0) * sf[kp["octave"]]).astype(f32)
    lo, hi = np.floor((kp["y"] - r).astype(f32)), np.ceil((kp["y"] + r).astype(f32))
    return np.flatnonzero((lo < 0) | (hi >= c["H"]))


def reduce_point_case(c):
    """-> (reduced case or None, dropped left rows, their labels, dropped right rows, case label or None)."""
    dr = right_band_outside(c)
    c1 = dict(c)
    if dr.size:
        keep = np.setdiff1d(np.arange(len(c["kpR"])), dr)
        c1["kpR"], c1["descR"] = c["kpR"][keep], c["descR"][keep]
    ex = hm.run_points(c1)[4]
    dl = np.array([i for i, e in enumerate(ex) if e and e[0] in UNDEFINED_POINT_EXITS], np.int64)
    labels = [ex[i][0] for i in dl]
    if dl.size:
        keep = np.setdiff1d(np.arange(len(c["kpL"])), dl)
        c1["kpL"], c1["descL"] = c["kpL"][keep], c["descL"][keep]
    r = hm.run_points(c1)
    assert not [e for e in r[4] if e and e[0] in UNDEFINED_POINT_EXITS]
    if UNDEFINED_FRAME_TAG in r[5]:
        return None, dl, labels, dr, UNDEFINED_FRAME_TAG
    return c1, dl, labels, dr, None


# --------------------------------------------------------------------------------------------------------------- the corpus
_IMAGES = {}


def images():
    """The natural images of the point cases, by name.  The synthetic pair keeps its four upper bits and the photograph its five
    upper bits (whole, the four images alone are larger than the size cap); the small pipeline pair keeps four."""
    if not _IMAGES:
        from pli_slam_amd import realdata, synth
        sl, sr = synth.make_stereo_pair(0, W, H)
        pl, pr = realdata.frames_752x480(1, seed=1)[0]
        ql, qr = synth.make_stereo_pair(3, PIPE_W, PIPE_H)
        _IMAGES.update(synthL=np.ascontiguousarray(sl & 0xF0), synthR=np.ascontiguousarray(sr & 0xF0), photoL=np.ascontiguousarray(pl & 0xF8),
                       photoR=np.ascontiguousarray(pr & 0xF8), pipeL=np.ascontiguousarray(ql & 0xF0), pipeR=np.ascontiguousarray(qr & 0xF0))
    return _IMAGES


IMAGE_OF = {"same_synth": ("synthL", "synthL"), "same_photo": ("photoL", "photoL"), "synth_pair": ("synthL", "synthR"),
            "synth_pair_maxd_inf": ("synthL", "synthR"), "photo_pair": ("photoL", "photoR"), "photo_pair_maxd_inf": ("photoL", "photoR"),
            "pipeline_small": ("pipeL", "pipeR")}


def _with_pyramids(po, c):
    fr = po.Frame(c["cfg"])
    c["pyr"] = []
    for eye, img in ((0, c["L"]), (1, c["R"])):
        fr.orb_extract(eye, img)
        c["pyr"].append([fr.pyramid(eye, l) for l in range(c["cfg"].orb_nlevels)])
    return c


def extra_point_cases():
    """Exits the constructed cases of helpers_matchers reach fewer than five times: more of them, on the constant pair."""
    out = []
    P = hm._Pairs(41)
    slots = []
    for k in range(6):                                   # maxU < 0; iniu < 0; Hamming at / above the two limits
        P.pair(-1.5 - k, 40 + 20 * k, 0)
        i = P.left(30 + k, 200 + 20 * k, 0); P.right(-1.0 - k, 200 + 20 * k, 0, of=i)
        P.pair(300 + 10 * k, 60, 0, bits=75 + k)
        P.pair(300 + 10 * k, 100, 0, bits=100 + k)
        i = P.left(400 + 30 * k, 370 + 3 * k, 0); P.right(400 + 30 * k, 10, 0, of=i)          # no right keypoint on its row
    for k in range(6):                                   # endu >= cols; disparity >= maxD cannot be had on this rig: see const_maxd
        i = P.left(W - 6, 400 + 10 * k, 0); P.right(W - 11 + (k % 3), 400 + 10 * k, 0, of=i)
        if k % 3 == 0:                                   # endu == cols with a clear SAD minimum behind it, were the test `>`
            slots.append((W - 11, 400 + 10 * k, hm.sad_profile(10, 5, 5, 0)))
    for k in range(6):                                   # SAD minima at the two ends of the strip, negative disparities
        cx, cy = 100 + 60 * k, 150
        slots.append((cx, cy, hm.sad_profile(3, 9, 9, -5 if k % 2 else 5)))
        i = P.left(cx + 20, cy, 0); P.right(cx, cy, 0, of=i)
    for k in range(6):
        cx, cy = 100 + 60 * k, 270
        slots.append((cx, cy, hm.sad_profile(12, 5, 5, -2)))
        i = P.left(cx - 3, cy, 0); P.right(cx, cy, 0, of=i)                                   # uR > uL: outside [minU, maxU]
        slots.append((cx, cy + 30, hm.sad_profile(12, 5, 5, 2)))
        i = P.left(cx + 1, cy + 30, 0); P.right(cx, cy + 30, 0, of=i)                         # best at +2: disparity 1 - 2 < 0
        slots.append((cx, cy + 60, hm.sad_profile(12 + k, 5, 5, 0)))
        i = P.left(cx, cy + 60, 0); P.right(cx, cy + 60, 0, of=i)                             # disparity 0: the 0.01 rewrite
    L, R = hm.constant_pair_with_markers(W, H, slots)
    out.append(hm.validate_tables(dict(name="extra_exits", W=W, H=H, nlevels=8, L=L, R=R, cfg={}, **P.tables(), **hm._empty_lines())))
    # disparity >= maxD on a rig with maxD = 512, and sads far above the median (the cut)
    P = hm._Pairs(42)
    slots = []
    for k, (v, a, b, inc, du) in enumerate(((10, 5, 5, 0, 512), (10, 8, 24, 0, 512), (10, 8, 24, 0, 511.75), (10, 8, 24, 0, 511.875),
                                            (0, 7, 7, -4, 508), (0, 7, 7, -4, 509.5))):
        cx, cy = 60 + 20 * k, 40 + 30 * k
        slots.append((cx, cy, hm.sad_profile(v, a, b, inc)))
        i = P.left(f32(cx + du), cy, 0); P.right(cx, cy, 0, of=i)                               # disparity du - inc - deltaR >= 512
    for k in range(8):
        cx, cy = 100 + 40 * k, 300
        slots.append((cx, cy, hm.sad_profile(10 if k < 5 else 60 + k, 5, 5, 0)))
        i = P.left(cx + 20, cy, 0); P.right(cx, cy, 0, of=i)
    L, R = hm.constant_pair_with_markers(W, H, slots)
    out.append(hm.validate_tables(dict(name="extra_maxd_cut", W=W, H=H, nlevels=8, L=L, R=R, cfg=dict(bf=64.0, fx=512.0), **P.tables(),
                                       **hm._empty_lines())))
    return out


def extra_line_cases():
    """Line exits that build_line_cases reaches fewer than five times."""
    rng = np.random.default_rng(43)
    out = []

    def add(name, L, R, dists, **cfg):
        n1, n2 = len(L), len(R)
        ldL = rng.integers(0, 256, (n1, 32), dtype=np.uint8); ldR = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        done = set()
        for (i, j), d in dists.items():
            if j in done:
                ldL[i] = hm._flip(ldR[j], d)
            else:
                ldR[j] = hm._flip(ldL[i], d); done.add(j)
        out.append(hm.validate_tables(dict(name=name, W=W, H=H, nlevels=8, L=None, R=None, cfg=cfg, klL=hm._kl(L), ldL=ldL, klR=hm._kl(R),
                                           ldR=ldR, **hm._empty_points())))
    L, R, D = [], [], {}
    for k in range(6):
        x = 60 + 110 * k
        # two right candidates: 9 against 10 fails the ratio test at 0.9, in double and in float
        L.append((x, 40, x + 4, 110)); R.append((x - 5, 40, x - 1, 110)); R.append((x - 4, 40, x, 110))
        D[(len(L) - 1, len(R) - 2)] = 18 + k; D[(len(L) - 1, len(R) - 1)] = 20 + k
        # two left lines on one right line: the farther one fails the mutual check
        L.append((x, 150, x + 4, 220)); L.append((x + 2, 150, x + 6, 220)); R.append((x - 5, 150, x - 1, 220))
        D[(len(L) - 2, len(R) - 1)] = 10; D[(len(L) - 1, len(R) - 1)] = 4
        # a horizontal left line with a partner: matched by matchGrid, rejected as horizontal
        L.append((x, 260, x + 60, 260.05)); R.append((x - 6, 260, x + 54, 260.05)); D[(len(L) - 1, len(R) - 1)] = 2
        # overlap below the threshold; disparity below min_disp; a line with no right line in its window
        L.append((x, 300, x + 4, 400)); R.append((x - 6, 300, x - 4, 350)); D[(len(L) - 1, len(R) - 1)] = 2
        L.append((x + 20, 300, x + 24, 400)); R.append((x + 19.5, 300, x + 23.5, 400)); D[(len(L) - 1, len(R) - 1)] = 2
        L.append((x + 40, 420, x + 44, 470))
    add("lines_extra_exits", L, R, D)
    add("lines_none_right_6", [(100 + 20 * k, 100, 104 + 20 * k, 180) for k in range(6)], [], {})
    # equal best distances (the ratio test rejects them), and single candidates far away that still match (best_d2 == INT_MAX)
    L, R, D = [], [], {}
    for k in range(5):
        x = 60 + 130 * k
        L.append((x, 40, x + 4, 110)); R.append((x - 5, 40, x - 1, 110)); R.append((x - 4, 40, x, 110))
        D[(len(L) - 1, len(R) - 2)] = 12; D[(len(L) - 1, len(R) - 1)] = 12
        L.append((x, 200, x + 4, 280)); R.append((x - 7, 200, x - 3, 280)); D[(len(L) - 1, len(R) - 1)] = 200 + k
    add("lines_equal_best_and_single", L, R, D)
    return out


def point_cases(po):
    im = images()
    cases = hm.build_point_cases((im["synthL"], im["synthR"]), (im["photoL"], im["photoR"])) + extra_point_cases()
    for c in cases:
        c["cfg"] = po.default_config(c["W"], c["H"], **c["cfg"])
        hm.validate_tables(_with_pyramids(po, c))
    return cases


def line_cases(po):
    cases = hm.build_line_cases() + extra_line_cases()
    for c in cases:
        c["cfg"] = po.default_config(c["W"], c["H"], **c["cfg"])
        c["pyr"] = None
    return cases


PIPE_W, PIPE_H = 320, 240


def pipeline_case(po):
    """One small pipeline case: the oracle's extractors on a synthetic pair."""
    L, R = images()["pipeL"], images()["pipeR"]
    cfg = po.default_config(PIPE_W, PIPE_H, orb_nfeatures=300, lsd_nfeatures=60)
    fr = po.Frame(cfg)
    t = {}
    for eye, img, k in ((0, L, "L"), (1, R, "R")):
        _, t["kp" + k], t["desc" + k] = fr.orb_extract(eye, img)
        _, t["kl" + k], t["ld" + k] = fr.line_extract(eye, img)
    pyr = [[fr.pyramid(e, l) for l in range(8)] for e in (0, 1)]
    return dict(name="pipeline_small", W=PIPE_W, H=PIPE_H, nlevels=8, cfg=cfg, pyr=pyr, L=L, R=R, **t)


def overlap_table():
    rng = np.random.default_rng(51)
    rows = []
    for k in range(8):
        y = 100.0 + 10 * k
        rows += [(y, y + 0.05, y, y + 40), (y, y + 0.1, y - 3, y + 9),                          # horizontal (|dy| <= 0.1)
                 (y, y + 50, y + 60 + k, y + 90), (y + 50, y, y - 40, y - 1 - k),              # disjoint, above and below
                 (y, y + 50, y - 5 - k, y + 60), (y + 50, y, y + 70, y - 2),                   # right contains left
                 (y, y + 50, y + 10 + k, y + 40), (y, y + 50, y - 20, y + 25 + k), (y, y + 50, y + 30, y + 80),   # partial
                 (y, y + 50, y + 49.995, y + 50), (y, y + 0.125, y + 0.12, y + 0.125),         # length = eln - spn <= 0.01
                 (y, y + 50, y + 45, y + 200 + k), (y, y + 50, y - 1, y + 49.5)]               # partial, a short and a long length
    rows += [(float("nan"), 1.0, 0.0, 1.0), (0.0, 10.0, float("nan"), 5.0), (0.0, 10.0, 5.0, float("nan")), (0.0, float("inf"), 0.0, 5.0)]
    rnd = rng.uniform(0, 480, (60, 4))
    return np.concatenate([np.array(rows, f64), rnd]).astype(f64)


def filter_table():
    rng = np.random.default_rng(52)
    rows = []
    for k in range(6):
        x = 100.0 + 7 * k
        rows += [(x, 0, x + 4, 80, x - 10, 0, x - 6, 80),                 # equal disparities
                 (x, 0, x + 4, 80, x - 20, 0, x, 80),                      # ratio 4 / 20: reset
                 (x, 0, x + 4, 80, x + 5, 0, x - 9, 80),                   # mixed sign: a negative ratio
                 (x, 0, x + 4, 80, x + 5, 0, x + 12, 80),                  # both negative: ratio > 1
                 (x, 0, x + 4, 80, x, 0, x + 4, 80),                       # 0 / 0: NaN
                 (x, 0, x + 4, 80, float("nan"), 0, x, 80), (x, 0, x + 4, 80, x - 3, 0, float("nan"), 80),
                 (x, 0, x + 4, 80, float("-inf"), 0, float("-inf"), 80),   # inf / inf: NaN
                 (x, 0, x + 4, 80, x - 7, 0, x - 6, 80)]                   # 7 / 10 == 0.7: not below
    return np.concatenate([np.array(rows, f64), rng.uniform(0, 752, (40, 8))]).astype(f64)


def descriptor_tables():
    a, b, c, d = hm.descriptor_tables_random_and_ties()
    return dict(random=(a, b), low_entropy=(c, d), short=(a[:5], b[:2]))


def descriptor_inputs(name):
    """(d1, d2) of an nnr / match fixture: its own arrays, or the shared tables its name points to."""
    ins = load_fixture(name)[0]
    if "d1" in ins:
        return ins["d1"], ins["d2"]
    t = load_fixture("descriptor_tables")[0]
    tag = _text(ins["tables"])
    return t[tag + "_q"], t[tag + "_t"]


def descriptor_cases():
    """-> {name: bag} for nnr / match / dist; train tables shorter than two rows never go to the reference."""
    a, b, c, d = hm.descriptor_tables_random_and_ties()
    out = {}
    for tag, q, t in (("random", a, b), ("low_entropy", c, d), ("short", a[:5], b[:2])):
        for nnr in (0.9, 0.75, 1.0):
            out["nnr_%s_%g" % (tag, nnr)] = dict(fn=_fn("nnr"), d1=q, d2=t, params=np.array([nnr], f64))
            for lr in (1, 0):
                out["match_%s_%g_lr%d" % (tag, nnr, lr)] = dict(fn=_fn("match"), d1=q, d2=t, params=np.array([nnr, lr], f64))
    for k, (q, t, d0, d1) in enumerate(hm.nnr_float_boundary_tables()):
        for nnr in (0.9, 0.6):
            out["nnr_boundary_%d_%d_%g" % (d0, d1, nnr)] = dict(fn=_fn("nnr"), d1=q, d2=t, params=np.array([nnr], f64))
    out["dist_random"] = dict(fn=_fn("dist"), a=a[:257], b=b)
    out["dist_low_entropy"] = dict(fn=_fn("dist"), a=c[:70], b=d)
    for name, bag in out.items():
        assert len(bag.get("d2", b)) >= 2 and (bag["fn"].tobytes() != b"match" or len(bag["d1"]) >= 2), name
    return out


AREA_BOUNDS = (0.0, 640.0, 0.0, 480.0)


def area_cases():
    """-> {name: bag}: a one-camera frame (undistorted keypoints, bounds that do not start at 0 too) and a two-camera frame."""
    out = {}
    for name, seed, bounds, nleft in (("area_one_camera", 61, AREA_BOUNDS, -1), ("area_one_camera_offset", 62, (-12.5, 651.25, -7.75, 489.5), -1),
                                      ("area_two_cameras", 63, AREA_BOUNDS, 260)):
        rng = np.random.default_rng(seed)
        n = 400
        kp = np.zeros((n, 3), f32)
        kp[:, 0] = rng.uniform(bounds[0] - 5, bounds[1] + 5, n); kp[:, 1] = rng.uniform(bounds[2] - 5, bounds[3] + 5, n)
        kp[:, 2] = rng.integers(0, 8, n)
        kp[:8, 0] = np.array([0.0, 4.9, 5.0, 5.1, 639.9, 635.0, 320.0, 325.0], f32) + f32(bounds[0])      # cell borders (10 px wide cells)
        kp[:8, 1] = np.array([0.0, 4.9, 5.0, 5.1, 479.9, 475.0, 240.0, 245.0], f32) + f32(bounds[2])
        m = 160
        q = np.zeros((m, 6), f32)
        src = rng.integers(0, n, m)
        q[:, 0] = kp[src, 0] + rng.uniform(-6, 6, m); q[:, 1] = kp[src, 1] + rng.uniform(-6, 6, m)
        q[:, 2] = np.where(rng.random(m) < 0.7, rng.uniform(2, 40, m), rng.uniform(60, 300, m))
        q[:, 3] = rng.integers(-1, 4, m); q[:, 4] = np.where(rng.random(m) < 0.4, -1, q[:, 3] + rng.integers(0, 5, m))
        q[:10, 0] = [-500, 1500, 100, 100, 0, 640, 320, 320, -39.9, 679.9]      # windows that leave the grid on every side
        q[:10, 1] = [100, 100, -500, 1500, 0, 480, 240, 240, 100, 100]
        q[:10, 2] = [40, 40, 40, 40, 10, 10, 10, 0, 40, 40]
        q[10:14, 2] = kp[src[10:14], 0] * 0 + np.abs(kp[src[10:14], 0] - q[10:14, 0])           # |dx| == r: excluded
        q[:, 5] = (rng.random(m) < 0.5) if nleft != -1 else 0
        out[name] = dict(fn=_fn("area"), kp=kp, nleft=np.array([nleft], np.int32), bounds=np.array(bounds, f32), q=q)
    return out


def area_restated(bag):
    """helpers_matchers._cells / _area (what the matcher pins rest on) over the bag -> the lists, in walking order."""
    kp3, nleft, bounds = bag["kp"], int(bag["nleft"][0]), tuple(float(b) for b in bag["bounds"])
    def table(rows):
        kp = np.zeros(len(rows), hm.KEYPOINT_DT)
        kp["x"], kp["y"], kp["octave"] = rows[:, 0], rows[:, 1], rows[:, 2].astype(np.int32)
        return (kp,) + tuple(hm._cells(kp, bounds))
    sides = [table(kp3)] if nleft == -1 else [table(kp3[:nleft]), table(kp3[nleft:])]
    lists = []
    for r in bag["q"]:
        Q = dict(u=r[0], v=r[1], radius=r[2], min_level=int(r[3]), max_level=int(r[4]))
        kp, px, py, ingrid, gw, gh = sides[int(r[5] != 0)]
        idx = hm._area(Q, kp, px, py, ingrid, bounds, gw, gh, [])
        lists.append(np.zeros(0, np.int32) if idx is None else idx.astype(np.int32))
    return lists


def rgbd_case():
    rng = np.random.default_rng(71)
    n, w, h = 120, 48, 32
    kp = np.zeros((n, 3), f32)
    kp[:, 0] = rng.uniform(0, w - 1, n); kp[:, 1] = rng.uniform(0, h - 1, n)
    depth = rng.uniform(0.3, 8.0, (h, w)).astype(f32)
    depth[rng.random((h, w)) < 0.3] = 0
    depth[rng.random((h, w)) < 0.05] = -1
    return dict(fn=_fn("rgbd"), kp=kp, kpun=kp.copy(), depth_image=depth, rig=np.array([0.11, 47.90639384423901], f32))


# ------------------------------------------------------------------------------------------------ a case as the tests take it
def stored_tables(c):
    return dict(kpL=c["kpL"], descL=c["descL"], kpR=c["kpR"], descR=c["descR"], klL=c["klL"], ldL=c["ldL"], klR=c["klR"], ldR=c["ldR"],
                cfg=np.frombuffer(bytes(c["cfg"]), np.uint8), size=np.array([c["W"], c["H"], c["nlevels"]], np.int32))


def case_of_fixture(name, config_type, po=None):
    """The case a points / lines fixture holds, as helpers_matchers' corpus shapes it.  config_type: the Config structure the
    caller works with (the oracle's or the device's: one layout).  po: the oracle, where the pyramids are wanted (CPU tests)."""
    ins, outs = load_fixture(name)
    c = {k: ins[k] for k in ("kpL", "descL", "kpR", "descR", "klL", "ldL", "klR", "ldR")}
    c["name"] = name
    c["cfg"] = config_type.from_buffer_copy(bytes(ins["cfg"]))
    c["W"], c["H"], c["nlevels"] = (int(v) for v in ins["size"])
    c["L"] = c["R"] = c["pyr"] = None
    if "images" in ins:
        nl, nr = _text(ins["images"]).split(",")
        im = load_fixture("images")[0]
        c["L"], c["R"] = im[nl], im[nr]
    elif "L" in ins:
        c["L"], c["R"] = ins["L"], ins["R"]
    if po is not None and c["L"] is not None:
        _with_pyramids(po, c)
    return c, outs


# ------------------------------------------------------------------------------------------------------------ the generator
def build_all(po):
    """-> (fixtures {name: (inputs, bag)}, manifest dict).  Nothing is run here."""
    fixtures, man = {}, dict(dropped_cases={}, dropped_left_rows={}, dropped_right_rows={})
    fixtures["images"] = (dict(images()), None)
    for c in point_cases(po) + [pipeline_case(po)]:
        c1, dl, labels, dr, why = reduce_point_case(c)
        name = "points_" + c["name"]
        if dl.size:
            man["dropped_left_rows"][name] = {str(int(i)): l for i, l in zip(dl, labels)}
        if dr.size:
            man["dropped_right_rows"][name] = [int(i) for i in dr]
        if c1 is None:
            man["dropped_cases"][name] = why
            continue
        ins = stored_tables(c1)
        if c["name"] in IMAGE_OF:
            ins["images"] = _fn(",".join(IMAGE_OF[c["name"]]))
        else:
            ins["L"], ins["R"] = c["L"], c["R"]
        ins["dropped_left"] = dl.astype(np.int32); ins["dropped_right"] = dr.astype(np.int32)
        fixtures[name] = (ins, points_bag(c1))
    pipe = pipeline_case(po)
    for c in line_cases(po) + [pipe]:
        ins = stored_tables(c)
        if c["name"] in IMAGE_OF:
            ins["images"] = _fn(",".join(IMAGE_OF[c["name"]]))
        fixtures["lines_" + c["name"]] = (ins, lines_bag(c))
    cfg = po.default_config(W, H)
    fixtures["overlap"] = (dict(table=overlap_table(), cfg=cfg_lines(cfg)), dict(fn=_fn("overlap"), table=overlap_table(), cfg=cfg_lines(cfg)))
    fixtures["filter"] = (dict(table=filter_table(), cfg=cfg_lines(cfg)), dict(fn=_fn("filter"), table=filter_table(), cfg=cfg_lines(cfg)))
    tabs = descriptor_tables()
    fixtures["descriptor_tables"] = ({t + s: v for t, qt in tabs.items() for s, v in zip(("_q", "_t"), qt)}, None)
    for name, bag in list(descriptor_cases().items()) + list(area_cases().items()) + [("rgbd", rgbd_case())]:
        ins = {k: v for k, v in bag.items() if k != "fn"}
        tag = [t for t in tabs if name.startswith(("nnr_" + t + "_", "match_" + t + "_"))]
        if tag:
            ins = dict(params=bag["params"], tables=_fn(tag[0]))
        fixtures[name] = (ins, bag)
    return fixtures, man


def coverage(po, config_type=None):
    """Label counts over the committed fixtures (the reduced cases): exits of the two stereo functions, overlap branches, and the
    named conditions of the corpus."""
    config_type = config_type or po.Config
    pts, lns, ftags = Counter(), Counter(), Counter()
    for name in fixture_names():
        if name.startswith("points_"):
            c, _ = case_of_fixture(name, config_type, po)
            r = hm.run_points(c)
            for e in r[4]:
                pts.update(e[:1]); pts.update("tag:" + t for t in e[1:])
            ftags.update(r[5])
        elif name.startswith("lines_"):
            c, _ = case_of_fixture(name, config_type)
            for e in hm.stereo_lines(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"])[3]:
                lns.update(e[:1]); lns.update("tag:" + t for t in e[1:])
    ins = load_fixture("overlap")[0]
    ov = Counter()
    for r in ins["table"]:
        t = []
        hm.overlap_stereo(r[0], r[1], r[2], r[3], float(ins["cfg"][5]), tags=t)
        ov.update(t)
    ins = load_fixture("filter")[0]
    fl = Counter()
    for r in ins["table"]:
        t = []
        hm.filter_disparity(r[0], r[2], r[4], r[6], float(ins["cfg"][7]), tags=t)
        fl.update(t)
    nn = Counter()
    for name in fixture_names():
        if name.startswith("nnr_boundary_"):
            ins = load_fixture(name)[0]
            d1, d2 = descriptor_inputs(name)
            nn["nnr_boundary_%s" % ("accepted" if hm.match_nnr(d1, d2, float(ins["params"][0]))[0] else "rejected")] += 1
    return dict(point_exits={k: pts[k] for k in POINT_EXITS}, line_exits={k: lns[k] for k in LINE_EXITS},
                overlap_branches={k: ov[k] + lns["tag:" + k] for k in OVERLAP_BRANCHES},
                conditions={"disparity_zero_rewrite": pts["tag:disparity_zero"], "median_tie": ftags["equal_sads_around_median"],
                            "equal_sads_different_iL": ftags["equal_sads_around_median"],
                            "line_match_best_d2_INT_MAX": sum(1 for n in fixture_names() if n.startswith("lines_") for e in _line_exits(n, config_type)
                                                               if e[0] == "matched" and "single_candidate" in e),
                            "line_pair_equal_best_distances": sum(1 for n in fixture_names() if n.startswith("lines_")
                                                                  for _ in _equal_best(n, config_type)),
                            "negative_disparity_ratio": fl["disparity_ratio_negative"], "nan_disparity_ratio": fl["disparity_ratio_nan"],
                            "nnr_boundary_accepted": nn["nnr_boundary_accepted"], "nnr_boundary_rejected": nn["nnr_boundary_rejected"]})


def _line_exits(name, config_type):
    c, _ = case_of_fixture(name, config_type)
    return hm.stereo_lines(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"])[3]


def _equal_best(name, config_type):
    """Left lines whose two nearest right descriptors (over the whole right table) are equally far."""
    c, _ = case_of_fixture(name, config_type)
    if len(c["ldR"]) < 2:
        return []
    _, dist = hm.knn2(c["ldL"], c["ldR"])
    return [i for i in range(len(dist)) if dist[i, 0] == dist[i, 1] and dist[i, 0] < 64]


def check_coverage(cov):
    low = {k: v for part in ("point_exits", "line_exits", "overlap_branches") for k, v in cov[part].items() if v < 5}
    assert not low, "reached fewer than five times over the reference cases: %s" % low
    none = [k for k, v in cov["conditions"].items() if v < 1]
    assert not none, "the corpus does not hold: %s" % none


def generate(po, exe=REF_EXE, write=True):
    """Runs every case through the reference program.  write: save fixtures and the manifest; else only compare with what is there
    -> names that differ."""
    fixtures, man = build_all(po)
    differ = []
    if write:
        os.makedirs(GOLD_DIR, exist_ok=True)
        for stale in sorted(set(os.listdir(GOLD_DIR)) - {n + ".npz" for n in fixtures} - {"manifest.json"}):
            os.remove(os.path.join(GOLD_DIR, stale))
    for name, (ins, bag) in fixtures.items():
        res = run_reference(bag, exe) if bag is not None else {}
        if write:
            save_fixture(name, ins, res)
        else:
            old_in, old_out = load_fixture(name)
            same = set(old_in) == set(ins) and set(old_out) == set(res) and \
                all(np.ascontiguousarray(ins[k]).tobytes() == old_in[k].tobytes() for k in ins) and \
                all(np.ascontiguousarray(res[k]).tobytes() == old_out[k].tobytes() and res[k].dtype == old_out[k].dtype for k in res)
            if not same:
                differ.append(name)
    if write:
        _FIX.clear()
        man["coverage"] = coverage(po)
        check_coverage(man["coverage"])
        with open(MANIFEST, "w") as f:
            json.dump(man, f, indent=1, sort_keys=True)
            f.write("\n")
    return differ
