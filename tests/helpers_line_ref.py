"""Corpus of the line extractor pin (tests/test_ref_pin_line.py, tests/test_ref_pin_line_gpu.py, tools/gen_line_ref.py).

tests/golden/line_ref/<name>.npz holds what the reference's own Lineextractor::operator() returned for a case
(oracle/_ref/pli_ref_line and pli_ref_line_mathh, built by oracle/Makefile from the reference tree): the segments its detector
stand-in handed over, the key lines (all 17 fields), the 32-byte descriptors, the 72-float descriptors of a second
compute(..., returnFloatDescr = true), and SHA-256 digests of the dx / dy planes (the planes themselves for small images).
Where pli_ref_line_mathh returned the same bytes, the fixture says so (`mathh_same`) and holds them once.

Two kinds of case.  IMAGE cases run the detector (the oracle's restatement of cv::LineSegmentDetector, inside the reference's
detectImpl); the device runs them too.  SEGMENT cases replace the detector's output by a constructed list, so that the clamps,
the gate, ties and the cut are driven directly; CPU only.  Images are generated from a seed, a table or a crop of
tests/golden/real, never stored.

Ties.  Lineextractor sorts by response with std::sort, which is not stable for more than 16 elements; the oracle and the
device use a stable sort.  TIE_INSIDE names the cases constructed so that groups of equal responses lie wholly inside the kept
lines (rows inside one group may be permuted), TIE_STRADDLE those where a group straddles the cut (the kept members may differ).
Every other case must be free of equal responses among its lines before the cut whenever it cuts; tie_groups() computes the
groups from the fixture and check_tie_contract() asserts all of this, so a corpus that lost its ties fails.

restate() is a Python restatement of the reading (key lines, cut, LBD) with switches for deliberate misreadings (MUTANTS); the
pin test requires the plain restatement to equal the fixtures and every mutant to be rejected by them.
"""
import collections
import ctypes
import ctypes.util
import hashlib
import os
import struct
import subprocess
import tempfile

import numpy as np

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_ref")
KEYLINE_DT = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"),
                       ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"),
                       ("startPointX", "<f4"), ("startPointY", "<f4"), ("endPointX", "<f4"),
                       ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"), ("sPointInOctaveY", "<f4"),
                       ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"), ("lineLength", "<f4"),
                       ("numOfPixels", "<i4")])
assert KEYLINE_DT.itemsize == 68
FIELDS_WITHOUT_CLASS_ID = [f for f in KEYLINE_DT.names if f != "class_id"]
F32 = np.float32
# Examples/Stereo/Config/EuRoC.yaml: refine, scale, sigma_scale, quant, ang_th, log_eps, density_th, n_bins
LSD = dict(refine=0, scale=1.2, sigma_scale=0.6, quant=2.0, ang_th=22.5, log_eps=1.0, density_th=0.6, n_bins=1024)
LSD_FLAGS = 1           # the detector stand-in: CV_64F input, double trig in the grower (the project's defaults)
PLANES_STORED_UP_TO = 100 * 100

Case = collections.namedtuple("Case", "name image nfeatures min_line_length segments")


# ---------------------------------------------------------------------------------------------------------------- images
def real_crop(name, x0, y0, W, H):
    from pli_slam_amd import realdata
    img = realdata.photos()[name]
    assert y0 + H <= img.shape[0] and x0 + W <= img.shape[1]
    return np.ascontiguousarray(img[y0:y0 + H, x0:x0 + W])


def synth_image(W, H, seed, eye):
    from pli_slam_amd import synth
    return synth.make_stereo_pair(seed, W, H)[eye]


def flat_image(W, H, v=90):
    return np.full((H, W), v, np.uint8)


def bars_image(W, H, x0, x1, ys, thickness, lo=40, hi=200):
    """Noise-free horizontal bars of identical x-extent: every bar gives two horizontal edges of the same length."""
    img = np.full((H, W), lo, np.uint8)
    for y in ys:
        img[y:y + thickness, x0:x1] = hi
    return img


def frame_image(W, H, inset=6, lo=50, hi=190):
    """A bright rectangle whose sides run `inset` px from the four borders, plus short slanted strokes near each border: the
    63-row support bands of those lines leave the image on every side."""
    img = np.full((H, W), lo, np.uint8)
    img[inset:H - inset, inset:W - inset] = hi
    img[inset + 24:H - inset - 24, inset + 24:W - inset - 24] = lo + 30
    yy, xx = np.mgrid[0:H, 0:W]
    for (cx, cy, sl) in ((W // 2, 12, 0.15), (W // 2, H - 13, -0.2), (12, H // 2, 6.0), (W - 13, H // 2, -5.0)):
        d = np.abs((yy - cy) - sl * (xx - cx)) / np.sqrt(1 + sl * sl)
        near = (np.abs(xx - cx) < 40) & (np.abs(yy - cy) < 40) & (d < 2.0)
        img[near] = 20
    return img


def blobs_image(W, H, seed, n=40):
    """Small bright blobs on a flat background: short segments for min_line_length = 0."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 60, np.uint8)
    for _ in range(n):
        x, y = int(rng.integers(4, W - 10)), int(rng.integers(4, H - 10))
        w, h = int(rng.integers(2, 6)), int(rng.integers(2, 6))
        img[y:y + h, x:x + w] = int(rng.integers(140, 250))
    return img


def noise_image(W, H, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (H, W), dtype=np.uint8)


SEG_W, SEG_H = 96, 64


def _seg_image():
    return noise_image(SEG_W, SEG_H, 41, 30, 220)


# --------------------------------------------------------------------------------------------------------- segment lists
def _segs_clamps():
    """End points outside every border (all eight clamps of checkLineExtremes), one exactly on width / height (the clamps are >=),
    one that the clamp collapses to zero length, and ordinary ones."""
    W, H = float(SEG_W), float(SEG_H)
    return np.array([
        (-3.5, 10.0, 40.0, 12.0),          # x1 < 0
        (W + 2.0, 20.0, 30.0, 25.0),       # x1 >= W
        (50.0, 30.0, -0.25, 33.0),         # x2 < 0
        (20.0, 40.0, W, 44.0),             # x2 >= W (exactly W)
        (10.0, -2.0, 14.0, 30.0),          # y1 < 0
        (30.0, H + 5.0, 36.0, 20.0),       # y1 >= H
        (60.0, 50.0, 64.0, -7.0),          # y2 < 0
        (70.0, 10.0, 75.0, H),             # y2 >= H (exactly H)
        (-9.0, -9.0, W + 9.0, H + 9.0),    # four clamps at once
        (-5.0, -5.0, -3.0, -1.0),          # collapses to (0, 0)-(0, 0): length 0 is not > 0
        (W + 1.0, H + 4.0, W + 8.0, H + 1.0),   # collapses to (W-1, H-1)
        (W - 0.5, 5.0, 40.5, 5.5),         # W - 0.5 < W: not clamped, the iterator rounds it to W
        (12.25, 48.5, 55.75, 51.25),
        (33.0, 7.0, 33.0, 57.0),
        (20.5, 20.5, 60.5, 20.5),          # axis-aligned through pixel corners: every sample coordinate is a tie of round()
        (71.5, 50.5, 71.5, 12.5),
    ], np.float32)


def _segs_gate():
    """min_line_length 0.25 of min(96, 64) = 16.0: axis-aligned lengths exactly 16 (the gate is >), one ulp above and below, and
    equal responses from different (dx, dy): 20 = |(20, 0)| = |(0, 20)| = |(12, 16)| = |(16, 12)|."""
    up, dn = np.nextafter(F32(26.0), F32(100)), np.nextafter(F32(26.0), F32(0))
    return np.array([
        (10.0, 5.0, 26.0, 5.0),            # exactly 16: the gate is >, dropped
        (10.0, 8.0, up, 8.0),              # one ulp longer: kept
        (10.0, 11.0, dn, 11.0),            # one ulp shorter: dropped
        (40.0, 10.0, 40.0, 26.0),          # exactly 16, vertical: dropped
        (50.0, 10.0, 50.0, up),            # kept
        (10.0, 30.0, 30.0, 30.0),          # 20 from (20, 0)
        (60.0, 30.0, 60.0, 50.0),          # 20 from (0, 20)
        (10.0, 40.0, 22.0, 56.0),          # 20 from (12, 16)
        (70.0, 20.0, 86.0, 32.0),          # 20 from (16, 12)
        (30.0, 60.0, 50.0, 60.0),          # 20 again
        (5.0, 2.0, 90.0, 3.0),
        (2.0, 2.0, 3.0, 3.0),              # short: dropped
    ], np.float32)


def _segs_ties(n, seed, groups):
    """n segments inside the 96x64 image with distinct lengths, except that `groups` = [(first index, size, length)] makes runs of
    equal length at the given detection positions (horizontal, vertical and 3-4-5 members, so the (dx, dy) differ)."""
    rng = np.random.default_rng(seed)
    lengths = 4.0 + np.arange(n) * (52.0 / n) + 0.125      # distinct multiples of small dyadic steps
    lengths = rng.permutation(lengths)
    tied = {}
    for first, size, length in groups:
        for k in range(size):
            tied[first + k] = length
    out = []
    for i in range(n):
        L = float(tied.get(i, lengths[i]))
        kind = i % 3 if i in tied and L % 5 == 0 else i % 2
        if kind == 0:
            x = float(rng.integers(2, int(SEG_W - 2 - L)))
            y = float(rng.integers(2, SEG_H - 2))
            out.append((x, y, x + L, y))
        elif kind == 1:
            x = float(rng.integers(2, SEG_W - 2))
            y = float(rng.integers(2, int(SEG_H - 2 - L)))
            out.append((x, y + L, x, y))
        else:
            x = float(rng.integers(2, int(SEG_W - 2 - 0.8 * L)))
            y = float(rng.integers(2, int(SEG_H - 2 - 0.6 * L)))
            out.append((x, y, x + 0.8 * L, y + 0.6 * L))
    return np.array(out, np.float32)


# ----------------------------------------------------------------------------------------------------------------- cases
def _img(name, image, nfeatures, mll=0.025):
    return Case(name, image, nfeatures, mll, None)


def _seg(name, segments, nfeatures, mll=0.0):
    return Case(name, _seg_image, nfeatures, mll, segments)


BARS_YS = tuple(range(10, 206, 14))      # 14 bars: 28 horizontal edges of identical extent


def _bars():
    """The tie image: 14 identical bars, and 4 shorter ones of distinct lengths below them (they rank after every tie group)."""
    img = bars_image(376, 240, 60, 300, BARS_YS, 6)
    for k, y in enumerate((208, 216, 224, 232)):
        img[y:y + 4, 80:200 - 17 * k] = 200
    return img


def _camera():
    return real_crop("camera", 150, 100, 180, 240)     # portrait: max(cols, rows) and min(cols, rows) take different sides


CASES = [
    # two windows of the photographs (one of odd width) and the two eyes of one synthetic pair
    _img("real_coins_257x231_all", lambda: real_crop("coins", 60, 40, 257, 231), 0),
    _img("real_brick_376x240_small", lambda: real_crop("brick", 40, 100, 376, 240), 12),
    _img("synth_left_376x240_n60", lambda: synth_image(376, 240, 3, 0), 60),
    _img("synth_right_376x240_n200", lambda: synth_image(376, 240, 3, 1), 200),
    # portrait; min_line_length 0, and 0.2 (removes most: 15 lines stay), with lsd_nfeatures larger than, exactly and one under that count
    _img("real_camera_180x240_mll0", _camera, 0, 0.0),
    _img("real_camera_180x240_mll_most_larger", _camera, 500, 0.2),
    _img("real_camera_180x240_mll_most_exact", _camera, 15, 0.2),
    _img("real_camera_180x240_mll_most_minus1", _camera, 14, 0.2),
    _img("frame_257x231_bands", lambda: frame_image(257, 231), 0),
    _img("blobs_80x64_short", lambda: blobs_image(80, 64, 0), 0, 0.0),          # holds a line of numOfPixels = 2: halfWidth 0
    _img("flat_180x240_empty", lambda: flat_image(180, 240), 20),
    _img("bars_376x240_ties_inside", _bars, 28),
    _img("bars_376x240_ties_straddle", _bars, 20),
    # constructed segment lists
    _seg("seg_clamps", _segs_clamps, 0),
    _seg("seg_clamps_cut", _segs_clamps, 5),
    _seg("seg_gate", _segs_gate, 0, 0.25),
    _seg("seg_ties_16", lambda: _segs_ties(16, 1, [(2, 3, 20.0), (9, 2, 35.0)]), 10),
    _seg("seg_ties_17_inside", lambda: _segs_ties(17, 2, [(1, 4, 40.0), (8, 2, 45.0)]), 12),
    _seg("seg_ties_17_straddle", lambda: _segs_ties(17, 2, [(1, 4, 40.0), (8, 5, 30.0)]), 9),
    _seg("seg_ties_200_inside", lambda: _segs_ties(200, 3, [(5, 20, 50.0), (60, 7, 45.0), (120, 2, 55.0), (150, 11, 40.0)]), 120),
    _seg("seg_ties_200_straddle", lambda: _segs_ties(200, 3, [(5, 20, 30.0), (60, 7, 45.0), (120, 2, 55.0), (150, 11, 40.0)]), 120),
    _seg("seg_ties_200_past", lambda: _segs_ties(200, 4, [(10, 13, 10.0), (90, 6, 8.0)]), 60),
    _seg("seg_ties_200_nocut", lambda: _segs_ties(200, 3, [(5, 20, 30.0)]), 0),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
IMAGE_CASES = [c for c in CASES if c.segments is None]
SEGMENT_CASES = [c for c in CASES if c.segments is not None]
TIE_INSIDE = ("bars_376x240_ties_inside", "seg_ties_17_inside", "seg_ties_200_inside")
TIE_STRADDLE = ("bars_376x240_ties_straddle", "seg_ties_17_straddle", "seg_ties_200_straddle")
# 16 elements or fewer: libstdc++ sorts by insertion, which is stable; ties are allowed there and must match in place
TIE_SMALL = ("seg_ties_16", "seg_clamps_cut")


# -------------------------------------------------------------------------------------------- the reference's own program
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_reference(exe, case, image=None):
    """One run of oracle/_ref/pli_ref_line (or _mathh) as a child process: {"segs" (m, 4) f4, "kl" (KEYLINE_DT), "desc" (rows, 32) u8,
    "fdesc" (rows, 72) f4, "dx", "dy" (H, W) i2 or None, "stdout"}."""
    image = case.image() if image is None else image
    H, W = image.shape
    segs = np.zeros((0, 4), np.float32) if case.segments is None else np.ascontiguousarray(case.segments(), np.float32)
    with tempfile.TemporaryDirectory() as d:
        req, rsp = os.path.join(d, "request"), os.path.join(d, "response")
        with open(req, "wb") as f:
            f.write(struct.pack("<8i", 0 if case.segments is None else 1, W, H, case.nfeatures, LSD["refine"], LSD["n_bins"], LSD_FLAGS, len(segs)))
            f.write(struct.pack("<7d", case.min_line_length, LSD["scale"], LSD["sigma_scale"], LSD["quant"], LSD["ang_th"], LSD["log_eps"],
                                LSD["density_th"]))
            f.write(np.ascontiguousarray(image, np.uint8).tobytes())
            f.write(segs.tobytes())
        p = subprocess.run([exe, req, rsp], check=True, timeout=120, stdout=subprocess.PIPE)
        raw = open(rsp, "rb").read()
    o = 0

    def take(dtype, count, shape):
        nonlocal o
        a = np.frombuffer(raw, dtype, count, o).reshape(shape).copy()
        o += a.nbytes
        return a

    (m,) = struct.unpack_from("<i", raw, o); o += 4
    out = {"segs": take(np.float32, m * 4, (m, 4))}
    (n,) = struct.unpack_from("<i", raw, o); o += 4
    out["kl"] = take(KEYLINE_DT, n, (n,))
    (rows,) = struct.unpack_from("<i", raw, o); o += 4
    out["desc"] = take(np.uint8, rows * 32, (rows, 32))
    (rows_f,) = struct.unpack_from("<i", raw, o); o += 4
    out["fdesc"] = take(np.float32, rows_f * 72, (rows_f, 72))
    (planes,) = struct.unpack_from("<i", raw, o); o += 4
    out["dx"] = take(np.int16, W * H, (H, W)) if planes else None
    out["dy"] = take(np.int16, W * H, (H, W)) if planes else None
    assert o == len(raw)
    out["stdout"] = p.stdout.decode()
    return out


# -------------------------------------------------------------------------------------------------------------- fixtures
def fixture_path(name):
    return os.path.join(GOLD_DIR, name + ".npz")


def _pack(res, W, H):
    a = {"kl": res["kl"].view(np.uint8).reshape(-1, KEYLINE_DT.itemsize), "desc": res["desc"], "fdesc": res["fdesc"],
         "empty_message": np.int32("keypoint list is empty" in res["stdout"])}
    if res["dx"] is not None:
        a["dx_sha"], a["dy_sha"] = np.array(_sha(res["dx"])), np.array(_sha(res["dy"]))
        if W * H <= PLANES_STORED_UP_TO:
            a["dx"], a["dy"] = res["dx"], res["dy"]
    return a


def save_fixture(case, res, res_mathh):
    os.makedirs(GOLD_DIR, exist_ok=True)
    H, W = case.image().shape
    assert np.array_equal(res["segs"], res_mathh["segs"])
    a, b = _pack(res, W, H), _pack(res_mathh, W, H)
    same = a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    arrays = {"segs": res["segs"], "mathh_same": np.int32(same)}
    arrays.update(a)
    if not same:
        arrays.update({"mathh_" + k: v for k, v in b.items()})
    np.savez_compressed(fixture_path(case.name), **arrays)


def load_fixture(name, mathh=False):
    """The recorded result of pli_ref_line (or, mathh=True, of pli_ref_line_mathh): {"segs", "kl", "desc", "fdesc", "dx_sha",
    "dy_sha" (None where computeSobel never ran), "dx", "dy" (None where not stored), "empty_message", "mathh_same"}."""
    z = np.load(fixture_path(name))
    same = bool(z["mathh_same"])
    pre = "mathh_" if mathh and not same else ""
    g = lambda k: z[pre + k] if pre + k in z.files else None
    sha = lambda k: None if g(k) is None else str(g(k))
    return {"segs": z["segs"], "kl": g("kl").view(KEYLINE_DT).reshape(-1), "desc": g("desc"), "fdesc": g("fdesc"),
            "dx_sha": sha("dx_sha"), "dy_sha": sha("dy_sha"), "dx": g("dx"), "dy": g("dy"),
            "empty_message": bool(g("empty_message")), "mathh_same": same}


def result_of_fixture_form(res, case):
    """A live run_reference result in load_fixture's form."""
    H, W = case.image().shape
    a = _pack(res, W, H)
    return {"segs": res["segs"], "kl": res["kl"], "desc": res["desc"], "fdesc": res["fdesc"],
            "dx_sha": str(a["dx_sha"]) if "dx_sha" in a else None, "dy_sha": str(a["dy_sha"]) if "dy_sha" in a else None,
            "dx": a.get("dx"), "dy": a.get("dy"), "empty_message": bool(a["empty_message"])}


# ------------------------------------------------------------------------------------------------------------------ ties
def clamp_segments(segs, W, H):
    """checkLineExtremes on every row, and which of its eight clamps fired: (clamped (m, 4) f4, fired (m, 8) bool in the order
    x1<0, x1>=W, x2<0, x2>=W, y1<0, y1>=H, y2<0, y2>=H)."""
    e = np.array(segs, np.float32).reshape(-1, 4).copy()
    fired = np.zeros((len(e), 8), bool)
    for j, (col, lim) in enumerate(((0, W), (2, W), (1, H), (3, H))):
        lo = e[:, col] < 0
        e[lo, col] = 0
        hi = e[:, col] >= lim
        e[hi, col] = F32(lim) - F32(1)
        fired[:, 2 * j], fired[:, 2 * j + 1] = lo, hi
    return e, fired


def lengths_of(e):
    """(float) sqrt( pow( x1 - x2, 2 ) + pow( y1 - y2, 2 ) ): float differences, double squares, sum and root."""
    ddx = (e[:, 0] - e[:, 2]).astype(np.float64)
    ddy = (e[:, 1] - e[:, 3]).astype(np.float64)
    return np.sqrt(ddx * ddx + ddy * ddy).astype(np.float32)


def before_cut(case, fix):
    """(responses f4 in detection order of the lines that pass the gate, min_length): from the fixture's segments alone."""
    H, W = case.image().shape
    e, _ = clamp_segments(fix["segs"], W, H)
    length = lengths_of(e)
    min_length = case.min_line_length * min(W, H)
    keep = length.astype(np.float64) > min_length
    return (length[keep] / F32(max(W, H))).astype(np.float32), min_length


def tie_groups(case, fix):
    """[(response, rank of the group's first member in the sorted order, size)] for every group of equal responses among the lines
    before the cut, and the number of lines kept (None: no cut)."""
    resp, _ = before_cut(case, fix)
    n = len(resp)
    cut = case.nfeatures if (case.nfeatures != 0 and n > case.nfeatures) else None
    vals, counts = np.unique(resp, return_counts=True)
    groups = []
    for v, c in zip(vals, counts):
        if c > 1:
            groups.append((float(v), int((resp > v).sum()), int(c)))
    return sorted(groups, key=lambda g: g[1]), cut


def classify_ties(case, fix):
    """(inside, straddle, past): the tie groups wholly kept, straddling the cut, wholly dropped; all three empty where nothing is cut
    (without a cut nothing is sorted)."""
    groups, cut = tie_groups(case, fix)
    if cut is None:
        return [], [], []
    inside = [g for g in groups if g[1] + g[2] <= cut]
    straddle = [g for g in groups if g[1] < cut < g[1] + g[2]]
    past = [g for g in groups if g[1] >= cut]
    return inside, straddle, past


def check_tie_contract(case, fix):
    """The named tie cases have the ties they were constructed for, among more than 16 lines; every other case that cuts has no
    equal responses at or before the cut."""
    inside, straddle, _ = classify_ties(case, fix)
    n = len(before_cut(case, fix)[0])
    if case.name in TIE_INSIDE:
        assert inside and not straddle and n > 16, (case.name, inside, straddle, n)
    elif case.name in TIE_STRADDLE:
        assert straddle and n > 16, (case.name, straddle, n)
    elif case.name in TIE_SMALL:
        assert n <= 16, (case.name, n)
    else:
        assert not inside and not straddle, (case.name, "unexpected response ties", inside, straddle)


# ------------------------------------------------------------------------------------------- a restatement with mutants
# Each name is ONE deliberate misreading; the fixtures must reject every one (tests/test_ref_pin_line.py).  Two suggested ones are
# not listed because they cannot be told from the reading by any input: re-numbering class_id without a cut (class_id already counts
# the kept lines in order) and comparing with 0.4f instead of 0.4 (the only float for which they disagree is 0.4f itself, which the
# branch replaces by 0.4f).
MUTANTS = ("gate_ge", "response_min", "class_id_counts_dropped", "class_id_kept_after_cut", "round_half_even", "half_width_from_length",
           "weights_real_division", "d_o_sign", "band_pair", "angle_swapped_arguments", "length_in_float")
LBD_COMBINATIONS = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6),
                    (2, 3), (2, 4), (2, 5), (2, 6), (2, 7), (2, 8), (3, 4), (3, 5), (3, 6), (3, 7), (3, 8),
                    (4, 5), (4, 6), (4, 7), (4, 8), (5, 6), (5, 7), (5, 8), (6, 7), (6, 8), (7, 8)]
_libm = None


def _m():
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for f in (_libm.cosf, _libm.sinf):
            f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
        _libm.atan2f.restype, _libm.atan2f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
        for f in (_libm.exp,):
            f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
    return _libm


def _round_half_away(v):
    v = v.astype(np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)


def _weights(real_division):
    m = _m()
    div = (lambda a, b: a / b) if real_division else (lambda a, b: float(a // b))
    u, sigma = div(7 * 3 - 1, 2), div(7 * 2 + 1, 2)
    inv = -1 / (2 * sigma * sigma)
    L = np.array([m.exp((i - u) * (i - u) * inv) for i in range(21)]).astype(np.float32)
    u = div(9 * 7 - 1, 2)
    inv = -1 / (2 * u * u)
    G = np.array([m.exp((i - u) * (i - u) * inv) for i in range(63)]).astype(np.float32)
    return L, G


def restate_keylines(segs, W, H, nfeatures, min_line_length, mut=None):
    """detectImpl(..., LSDOptions, ...) and the cut of Lineextractor::operator(), as the reference compiles on this toolchain (atan2f);
    a stable sort stands for std::sort (the tie rule of the comparison covers the difference)."""
    m = _m()
    e, _ = clamp_segments(segs, W, H)
    if mut == "length_in_float":
        fx, fy = e[:, 0] - e[:, 2], e[:, 1] - e[:, 3]
        length = np.sqrt(fx * fx + fy * fy).astype(np.float32)
    else:
        length = lengths_of(e)
    min_length = min_line_length * min(W, H)
    keep = (length.astype(np.float64) >= min_length) if mut == "gate_ge" else (length.astype(np.float64) > min_length)
    ids = (np.arange(len(e)) if mut == "class_id_counts_dropped" else np.cumsum(keep) - 1)[keep]
    e, length = e[keep], length[keep]
    kl = np.zeros(len(e), KEYLINE_DT)
    for a, b in (("startPointX", 0), ("startPointY", 1), ("endPointX", 2), ("endPointY", 3)):
        kl[a] = e[:, b]
        kl[a.replace("startPoint", "sPointInOctave").replace("endPoint", "ePointInOctave")] = e[:, b]
    kl["lineLength"] = length
    r = np.rint(e.astype(np.float64)).astype(np.int64)                      # Point2f -> Point: round half to even
    kl["numOfPixels"] = np.maximum(np.abs(r[:, 2] - r[:, 0]), np.abs(r[:, 3] - r[:, 1])) + 1
    dy, dx = e[:, 3] - e[:, 1], e[:, 2] - e[:, 0]
    if mut == "angle_swapped_arguments":
        dy, dx = dx, dy
    kl["angle"] = [m.atan2f(float(a), float(b)) for a, b in zip(dy, dx)]
    kl["class_id"] = ids
    kl["size"] = (e[:, 2] - e[:, 0]) * (e[:, 3] - e[:, 1])
    kl["response"] = length / F32(min(W, H) if mut == "response_min" else max(W, H))
    kl["pt_x"] = (e[:, 2] + e[:, 0]) / F32(2)
    kl["pt_y"] = (e[:, 3] + e[:, 1]) / F32(2)
    if nfeatures != 0 and len(kl) > nfeatures:
        kl = kl[np.argsort(-kl["response"].astype(np.float64), kind="stable")][:nfeatures].copy()
        if mut != "class_id_kept_after_cut":
            kl["class_id"] = np.arange(nfeatures)
    return kl


def restate_lbd(kl, dxp, dyp, mut=None, cover=None):
    """computeLBD and binaryConversion on the planes dxp, dyp (H, W) int16, float32 operation by operation, with cosf / sinf:
    (fdesc (n, 72) f4, desc (n, 32) u8).  `cover`, a dict, receives which of the four coordinate clamps fired (left, right, top, bottom)."""
    m = _m()
    n = len(kl)
    H, W = dxp.shape
    if n == 0:
        return np.zeros((0, 72), np.float32), np.zeros((0, 32), np.uint8)
    gL, gG = _weights(mut == "weights_real_division")
    f = lambda a: np.asarray(a, np.float32)
    length = kl["numOfPixels"].astype(np.int16).astype(np.int64)
    basis = kl["lineLength"].astype(np.int16).astype(np.int64) if mut == "half_width_from_length" else length
    half_w = f(np.trunc((basis - 1) / 2.0))
    half_h = F32(31)
    mx = f(0.5 * (kl["sPointInOctaveX"].astype(np.float64) + kl["ePointInOctaveX"].astype(np.float64)))
    my = f(0.5 * (kl["sPointInOctaveY"].astype(np.float64) + kl["ePointInOctaveY"].astype(np.float64)))
    dL0 = f([m.cosf(float(a)) for a in kl["angle"]])
    dL1 = f([m.sinf(float(a)) for a in kl["angle"]])
    dO0, dO1 = (dL1, -dL0) if mut == "d_o_sign" else (-dL1, dL0)
    x0 = (-dL0 * half_w + dL1 * half_h) + mx
    y0 = (-dL1 * half_w - dL0 * half_h) + my
    X0, Y0 = np.zeros((n, 63), np.float32), np.zeros((n, 63), np.float32)
    for h in range(63):
        X0[:, h], Y0[:, h] = x0, y0
        x0, y0 = x0 - dL1, y0 + dL0
    X, Y = X0.copy(), Y0.copy()
    pL, nL, pO, nO = (np.zeros((n, 63), np.float32) for _ in range(4))
    rnd = (lambda v: np.rint(v.astype(np.float64)).astype(np.int64)) if mut == "round_half_even" else _round_half_away
    a0, a1, b0, b1 = dL0[:, None], dL1[:, None], dO0[:, None], dO1[:, None]
    zero = F32(0)
    for w in range(int(length.max())):
        live = (w < length)[:, None]
        xr, yr = rnd(X).astype(np.int16).astype(np.int64), rnd(Y).astype(np.int16).astype(np.int64)
        if cover is not None:
            for k, hit in (("left", xr < 0), ("right", xr > W - 1), ("top", yr < 0), ("bottom", yr > H - 1)):
                cover[k] = cover.get(k, 0) + int((hit & live).sum())
        xc, yc = np.clip(xr, 0, W - 1), np.clip(yr, 0, H - 1)
        gx, gy = dxp[yc, xc].astype(np.float32), dyp[yc, xc].astype(np.float32)
        gDL = gx * a0 + gy * a1
        gDO = gx * b0 + gy * b1
        pL = pL + np.where(live & (gDL > 0), gDL, zero)
        nL = nL - np.where(live & ~(gDL > 0), gDL, zero)
        pO = pO + np.where(live & (gDO > 0), gDO, zero)
        nO = nO - np.where(live & ~(gDO > 0), gDO, zero)
        X, Y = X + a0, Y + a1
    G = gG[None, :]
    pL, nL, pO, nO = G * pL, G * nL, G * pO, G * nO
    rows = [pL, nL, pL * pL, nL * nL, pO, nO, pO * pO, nO * nO]           # L, L, L2, L2, O, O, O2, O2
    squared = [False, False, True, True, False, False, True, True]
    band = [np.zeros((n, 9), np.float32) for _ in range(8)]
    for h in range(63):
        b = h // 7
        for bb, c in ((b, gL[h % 7 + 7]), (b - 1, gL[h % 7 + 14]), (b + 1, gL[h % 7])):
            if 0 <= bb < 9:
                for k in range(8):
                    band[k][:, bb] = band[k][:, bb] + ((c * c) * rows[k][:, h] if squared[k] else c * rows[k][:, h])
    des = np.zeros((n, 72), np.float32)
    inv2, inv3 = F32(1.0 / 14.0), F32(1.0 / 21.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(9):
            inv = inv2 if b in (0, 8) else inv3
            for j, (mean_k, sq_k) in enumerate(((0, 2), (1, 3), (4, 6), (5, 7))):
                t = band[mean_k][:, b] * inv
                des[:, 8 * b + j] = t
                des[:, 8 * b + 4 + j] = np.sqrt(band[sq_k][:, b] * inv - t * t)
        tm, ts = np.zeros(n, np.float32), np.zeros(n, np.float32)
        for i in range(0, 72, 8):
            for j in range(4):
                tm = tm + des[:, i + j] * des[:, i + j]
            for j in range(4, 8):
                ts = ts + des[:, i + j] * des[:, i + j]
        tm, ts = F32(1) / np.sqrt(tm), F32(1) / np.sqrt(ts)
        for i in range(0, 72, 8):
            des[:, i:i + 4] = des[:, i:i + 4] * tm[:, None]
            des[:, i + 4:i + 8] = des[:, i + 4:i + 8] * ts[:, None]
        des = np.where(des.astype(np.float64) > 0.4, F32(0.4), des).astype(np.float32)
        t = np.zeros(n, np.float32)
        for i in range(72):
            t = t + des[:, i] * des[:, i]
        des = des * (F32(1) / np.sqrt(t))[:, None]
    pairs = list(LBD_COMBINATIONS)
    if mut == "band_pair":
        pairs[5] = (0, 7)
    desc = np.zeros((n, 32), np.uint8)
    for c, (i, j) in enumerate(pairs):
        bits = des[:, 8 * i:8 * i + 8] > des[:, 8 * j:8 * j + 8]
        desc[:, c] = (bits * (1 << np.arange(8))).sum(axis=1)
    return des, desc


# ------------------------------------------------------------------------------------------------------------ comparison
def compare_with_ties(case, fix, kl, desc, fdesc=None, with_desc=True):
    """Differences between a result (kl, desc, fdesc) and the fixture under the tie rule: rows outside tie groups must match in place;
    in a TIE_INSIDE case the rows of a kept group are compared as a multiset without class_id; in a TIE_STRADDLE case the rows from the
    straddling group's first rank on are counted, not asserted.  with_desc=False leaves the descriptors out.  Returns (list of difference messages, rows that differ inside kept
    tie groups, rows that differ from the straddling group on)."""
    msgs = []
    n = len(fix["kl"])
    if len(kl) != n or len(desc) != len(fix["desc"]):
        return ["count: %d key lines / %d descriptors, fixture %d / %d" % (len(kl), len(desc), n, len(fix["desc"]))], 0, 0
    inside, straddle, _ = classify_ties(case, fix) if case.name in TIE_INSIDE + TIE_STRADDLE else ([], [], [])
    free = np.ones(n, bool)
    for _, rank, size in inside:
        free[rank:rank + size] = False
    tail = min((g[1] for g in straddle), default=n)
    free[tail:] = False
    has_desc = with_desc and len(desc) == n

    def row_bytes(K, D, Fd, i, with_id):
        fields = KEYLINE_DT.names if with_id else FIELDS_WITHOUT_CLASS_ID
        b = b"".join(K[f][i:i + 1].tobytes() for f in fields)
        if has_desc:
            b += D[i].tobytes()
            if Fd is not None:
                b += Fd[i].tobytes()
        return b

    for f in KEYLINE_DT.names:
        d = np.flatnonzero((kl[f].view(np.int32) != fix["kl"][f].view(np.int32)) & free)
        if d.size:
            msgs.append("kl.%s differs at rows %s (%d rows)" % (f, d[:5].tolist(), d.size))
    if has_desc:
        d = np.flatnonzero((desc != fix["desc"]).any(axis=1) & free)
        if d.size:
            msgs.append("descriptor bytes differ at rows %s (%d rows)" % (d[:5].tolist(), d.size))
        if fdesc is not None:
            d = np.flatnonzero((fdesc.view(np.int32) != fix["fdesc"].view(np.int32)).any(axis=1) & free)
            if d.size:
                msgs.append("72-float descriptors differ at rows %s (%d rows)" % (d[:5].tolist(), d.size))
    fdf = None if fdesc is None else fix["fdesc"]
    moved_inside = 0
    for _, rank, size in inside:
        idx = range(rank, min(rank + size, tail))
        a = sorted(row_bytes(kl, desc, fdesc, i, False) for i in idx)
        b = sorted(row_bytes(fix["kl"], fix["desc"], fdf, i, False) for i in idx)
        if a != b:
            msgs.append("tie group at rank %d (%d rows): not the same multiset of rows" % (rank, size))
        d = np.flatnonzero(kl["class_id"][rank:rank + size] != fix["kl"]["class_id"][rank:rank + size])
        if d.size:
            msgs.append("tie group at rank %d: class_id differs" % rank)
        moved_inside += sum(row_bytes(kl, desc, fdesc, i, True) != row_bytes(fix["kl"], fix["desc"], fdf, i, True) for i in idx)
    moved_straddle = sum(row_bytes(kl, desc, fdesc, i, True) != row_bytes(fix["kl"], fix["desc"], fdf, i, True) for i in range(tail, n))
    return msgs, moved_inside, moved_straddle
