"""Corpus of the ORB extractor pin (tests/test_ref_pin_orb.py, tests/test_ref_pin_orb_gpu.py, tools/gen_orb_ref.py).

Every case is (name, image generator, extractor parameters, lapping interval); the image is generated from a seed or a short
table, never stored.  tests/golden/orb_ref/<name>.npz holds what the reference's own ORBextractor::operator() returned for it
(oracle/_ref/pli_ref_orb, built by oracle/Makefile from the reference tree under a monotone heap): the return value, the
keypoints, the descriptors and, for the cases with `pyramid`, every mvImagePyramid level.

Inputs the reference itself does not define stay out (asserted by check_contract): a level with nCols or nRows of 0 divides by
zero, and a level with nIni = round(width / height) = 0 indexes an empty vector.  With 8 levels and factor 1.2 both sides must
be >= 222 px; smaller images take fewer levels.

Dot images: an isolated pixel brighter than a flat background by d has FAST arc value d, so it is a corner at threshold t iff
d > t, with score d - 1.  A dot table is therefore a constructed level-0 candidate table through the public entry point.
Level-0 geometry used below (EDGE_THRESHOLD - 3 = 16): candidate coordinates are relative to (16, 16); the octree's root spans
[0, W - 32) x [0, H - 32); cell j covers the pixels 16 + j * wCell + 3 .. 16 + (j + 1) * wCell + 2.
"""
import collections
import os
import struct
import subprocess
import tempfile

import numpy as np

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orb_ref")
KEYPOINT_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])

Params = collections.namedtuple("Params", "W H nfeatures scale_factor nlevels ini_th min_th")
Case = collections.namedtuple("Case", "name image params lapping pyramid")


def P(W, H, nfeatures, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7):
    return Params(W, H, nfeatures, scale_factor, nlevels, ini_th, min_th)


# ---------------------------------------------------------------------------------------------------------------- images
def dot_image(W, H, background, dots):
    """Flat `background` with single pixels (x, y, value)."""
    img = np.full((H, W), background, np.uint8)
    for x, y, v in dots:
        assert 0 <= x < W and 0 <= y < H and 0 <= v <= 255
        img[y, x] = v
    return img


def noise_image(W, H, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (H, W), dtype=np.uint8)


def synth_image(W, H, seed, eye=0):
    from pli_slam_amd import synth
    return synth.make_stereo_pair(seed, W, H)[eye]


def real_crop(name, x0, y0, W, H):
    from pli_slam_amd import realdata
    img = realdata.photos()[name]
    assert y0 + H <= img.shape[0] and x0 + W <= img.shape[1]
    return np.ascontiguousarray(img[y0:y0 + H, x0:x0 + W])


def _split_line_dots():
    """240x240: root [0,208)^2 splits at 104 (pixel 120), its children at 52 / 156 (pixels 68 / 172), theirs at 26, 78, 130, 182
    (pixels 42, 94, 146, 198).  Dots ON those columns and rows (x == n1.UR.x, y == n1.BR.y go right / down), one pixel before
    them, and off them; distinct brightnesses so that no response ties."""
    lines = [42, 68, 94, 120, 146, 172, 198]
    dots, k = [], 0
    for y in lines:
        for x in lines:
            dots.append((x, y, 100 + (k * 7) % 150))
            k += 1
    for i, c in enumerate(lines):                       # one pixel before each line, between the dots on the lines
        dots.append((c - 1, 55 if i % 2 else 107, 90 + 9 * i))
        dots.append((55 if i % 2 else 107, c - 1, 95 + 9 * i))
    return dots


def _ini_boundary_dots():
    """640x240: nIni = 3, hX = 608 / 3 = 202.67; initial nodes start at (int)(hX * i) = 0, 202, 405, but a key goes to node
    (int)(x / hX): x = 202 -> node 0, 203 -> node 1, 405 -> node 1, 406 -> node 2.  Pixels 218, 219, 421, 422."""
    dots = []
    for k, y in enumerate(range(30, 211, 12)):
        for i, x in enumerate((218, 219, 421, 422)):
            dots.append((x, y + (4 if i % 2 else 0) + (0 if i < 2 else 2), 120 + 5 * k + i))
    for k, x in enumerate(range(40, 600, 23)):          # some everywhere else, so that every initial node splits
        dots.append((x, 36 + (k * 37) % 170, 90 + (k * 11) % 160))
    return dots


def _equal_maxima_dots():
    """240x240, budget 12 (per-level quotas 3, 2, 2, 1, ...): clusters of dots of EQUAL brightness that end in one final node, in
    an order in which the first in list order is not the first in raster order of the whole image."""
    dots = []
    for cx, cy in ((40, 40), (170, 50), (60, 180), (180, 170)):
        for dx, dy in ((0, 0), (9, 1), (2, 10), (11, 12), (20, 4)):
            dots.append((cx + dx, cy + dy, 200))
    return dots


def _tie_group_dots():
    """376x240, budget 300: a lattice of pairs and triples of dots: after the first passes nearly all nodes hold 2 or 3 keys, so
    the sort sees long runs of equal sizes and the quota is reached inside one."""
    dots, k = [], 0
    for y in range(28, 212, 9):
        for x in range(28, 350, 9):
            if (x // 9 + 2 * (y // 9)) % 5 != 0:
                dots.append((x + (k % 2), y + ((k // 2) % 2), 110 + (k * 13) % 140))
            k += 1
    return dots


def _threshold_dots():
    """240x240, thresholds 20 / 7, cells of 35 px from pixel 19 (cell j: 19 + 35 j .. 53 + 35 j).  Background 60.
    cell (0,0): only sub-iniTh dots (d = 8, 12, 20) -> fallback to minTh keeps them; d = 7 is no corner even at minTh
    cell (1,0): d = 21 (just a corner at iniTh) with d = 20 and 15 -> the two are dropped
    cell (2,0): d = 120 and d = 9 -> dropped;  cell (0,1): fallback again with one dot
    seams: equal dots on the two sides of the seam between cells 3|4 (pixels 158|159), of the seam between rows 3|4, and
    diagonally across the corner where four cells meet; inside ONE cell such a pair kills itself (equal) or leaves one (unequal)."""
    b = 60
    dots = [(25, 25, b + 8), (35, 30, b + 12), (45, 45, b + 20), (30, 45, b + 7),
            (60, 25, b + 21), (70, 35, b + 20), (80, 45, b + 15),
            (95, 25, b + 120), (110, 40, b + 9),
            (30, 70, b + 13),
            (158, 30, b + 50), (159, 30, b + 50),            # horizontal neighbours across a column seam: both survive
            (158, 45, b + 50), (159, 46, b + 70),            # diagonal neighbours across it
            (100, 158, b + 60), (100, 159, b + 60),          # vertical neighbours across a row seam
            (193, 193, b + 40), (194, 194, b + 40),          # diagonal across the corner of four cells
            (130, 100, b + 50), (131, 100, b + 50),          # the same pair inside one cell: neither is a strict maximum
            (130, 120, b + 50), (131, 121, b + 55)]          # unequal pair inside one cell: the brighter one stays
    return dots


def _low_threshold_dots():
    """Thresholds 5 / 2: d = 3, 4, 5 are corners only at minTh, d = 6 just at iniTh, d = 2 never."""
    b = 100
    dots = []
    for k, (x, y) in enumerate([(x, y) for y in range(26, 215, 17) for x in range(26, 215, 13)]):
        dots.append((x + k % 3, y + (k // 3) % 3, b + 2 + (k * 5) % 9))
    return dots


def _sparse_dots(W, H, n, seed, background=60, lo=30, hi=190, margin=20, step=8):
    """n dots on a jittered lattice (never closer than `step` - 2 px), seeded."""
    rng = np.random.default_rng(seed)
    cells = [(x, y) for y in range(margin, H - margin - step, step) for x in range(margin, W - margin - step, step)]
    pick = rng.choice(len(cells), size=min(n, len(cells)), replace=False)
    dots = []
    for i in sorted(pick):
        x, y = cells[i]
        dots.append((x + int(rng.integers(0, 3)), y + int(rng.integers(0, 3)), background + int(rng.integers(lo, hi))))
    return dots


# ----------------------------------------------------------------------------------------------------------------- cases
CASES = [
    # nIni = 1, budget 300
    Case("dots_split_lines_240", lambda: dot_image(240, 240, 40, _split_line_dots()), P(240, 240, 300), (0, 0), True),
    Case("dots_thresholds_seams_240", lambda: dot_image(240, 240, 60, _threshold_dots()), P(240, 240, 300), (0, 0), False),
    Case("dots_sparse_lap_some_240", lambda: dot_image(240, 240, 60, _sparse_dots(240, 240, 150, 5)), P(240, 240, 300), (90, 150), False),
    Case("noise_lap_all_240", lambda: noise_image(240, 240, 11), P(240, 240, 300), (0, 100000), False),
    Case("noise_lap_some_240", lambda: noise_image(240, 240, 12), P(240, 240, 300), (100, 140), False),
    # budget 12: quota reached in the first expansion pass, equal maxima inside the final nodes
    Case("dots_equal_maxima_240", lambda: dot_image(240, 240, 30, _equal_maxima_dots()), P(240, 240, 12), (0, 0), False),
    Case("noise_budget12_240", lambda: noise_image(240, 240, 13), P(240, 240, 12), (0, 0), False),
    # odd size, nIni = 1
    Case("real_coins_257x231", lambda: real_crop("coins", 60, 40, 257, 231), P(257, 231, 300), (0, 0), True),
    Case("noise_257x231", lambda: noise_image(257, 231, 14), P(257, 231, 300), (120, 121), False),
    Case("dots_257x231_budget12", lambda: dot_image(257, 231, 60, _sparse_dots(257, 231, 60, 6)), P(257, 231, 12), (0, 0), False),
    # nIni = 2, budget 1200 and 300
    Case("synth_left_376x240", lambda: synth_image(376, 240, 3, 0), P(376, 240, 1200), (0, 0), True),
    Case("synth_right_376x240", lambda: synth_image(376, 240, 3, 1), P(376, 240, 1200), (150, 400), False),
    Case("noise_376x240", lambda: noise_image(376, 240, 15), P(376, 240, 1200), (0, 0), False),
    Case("dots_tie_groups_376x240", lambda: dot_image(376, 240, 50, _tie_group_dots()), P(376, 240, 300), (0, 0), False),
    # nIni = 3 with a non-integer hX
    Case("dots_ini_boundary_640x240", lambda: dot_image(640, 240, 50, _ini_boundary_dots()), P(640, 240, 300), (0, 0), False),
    Case("real_brick_gravel_640x240", lambda: np.ascontiguousarray(np.hstack([real_crop("brick", 0, 100, 512, 240), real_crop("gravel", 0, 50, 128, 240)])),
         P(640, 240, 300), (200, 420), False),
    Case("noise_720x230", lambda: noise_image(720, 230, 16), P(720, 230, 1200), (0, 0), False),
    Case("dots_720x230", lambda: dot_image(720, 230, 70, _sparse_dots(720, 230, 500, 7)), P(720, 230, 1200), (300, 500), False),
    # non-default parameters
    Case("real_camera_509x501_l4_f2", lambda: real_crop("camera", 2, 5, 509, 501), P(509, 501, 300, 2.0, 4), (0, 0), False),
    Case("real_gravel_376x240_l12_f1.1", lambda: real_crop("gravel", 30, 60, 376, 240), P(376, 240, 1200, 1.1, 12), (0, 0), False),
    Case("dots_low_thresholds_240", lambda: dot_image(240, 240, 100, _low_threshold_dots()), P(240, 240, 300, 1.2, 8, 5, 2), (0, 0), False),
    Case("noise_soft_low_thresholds_240", lambda: noise_image(240, 240, 17, 100, 112), P(240, 240, 300, 1.2, 8, 5, 2), (0, 0), False),
    Case("noise_high_thresholds_240", lambda: noise_image(240, 240, 18), P(240, 240, 300, 1.2, 8, 80, 40), (0, 0), False),
    Case("real_moon_high_thresholds_240", lambda: real_crop("moon", 100, 120, 240, 240), P(240, 240, 300, 1.2, 8, 80, 40), (0, 0), False),
    # cell rows / columns skipped or under 7 px: only levels with >= 26 cells of 31 px in a direction have them (width - 32 = 781:
    # the last column starts at 775 >= 781 - 6 and is skipped, a last row of 6 px is searched by cv::FAST and returns nothing;
    # height - 32 = 871: the last row starts at 868 >= 871 - 3 and is skipped).  Two levels keep these quick.
    Case("noise_skip_column_813x240_l2", lambda: noise_image(813, 240, 19), P(813, 240, 300, 1.2, 2), (0, 0), False),
    # ... and one pixel more: the last column / row is 7 px, one column / row of pixels is searched and holds corners
    # (pixel column 794 of 814x240, pixel row 794 of 440x814; few enough dots that the octree keeps every one)
    Case("dots_7px_column_814x240_l2", lambda: dot_image(814, 240, 60, _sparse_dots(814, 240, 90, 20, step=16) +
                                                         [(794, y, 140 + y // 3) for y in range(30, 215, 23)]),
         P(814, 240, 300, 1.2, 2), (0, 0), False),
    Case("dots_7px_row_440x814_l2", lambda: dot_image(440, 814, 60, _sparse_dots(440, 814, 90, 21, step=16) +
                                                      [(x, 794, 120 + x // 4) for x in range(30, 415, 37)]),
         P(440, 814, 300, 1.2, 2), (0, 0), False),
    Case("dots_narrow_row_440x813_l2", lambda: dot_image(440, 813, 60, _sparse_dots(440, 813, 700, 8, step=16) + [(100, 792, 200), (200, 795, 210)]),
         P(440, 813, 300, 1.2, 2), (0, 0), False),
    Case("dots_skip_row_470x903_l2", lambda: dot_image(470, 903, 60, _sparse_dots(470, 903, 700, 9, step=16) + [(100, 884, 200), (200, 886, 210)]),
         P(470, 903, 300, 1.2, 2), (0, 0), False),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def level_sizes(p):
    """(w, h) per level as ComputePyramid rounds them (float32 arithmetic, ORBextractor.cc:1156-1157)."""
    out, sc = [], np.float32(1.0)
    for level in range(p.nlevels):
        if level:
            sc = np.float32(sc * np.float32(p.scale_factor))
        inv = np.float32(1.0) / sc
        out.append((int(np.rint(np.float32(p.W) * inv)), int(np.rint(np.float32(p.H) * inv))))
    return out


def check_contract(p):
    """Every level has nCols, nRows >= 1 and nIni >= 1; anything else is the reference's own undefined behaviour."""
    for w, h in level_sizes(p):
        width, height = w - 32, h - 32
        assert width >= 30 and height >= 30, ("a level without cells", p, w, h)
        nini = int(np.floor(np.float32(width) / np.float32(height) + np.float32(0.5)))
        assert nini >= 1, ("nIni == 0", p, w, h)


for _c in CASES:
    check_contract(_c.params)


def groups():
    """Cases grouped by configuration, in corpus order: [(Params, [Case, ...]), ...]."""
    g = collections.OrderedDict()
    for c in CASES:
        g.setdefault(c.params, []).append(c)
    return list(g.items())


# -------------------------------------------------------------------------------------------------------------- fixtures
def fixture_path(name):
    return os.path.join(GOLD_DIR, name + ".npz")


def load_fixture(name):
    """{"mono", "kp" (KEYPOINT_DT), "desc" (n, 32) u8, "levels": [u8 (h, w)] or None}"""
    z = np.load(fixture_path(name))
    out = {"mono": int(z["mono"]), "kp": z["kp"].view(KEYPOINT_DT).reshape(-1), "desc": z["desc"], "levels": None}
    if "nlevels" in z.files:
        out["levels"] = [z["level%d" % l] for l in range(int(z["nlevels"]))]
    return out


def save_fixture(name, res, with_levels):
    os.makedirs(GOLD_DIR, exist_ok=True)
    arrays = {"mono": np.int32(res["mono"]), "kp": res["kp"].view(np.uint8).reshape(-1, KEYPOINT_DT.itemsize), "desc": res["desc"]}
    if with_levels:
        arrays["nlevels"] = np.int32(len(res["levels"]))
        for l, a in enumerate(res["levels"]):
            arrays["level%d" % l] = a
    np.savez_compressed(fixture_path(name), **arrays)


# ------------------------------------------------------------------------------------------- the reference's own program
def run_reference(exe, case, image=None):
    """One run of oracle/_ref/pli_ref_orb (or _sysheap) as a child process; the result in load_fixture's form."""
    p = case.params
    image = case.image() if image is None else image
    assert image.shape == (p.H, p.W) and image.dtype == np.uint8
    with tempfile.TemporaryDirectory() as d:
        req, rsp = os.path.join(d, "request"), os.path.join(d, "response")
        with open(req, "wb") as f:
            f.write(struct.pack("<iiifiiiii", p.W, p.H, p.nfeatures, p.scale_factor, p.nlevels, p.ini_th, p.min_th, *case.lapping))
            f.write(np.ascontiguousarray(image).tobytes())
        subprocess.run([exe, req, rsp], check=True, timeout=120)
        raw = open(rsp, "rb").read()
    mono, n = struct.unpack_from("<ii", raw, 0)
    o = 8
    kp = np.frombuffer(raw, KEYPOINT_DT, n, o).copy()
    o += n * KEYPOINT_DT.itemsize
    desc = np.frombuffer(raw, np.uint8, n * 32, o).reshape(n, 32).copy()
    o += n * 32
    (nl,) = struct.unpack_from("<i", raw, o)
    o += 4
    levels = []
    for _ in range(nl):
        w, h = struct.unpack_from("<ii", raw, o)
        o += 8
        levels.append(np.frombuffer(raw, np.uint8, w * h, o).reshape(h, w).copy())
        o += w * h
    assert o == len(raw)
    return {"mono": mono, "kp": kp, "desc": desc, "levels": levels}


def differing_rows(a, b):
    """Rows (keypoint + descriptor) that differ between two results, out of max(len)."""
    n = min(len(a["kp"]), len(b["kp"]))
    same = (a["kp"][:n].view(np.uint8).reshape(n, -1) == b["kp"][:n].view(np.uint8).reshape(n, -1)).all(axis=1)
    same &= (a["desc"][:n] == b["desc"][:n]).all(axis=1)
    total = max(len(a["kp"]), len(b["kp"]))
    return total - int(same.sum()), total
