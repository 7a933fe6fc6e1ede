"""A second opinion for the two descriptor stages: steered rBRIEF with its intensity-centroid angle, and LBD.

tests/helpers_descriptors.py restates both from the published algorithms (not from oracle/); here its checks run on the
oracle's outputs, on synthetic scenes, constructed images and the photographs of tests/golden/real, with the trig flags
(PARITY_TRIG_F32_ORB / _LBD) both set and both clear.  test_independent_descriptors_gpu.py runs the same checks on the
kernels' own outputs.  The mutation tests prove that each check can fail: a helper with one deliberate mistake must be
caught on the same corpus.  The pins tie the pattern table and the LBD band pairs to the reference's source where that tree
is present.

The negative-variance case of LBD (sqrt of a band variance that float32 cancellation makes negative, giving NaN) is not
constructed here.  The variance is mean(c^2 R^2) - mean(c R)^2 over the band's 14 or 21 weighted row sums, non-negative by
Cauchy-Schwarz; float32 can only push it below zero when every c_k R_k of the band agrees to about 3e-4, i.e. when the row
gradient sums R follow 1 / (local weight x global weight) row by row, and the line detector would also have to return that
support region as a keyline.  An all-zero band gives 0 - 0 = 0 exactly, not NaN.  Should a NaN ever appear, the float check
fails on it (NaN is not within any bound)."""
import math
import os
import re

import numpy as np
import pytest

import helpers_descriptors as hd
from pli_slam_amd import capi, realdata, synth

REFERENCE = "/root/reference"           # the reference tree, where present (oracle/Makefile's REF)
TRIG = capi.PARITY_TRIG_F32_ORB | capi.PARITY_TRIG_F32_LBD


def oracle_cases(po, img, flags, **over):
    """Runs the oracle on one image; returns (orb level cases, lbd case) in the helper's terms."""
    H, W = img.shape
    cfg = capi.default_config(W, H, **over)
    cfg.parity_flags = (cfg.parity_flags & ~TRIG) | flags
    fr = po.Frame(po.Config.from_buffer_copy(bytes(cfg)))
    n, kp, desc = fr.orb_extract(0, img)
    trig = "cosf" if flags & capi.PARITY_TRIG_F32_ORB else "cr"
    orb, base = [], 0
    for l in range(cfg.orb_nlevels):
        pts = fr.level_points(0, l, True)
        m = len(pts)
        if m:
            k = kp[base:base + m]
            assert (k["octave"] == l).all()
            orb.append(dict(level=fr.pyramid(0, l), blur=fr.pyramid(0, l, True), lx=pts[:, 0] + 16, ly=pts[:, 1] + 16,
                            angle=k["angle"], desc=desc[base:base + m], trig=trig))
        base += m
    assert base == n
    m, kl, ld = fr.line_extract(0, img)
    dx, dy = fr.lbd_dxdy(0, (H, W))
    lbd = dict(dx=dx, dy=dy, keylines=kl, lbd_float=fr.lbd_float(0, m), ldesc=ld,
               trig="cosf" if flags & capi.PARITY_TRIG_F32_LBD else "cr")
    return orb, lbd


def tie_angles(trig):
    """Float32 keypoint angles whose float32 sine or cosine is exactly +-0.25, +-0.5 or +-0.75: rotated pattern points with one
    zero coordinate then land exactly on .5, so round-half-even is exercised on exact ties."""
    out = []
    for s in (0.25, 0.5, 0.75):
        base = math.degrees(math.asin(s))
        for deg in (base, 180 - base, 180 + base, 360 - base, 90 - base, 90 + base, 270 - base, 270 + base):
            a = np.float32(deg)
            cand = a + np.arange(-3000, 3001, dtype=np.float32) * np.spacing(a)
            for c in cand:
                ca, sb = hd.cos_sin_f32(np.float32(c * hd.FACTOR_PI), trig)
                if abs(float(sb)) in (0.25, 0.5, 0.75) or abs(float(ca)) in (0.25, 0.5, 0.75):
                    out.append(np.float32(c))
                    break
    return np.array(out, np.float32)


def sweep_case(po, trig):
    """Keypoints of a random image at the exact-tie angles, the axis angles and random ones, with the oracle's descriptors."""
    rng = np.random.default_rng(21)
    img = rng.integers(0, 256, (80, 80), dtype=np.uint8)
    ang = np.concatenate([tie_angles(trig), np.float32([0, 45, 90, 135, 180, 225, 270, 315]), rng.uniform(0, 360, 40)])
    ang = ang.astype(np.float32)
    x = rng.integers(20, 60, ang.size)
    y = rng.integers(20, 60, ang.size)
    desc = np.stack([po.orb_descriptor(img, int(a), int(b), float(t), trig == "cosf") for a, b, t in zip(x, y, ang)])
    return dict(level=None, blur=img, lx=x, ly=y, angle=ang, desc=desc, trig=trig)


@pytest.fixture(scope="module")
def corpus(oracle):
    po = oracle
    orb, lbd = [], []
    L, R = synth.make_stereo_pair(0, 752, 480)
    for img, flags in ((L, TRIG), (R, 0), (hd.constructed_image(), TRIG), (hd.constructed_image(), 0)):
        o, l_ = oracle_cases(po, img, flags, orb_nfeatures=1200, lsd_nfeatures=100)
        orb += o; lbd.append(l_)
    ph = realdata.photos()
    for i, name in enumerate(sorted(ph)):
        o, l_ = oracle_cases(po, ph[name], TRIG if i % 2 else 0, orb_nfeatures=1000, lsd_nfeatures=60)
        orb += o; lbd.append(l_)
    o, l_ = oracle_cases(po, L, capi.PARITY_TRIG_F32_ORB, orb_nfeatures=800, lsd_nfeatures=60, orb_scale_factor=1.5,
                         orb_nlevels=5)
    orb += o; lbd.append(l_)
    orb += [sweep_case(po, "cosf"), sweep_case(po, "cr")]
    return orb, lbd


def run_orb(po, cases, **mutation):
    fails, tot = [], dict(n=0, disagree=0, near_ties=0, flat=0)
    for c in cases:
        if c["level"] is None:               # angle sweep: the descriptor only
            b32, b64, mg = hd.steered_brief(c["blur"], c["lx"], c["ly"], c["angle"], c["trig"], **mutation)
            bad = (hd.pack_bits(b32) != c["desc"]).any(1)
            if bad.any():
                fails.append("sweep (%s): %d keypoints differ" % (c["trig"], int(bad.sum())))
            dis = b32 != b64
            if (mg[dis] >= hd.TIE_MARGIN).any():
                fails.append("sweep: float64 bits differ away from a tie")
            tot["disagree"] += int(dis.sum()); tot["near_ties"] += int((mg < hd.TIE_MARGIN).sum()); tot["n"] += len(c["lx"])
            continue
        r = hd.check_orb_level(c["level"], c["blur"], c["lx"], c["ly"], c["angle"], c["desc"], c["trig"], po.fast_atan2,
                               **mutation)
        fails += r["fail"]
        for k in tot:
            tot[k] += r[k]
    return fails, tot


def run_lbd(cases, **mutation):
    fails, und, n, worst = [], 0, 0, 0.0
    for c in cases:
        r = hd.check_lbd(c["dx"], c["dy"], c["keylines"], c["lbd_float"], c["ldesc"], c["trig"], **mutation)
        fails += r["fail"]; und += r["undecided"]; n += r["n"]; worst = max(worst, r["worst"])
    return fails, dict(n=n, undecided=und, worst=worst)


def test_umax_is_the_disk_the_oracle_uses(oracle):
    from oracle import pyoracle as po
    fr = po.Frame(po.default_config(752, 480))
    assert hd.umax_table().tolist() == fr.umax().tolist()
    u, v = hd.disk_offsets()
    assert set(zip(u.tolist(), v.tolist())) == set(zip(v.tolist(), u.tolist()))          # symmetric under transposition


def test_orb_angles_and_bits_equal_the_independent_restatement(oracle, corpus):
    fails, tot = run_orb(oracle, corpus[0])
    print("ORB: %d keypoints, %d flat patches, %d bits within %.0e px of a tie, %d float64 bits differ (all at ties)" % (
        tot["n"], tot["flat"], tot["near_ties"], hd.TIE_MARGIN, tot["disagree"]))
    assert not fails, fails[:5]
    assert tot["n"] > 10000 and tot["flat"] > 0 and tot["near_ties"] > 0


def test_lbd_floats_and_bits_equal_the_independent_restatement(corpus):
    fails, tot = run_lbd(corpus[1])
    print("LBD: %d lines, worst error %.3f of the bound, %d undecided bits" % (tot["n"], tot["worst"], tot["undecided"]))
    assert not fails, fails[:5]
    assert tot["n"] > 500


def test_tie_angles_give_exact_ties():
    for trig in ("cosf", "cr"):
        a = tie_angles(trig)
        assert len(a) >= 3 and np.float32(30) in a, (trig, a)


# ---- mutations: each deliberate mistake must be caught on the same corpus -------------------------------------------------
def test_mutation_swapped_cos_sin_is_caught(oracle, corpus):
    assert run_orb(oracle, corpus[0], swap_ab=True)[0]


def test_mutation_pattern_entry_moved_by_one_pixel_is_caught(oracle, corpus):
    P = hd.orb_pattern().copy()
    P[37, 2] += 1
    assert run_orb(oracle, corpus[0], pattern=P)[0]


def test_mutation_ties_rounded_down_is_caught(oracle, corpus):
    fails = run_orb(oracle, corpus[0], ties="down")[0]
    assert fails


def test_mutation_changed_lbd_pair_is_caught(corpus):
    C = hd.LBD_COMBINATIONS.copy()
    C[12] = (2, 6)
    assert run_lbd(corpus[1], combinations=C)[0]


def test_mutation_exchanged_gaussian_weights_is_caught(corpus):
    assert run_lbd(corpus[1], exchange_weights=True)[0]


def test_mutation_missing_clip_is_caught(corpus):
    assert run_lbd(corpus[1], clip=False)[0]


def test_mutation_std_without_mean_term_is_caught(corpus):
    assert run_lbd(corpus[1], std_mean_term=False)[0]


# ---- pins against the reference's source ------------------------------------------------------------------------------------
def _reference_source(rel):
    p = os.path.join(REFERENCE, rel)
    if not os.path.exists(p):
        pytest.skip("reference tree absent")
    return open(p).read()


def _int_table(src, decl):
    i = src.index(decl)
    j = src.index("{", i)
    body = re.sub(r"/\*.*?\*/", "", src[j:src.index("};", j)], flags=re.S)
    body = re.sub(r"//[^\n]*", "", body)
    return [int(t) for t in re.findall(r"-?\d+", body)]


def test_pin_orb_pattern_equals_reference_bit_pattern_31():
    src = _reference_source("src/ORBextractor.cc")
    ref = _int_table(src, "bit_pattern_31_[256*4]")
    assert len(ref) == 1024
    assert hd.orb_pattern().ravel().tolist() == ref


def test_pin_lbd_combinations_equal_reference():
    src = _reference_source("Thirdparty/line_descriptor/src/binary_descriptor_custom.cpp")
    ref = _int_table(src, "combinations[32][2]")
    assert len(ref) == 64
    assert hd.LBD_COMBINATIONS.ravel().tolist() == ref
