"""The front of the oracle's LSD — the scaled image, the gradient norm, which pixels have a level-line angle, the angle, the largest
norm (oracle/line_oracle.hpp lsdDetect, oracle/ocv_prims.hpp gaussianBlur64f / resizeLinear64f) — against a restatement that saw
neither the oracle nor the kernels (tests/helpers_lsd_front.py: numpy in long double), plane by plane and
pixel by pixel, at the sizes where the strip and chunk logic of csrc/lsd_f64.hip has edges (helpers_lsd_front.cases(): the GPU
counterpart, tests/test_lsd_front_planes_gpu.py, compares the kernels' planes with this oracle byte for byte at the same sizes).

Measured over the whole case list at chunk 64 (30 cases of 3 images, 0.46 M scaled pixels; x87 long doubles): the largest
|oracle - restatement| on the scaled and norm planes and the largest norm is 1.7e-13 (1.68e-13; helpers_lsd_front.MEASURED_MAX; the
comparison test prints what it finds).  The bound T is 16 times that, 2.7e-12: the factor covers the spread of differently ordered
sums on images outside the list, and T stays below 1e-9 — the nearest real error, the resize with its position kept in double, is at 5e-4.  No pixel of the list
has a norm within 1e-9 of rho, so none is left out of the defined / undefined comparison; a seed that produced one would be changed,
not the rule.

The comparison must also reject five wrong statements of the pass (helpers_lsd_front.MUTANTS), each on at least one case."""
import numpy as np
import pytest

import helpers_lsd_front as H


@pytest.fixture(scope="module")
def agreement(oracle):
    """{case: [(what is wrong, largest difference, pixels left out)] per image}: the oracle against the restatement."""
    out = {}
    for case in H.cases():
        out[case] = [H.compare(f, o.scaled, o.norm, o.angle, o.max_grad, what="%s image %d:" % (case.name, i))
                     for i, (_, o, f) in enumerate(H.references(oracle, case))]
    return out


def mutant_caught(oracle, case, **mutant):
    """What the comparison finds wrong, over the case's images, when the restatement is stated wrongly."""
    bad = []
    for i, (img, o, _) in enumerate(H.references(oracle, case)):
        bad += H.compare(H.front(img, case.scale, case.sigma_scale, **mutant), o.scaled, o.norm, o.angle, o.max_grad,
                         what="%s image %d:" % (case.name, i))[0]
    return bad


def case_named(name):
    (c,) = [c for c in H.cases() if c.name == name]
    return c


def test_case_list_has_the_edges_it_claims():
    cs = H.cases()
    assert len(cs) == 16 + 2 + 10 + 2
    at12 = [c for c in cs[:16]]
    assert sorted({H.scaled_len(c.w, 1.2) for c in at12}) == [64, 65, 90, 128]
    assert sorted({c.h for c in at12}) == [27, 53, 54, 164]
    assert sorted({H.scaled_len(c.h, 1.2) for c in at12}) == [32, 64, 65, 197] and 197 >= 3 * 64 + 5
    assert [(c.scale, H.scaled_len(c.h, c.scale)) for c in cs[16:18]] == [(1.5, 66), (2.0, 66)]      # (no height scales to 65 there: the next)
    assert [H.gauss_taps(c.sigma_scale, c.scale)[1] for c in cs[-2:]] == [1, 2] and H.gauss_taps(0.6, 1.2)[1] == 3


def test_oracle_planes_agree_with_the_restatement(agreement):
    worst, left_out, pixels = 0.0, 0, 0
    for case, per_image in agreement.items():
        for bad, w, close in per_image:
            assert not bad, "\n".join(bad)
            worst, left_out = max(worst, w), left_out + close
        pixels += 3 * H.scaled_len(case.w, case.scale) * H.scaled_len(case.h, case.scale)
    print("largest |oracle - restatement| over %d scaled pixels: %.3g (T = %.3g); pixels within %g of rho: %d" % (
        pixels, worst, H.T, H.RHO_MARGIN, left_out))
    assert left_out == 0, "a pixel of the case list is within %g of rho: change the seed, not the rule" % H.RHO_MARGIN


def test_polynomial_angle_stays_near_the_true_arctangent():
    rng = np.random.default_rng(3)
    gx, gy = rng.normal(0, 40, 200000).astype(np.float32), rng.normal(0, 40, 200000).astype(np.float32)
    d = H.angle_distance(H.fast_atan2_deg(gx, gy), H.true_atan2_deg(gx, gy))
    print("fastAtan2 against the true arctangent: %.4f degrees at most" % d.max())
    assert d.max() < 0.02
    # the axes and the diagonals, by their known values
    assert [H.fast_atan2_deg(y, x) for y, x in ((0, 1), (1, 0), (0, -1), (-1, 0))] == [0.0, 90.0, 180.0, 270.0]
    assert abs(H.fast_atan2_deg(1, 1) - 45.0) < 0.02 and abs(H.fast_atan2_deg(-1, -1) - 225.0) < 0.02


@pytest.mark.parametrize("name", ["75x54", "75x44 x1.5"])
def test_textbook_resize_is_rejected(oracle, agreement, name):
    """The bilinear enlargement with its position kept in double is not what OpenCV 3.x computes: off by ~5e-4 at 1.2 and 1.5."""
    bad = mutant_caught(oracle, case_named(name), resize="textbook")
    assert any("scaled plane differs" in b for b in bad), bad


def test_textbook_resize_is_exact_where_the_positions_are():
    """At scale 2.0 the positions are multiples of a quarter in either format: the built-in mutant is no mutant there."""
    s = [c for c in H.cases() if c.scale == 2.0][0]
    for n in (s.w, s.h):
        for a, b in zip(H.resize_taps(n, 2.0, "float"), H.resize_taps(n, 2.0, "textbook")):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("mutant", ["BORDER_REFLECT", "unnormalised taps", "gy with the wrong sign"])
def test_wrong_statement_is_rejected(oracle, agreement, mutant):
    bad = mutant_caught(oracle, case_named("75x54"), **H.MUTANTS[mutant])
    assert bad, "the comparison accepts the restatement with " + mutant
    print(mutant, "->", bad[0])
    expect = {"BORDER_REFLECT": "scaled plane differs", "unnormalised taps": "scaled plane differs", "gy with the wrong sign": "angle is up to"}
    assert any(expect[mutant] in b for b in bad), bad


def test_constant_image_has_no_defined_pixel(oracle):
    for img in H.constant_batch():
        o = H.oracle_front(oracle, img)
        assert np.all(o.angle == np.float32(H.NOTDEF)) and o.max_grad <= 0
        assert np.abs(o.norm).max() <= H.T and np.abs(o.scaled - 17.0).max() <= H.T
        bad, _, _ = H.compare(H.front(img), o.scaled, o.norm, o.angle, o.max_grad, what="constant:")
        assert not bad, bad


def test_vertical_step_edge(oracle):
    """Left 40, right 200: every row of the image is the same, so gy vanishes (to rounding) and the angle of every defined pixel is
    exactly fastAtan2(gx, 0) with gx > 0 — 90 degrees —, on the columns of the edge and nowhere else; along the edge, away from the
    top and bottom borders, the norm does not change."""
    img = H.step_edge()
    o = H.oracle_front(oracle, img)
    f = H.front(img)
    bad, _, _ = H.compare(f, o.scaled, o.norm, o.angle, o.max_grad, what="step edge:")
    assert not bad, bad
    defined = o.angle != np.float32(H.NOTDEF)
    cols = np.flatnonzero(defined.any(axis=0))
    assert len(cols) >= 2 and np.all(np.diff(cols) == 1), cols
    assert abs(cols.mean() - 26 * 1.2) < 2.0                                  # the edge, in scaled pixels
    assert np.all(defined[:-1, cols]), "a pixel of the edge columns has no angle"
    gx = float(np.float32(o.norm[10, cols[0]] * 2))                            # (gy = 0: norm = gx / 2)
    assert gx > 0 and H.fast_atan2_deg(gx, 0.0) == 90.0
    assert np.all(o.angle[defined] == np.float32(H.fast_atan2_deg(gx, 0.0)))
    inner = o.norm[8:-8, cols]
    assert np.abs(inner - inner[0]).max() <= H.T
    assert o.max_grad > 0 and abs(o.max_grad - o.norm[defined].max()) == 0.0


RAMP = dict(scale=2.0, sigma_scale=0.05, lsd_quant=2.0, lsd_ang_th=90.0)


def ramp_at_rho():
    """I = 4 x under a blur whose outer taps (exp(-200)) vanish against the centre in either precision, enlarged by 2 (weights 1/4 and
    3/4: exact): the scaled image is 2 x' - 1 exactly, gx = 4, gy = 0, and the norm is 2 = rho exactly (ang_th 90: sin = 1)."""
    return np.tile((4 * np.arange(40)).astype(np.uint8), (12, 1))


def test_norm_equal_to_rho_is_not_defined(oracle):
    """`norm <= rho` has no angle.  The only comparison in which `<` for `<=` shows is a norm that EQUALS rho; the defined / undefined
    comparison leaves such pixels out by its rule, so here the largest norm (none) and the known answer carry it."""
    img = ramp_at_rho()
    rho = H.lsd_rho(2.0, 90.0)
    assert rho == 2.0
    o = H.oracle_front(oracle, img, **RAMP)
    f = H.front(img, RAMP["scale"], RAMP["sigma_scale"], rho=rho)
    assert np.all(f.norm[:-1, 2:-3] == 2.0) and np.all(o.norm[:-1, 2:-3] == 2.0), "the ramp was meant to put the norm on rho exactly"
    assert not f.defined.any() and f.max_grad is None
    assert np.all(o.angle == np.float32(H.NOTDEF)) and o.max_grad <= 0, "the oracle gives a pixel with norm == rho an angle"
    assert not H.compare(f, o.scaled, o.norm, o.angle, o.max_grad, what="ramp:")[0]
    # the wrong statement: caught by the largest norm
    m = H.front(img, RAMP["scale"], RAMP["sigma_scale"], rho=rho, **H.MUTANTS[">= rho defines"])
    assert m.defined.any()
    bad = H.compare(m, o.scaled, o.norm, o.angle, o.max_grad, what="ramp, >= rho defines:")[0]
    assert any("largest norm" in b for b in bad), bad
