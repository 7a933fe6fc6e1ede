"""The planes each form of the LSD front pass writes (csrc/lsd_f64.hip: the three kernels k_lsd_blur64 -> k_lsd_resize64 ->
k_lsd_grad64, the tiled k_lsd_front64, the streaming k_lsd_front64s — the default product path), read back by
pli_selftest_front_planes and compared with something that does not call the shared rules of that file:

  the oracle, byte for byte in the true columns x < dw: the angle, the double norm plane, the largest norm per image, {cos, sin}
    (oracle/pyoracle.lsd_pixel_trig: what the oracle's grower adds for an accepted pixel, in both trig modes), the scaled plane of the
    three kernels;
  exact values where there is no angle: the last row and column, the pad columns dw <= x < dp and the pixels with norm <= rho hold
    angle -1024 and cold = (-1024, 0); pad columns and the last row and column hold norm 0, a pixel with norm <= rho keeps its norm;
    the owner plane holds 0x7FFFFFFF twice; no word of a written plane is left at the 0xA5 fill;
  the owner / norm word: tx_unclaimed_norm_word of the oracle's norm with packW, 0 without;
  the restatement of tests/helpers_lsd_front.py directly, without the oracle: norm within T, defined / undefined identical, the angle
    within 1e-3 degrees of the polynomial and 0.3 degrees of the true arctangent (tests/test_independent_lsd_front.py has the bounds).

tests/test_front_stream_gpu.py shows that the forms write the same words; they share the rule code, so a wrong rule is wrong three
times there.  Here a wrong rule shows with its plane and pixel.  The cases are helpers_lsd_front.cases() at the chunk height the
library reports: every form that applies to a case runs it, with packW off and on, writing the hot / cold planes and the 16-byte
records + owner plane, in a context with PLI_PARITY_TRIG_F32_LSD clear and one with it set.

The tiny sizes (down to 1 x 1) were admitted after reading the index arithmetic: the three kernels guard every store by x < W / WP,
y < H and read through reflect101 (any length) and clamped resize taps; the tiled form runs where frontTiledFits bounds its source
window (cw <= 64, ch <= 20, so tw <= 70 < 72 and th <= 26) and takes the looped reflect101 path when sw <= 6 or sh <= 6; the streaming
form runs only where frontStreamFits (radius 3, sw > 6, sh > 6: rows and columns -3 .. n + 2 reflect once into the image) — 7 x 7 is the
first such size, and the library must refuse the form below it."""
import numpy as np
import pytest

import helpers_lsd_front as H

pytestmark = pytest.mark.gpu

NOTDEF32 = np.float32(H.NOTDEF)
FILL32, FILL64 = np.uint32(0xA5A5A5A5), np.uint64(0xA5A5A5A5A5A5A5A5)
FORMS = {0: "three kernels", 1: "tiled", 2: "streaming"}
CASE_IDS = [c.name for c in H.cases()]


@pytest.fixture(scope="module")
def contexts():
    """Frontend contexts by (lsd_sigma_scale, PLI_PARITY_TRIG_F32_LSD), made on first use."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    made = {}

    def get(sigma_scale=0.6, trig_f32=False, **config):
        key = (sigma_scale, trig_f32, tuple(sorted(config.items())))
        if key not in made:
            flags = capi.default_config(128, 128).parity_flags & ~capi.PARITY_TRIG_F32_LSD
            made[key] = Frontend(capi.default_config(128, 128, lsd_sigma_scale=sigma_scale,
                                                     parity_flags=flags | (capi.PARITY_TRIG_F32_LSD if trig_f32 else 0), **config))
        return made[key]
    return get


@pytest.fixture(scope="module")
def chunk(contexts):
    return contexts().selftest_front_stream(np.zeros((1, 16, 16), np.uint8))["chunk"]


def forms_of(case):
    """The forms that apply to a case of the list, stated here and not asked of the library: the three kernels always; the tiled form
    at every size of the list (no source window of a 64 x 16 tile exceeds 64 x 20 at a scale above 1); the streaming form with blur
    radius 3 and more than 6 source rows and columns."""
    return [0, 1] + ([2] if H.gauss_taps(case.sigma_scale, case.scale)[1] == 3 and case.w > 6 and case.h > 6 else [])


def refused(fe, imgs, form, scale):
    from pli_slam_amd import capi
    with pytest.raises(capi.PliError) as e:
        fe.selftest_front_planes(imgs, form, scale=scale)
    return e.value.status == -1                               # PLI_ERR_INVALID


def first(mask):
    i, y, x = np.argwhere(mask)[0]
    return "%d pixels, first (image %d, x %d, y %d)" % (int(mask.sum()), i, x, y)


def check_planes(r, refs, trig, pack_w, records, form, what, rho=None, on_rho=False):
    """One read-back `r` of a form against the oracle planes and the restatement of every image (refs: [(image, OraclePlanes, Front)])."""
    from oracle import pyoracle as po
    n, dw = len(refs), r["dw"]
    dh, dp = r["norm"].shape[1:]
    assert dp == (dw + 15) // 16 * 16 and (dh, dw) == refs[0][1].angle.shape, what
    o_scaled, o_norm, o_angle = (np.stack([o[k] for _, o, _ in refs]) for k in range(3))
    o_max = np.array([o.max_grad for _, o, _ in refs])
    if records:
        ang, cs, sn = (np.ascontiguousarray(r["rec"][..., k]) for k in range(3))
        word = np.ascontiguousarray(r["rec"][..., 3]).view(np.uint32)
    else:
        ang = np.ascontiguousarray(r["hot"][..., 0]).view(np.float32)
        word = np.ascontiguousarray(r["hot"][..., 1]).view(np.uint32)
        cs, sn = r["cold"][..., 0], r["cold"][..., 1]
    norm = r["norm"]
    # --- nothing left at the fill
    for name, plane in (("angle", ang), ("cos", cs), ("sin", sn)):
        assert not (np.ascontiguousarray(plane).view(np.uint32) == FILL32).any(), "%s: %s words left unwritten" % (what, name)
    assert not (norm.view(np.uint64) == FILL64).any(), "%s: norm words left unwritten: %s" % (what, first(norm.view(np.uint64) == FILL64))
    assert not (r["max_bits"] == FILL64).any(), what
    # --- byte-equal with the oracle in the true columns
    t = np.s_[:, :, :dw]
    bits32, bits64 = (lambda a: np.ascontiguousarray(a).view(np.uint32)), (lambda a: np.ascontiguousarray(a).view(np.uint64))
    if form == 0:                                             # (first: what is wrong in the scaled plane is wrong in every plane after it)
        d = bits64(r["scaled"]) != bits64(o_scaled)
        assert not d.any(), "%s: scaled plane differs from the oracle: %s (largest difference %.3g)" % (
            what, first(d), np.abs(r["scaled"] - o_scaled).max())
    d = bits32(ang[t]) != bits32(o_angle)
    assert not d.any(), "%s: angle plane differs from the oracle: %s" % (what, first(d))
    d = bits64(norm[t]) != bits64(o_norm)
    assert not d.any(), "%s: norm plane differs from the oracle: %s (largest difference %.3g)" % (what, first(d), np.abs(norm[t] - o_norm).max())
    want_max = np.where(o_max > 0, o_max, 0.0).view(np.uint64)
    assert np.array_equal(r["max_bits"], want_max), "%s: largest norm per image %s, oracle %s" % (what, r["max_bits"].view(np.float64), o_max)
    defined = o_angle != NOTDEF32
    trig_want = po.lsd_pixel_trig(o_angle, trig)
    for name, plane, k in (("cos", cs, 0), ("sin", sn, 1)):
        d = (bits32(plane[t]) != bits32(trig_want[..., k])) & defined
        assert not d.any(), "%s: %s differs from the oracle's (trig_f32 %d): %s" % (what, name, trig, first(d))
    # --- exact values where there is no angle
    undef = np.ones((n, dh, dp), bool)
    undef[t] = ~defined
    assert undef[:, -1, :].all() and undef[:, :, dw - 1:].all()              # (the oracle: last row and column; here: the pad too)
    rho = H.lsd_rho() if rho is None else rho
    assert np.array_equal(undef[t][:, :-1, :-1], (o_norm <= rho)[:, :-1, :-1])
    assert np.all(ang[undef] == NOTDEF32), "%s: a pixel without an angle does not hold -1024" % what
    if records:
        assert np.all(cs[undef] == 0) and np.all(sn[undef] == 0), "%s: the record of a pixel without an angle" % what
        assert np.all(r["own"].view(np.uint32) == 0x7FFFFFFF) and r["own"].shape == (n, dh, dp, 2), "%s: owner plane" % what
    else:
        assert np.all(cs[undef] == NOTDEF32) and np.all(sn[undef] == 0), "%s: cold plane of a pixel without an angle is not (-1024, 0)" % what
    assert np.all(norm[:, -1, :] == 0) and np.all(norm[:, :, dw - 1:] == 0), "%s: norm of the last row / column / pad columns is not 0" % what
    # --- the owner / norm word
    full_norm = np.zeros((n, dh, dp))
    full_norm[t] = o_norm
    want_word = H.unclaimed_norm_word(full_norm) if pack_w else np.zeros((n, dh, dp), np.uint32)
    d = word != want_word
    assert not d.any(), "%s: owner / norm word: %s" % (what, first(d))
    # --- against the restatement, without the oracle
    for i, (_, _, f) in enumerate(refs):
        got_max = r["max_bits"][i:i + 1].view(np.float64)[0]
        bad, _, left_out = H.compare(f, r["scaled"][i] if form == 0 else None, norm[i, :, :dw], ang[i, :, :dw], got_max,
                                     what="%s image %d:" % (what, i))
        assert not bad, "\n".join(bad)
        assert on_rho or left_out == 0, "%s: a pixel within %g of rho" % (what, H.RHO_MARGIN)


def run_case(contexts, case, refs, forms, rho=None, on_rho=False, **config):
    ran = 0
    for trig in (False, True):
        fe = contexts(case.sigma_scale, trig, **config)
        imgs = np.stack([img for img, _, _ in refs])
        for form in forms:
            for records in (False, True):
                for pack_w in (False, True):
                    what = "%s, %s, trig_f32 %d, %s, packW %d" % (case.name, FORMS[form], trig, "records" if records else "hot/cold", pack_w)
                    r = fe.selftest_front_planes(imgs, form, scale=case.scale, pack_w=pack_w, records=records)
                    check_planes(r, refs, trig, pack_w, records, form, what, rho=rho, on_rho=on_rho)
                    ran += 1
    print("%s: %d read-backs of %d images agree (forms %s)" % (case.name, ran, len(refs), ", ".join(FORMS[f] for f in forms)))


@pytest.mark.parametrize("k", range(len(CASE_IDS)), ids=CASE_IDS)
def test_front_planes_against_oracle_and_restatement(contexts, chunk, oracle, k):
    case = H.cases(chunk)[k]
    refs = H.references(oracle, case)
    forms = forms_of(case)
    run_case(contexts, case, refs, forms)
    imgs = np.stack([img for img, _, _ in refs])
    for form in set(FORMS) - set(forms):
        assert refused(contexts(case.sigma_scale), imgs, form, case.scale), "%s: the %s form does not apply and was not refused" % (
            case.name, FORMS[form])


def test_case_list_reaches_every_form_and_both_tile_paths(chunk):
    cs = H.cases(chunk)
    assert {f for c in cs for f in forms_of(c)} == {0, 1, 2}
    assert [c for c in cs if c.name == "tiny 7x7" and 2 in forms_of(c)] and [c for c in cs if c.name == "tiny 7x6" and 2 not in forms_of(c)]
    assert sorted(H.gauss_taps(c.sigma_scale, c.scale)[1] for c in cs if c.sigma_scale != 0.6) == [1, 2]      # lsd_front64_tile<0>
    assert max(H.scaled_len(c.w, c.scale) for c in cs if c.scale == 1.2) == 128 and max(H.scaled_len(c.w, c.scale) for c in cs) == 150
    assert max(H.scaled_len(c.h, c.scale) for c in cs) >= 3 * chunk + 5


def test_forms_that_do_not_apply_are_refused(contexts):
    imgs = np.stack([H.noise(1, 6, 6), H.checker(6, 6), np.full((6, 6), 200, np.uint8)])
    assert refused(contexts(), imgs, 2, 1.2), "streaming at 6 x 6"
    fe = contexts()
    assert fe.selftest_front_planes(imgs, 1)["norm"].shape == (3, 7, 16)
    imgs = H.batch(H.Case("", 75, 54, 1.2, 0.25))
    assert refused(contexts(0.25), imgs, 2, 1.2), "streaming with blur radius 1"
    assert refused(contexts(), imgs, 3, 1.2) and refused(contexts(), imgs, -1, 1.2)


def test_constant_image_has_no_defined_pixel(contexts, oracle):
    case = H.Case("constant", 53, 40, 1.2, 0.6)
    refs = [(img, H.oracle_front(oracle, img), H.front(img)) for img in H.constant_batch()]
    assert all(o.max_grad <= 0 and f.max_grad is None for _, o, f in refs)
    run_case(contexts, case, refs, [0, 1, 2])


def test_vertical_step_edge(contexts, oracle):
    img = H.step_edge()
    case = H.Case("step edge", img.shape[1], img.shape[0], 1.2, 0.6)
    across = np.full(img.shape, 40, np.uint8)
    across[20:] = 200                                         # (the same edge the other way round, and a horizontal one)
    refs = [(im, H.oracle_front(oracle, im), H.front(im)) for im in (img, img[:, ::-1].copy(), across)]
    run_case(contexts, case, refs, [0, 1, 2])
    r = contexts().selftest_front_planes(img[None], 2)
    ang = np.ascontiguousarray(r["hot"][0, :, :r["dw"], 0]).view(np.float32)
    assert (ang != NOTDEF32).any() and np.all(ang[ang != NOTDEF32] == np.float32(90.0))      # fastAtan2(gx, 0), gx > 0


def test_norm_equal_to_rho_is_not_defined(contexts, oracle):
    """`norm <= rho` has no angle: a ramp whose norm is exactly rho (tests/test_independent_lsd_front.py ramp_at_rho) has no defined
    pixel and no largest norm, in the forms that apply at blur radius 1."""
    from test_independent_lsd_front import RAMP, ramp_at_rho
    img = ramp_at_rho()
    rho = H.lsd_rho(RAMP["lsd_quant"], RAMP["lsd_ang_th"])
    case = H.Case("ramp at rho", img.shape[1], img.shape[0], RAMP["scale"], RAMP["sigma_scale"])
    refs = [(im, H.oracle_front(oracle, im, **RAMP), H.front(im, case.scale, case.sigma_scale, rho=rho)) for im in (img, img[:, ::-1].copy(), img)]
    assert all(np.all(o.norm[:-1, 2:-3] == rho) and o.max_grad <= 0 for _, o, _ in refs)
    run_case(contexts, case, refs, [0, 1], rho=rho, on_rho=True, lsd_quant=RAMP["lsd_quant"], lsd_ang_th=RAMP["lsd_ang_th"])
