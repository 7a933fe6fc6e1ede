"""A restatement of the front of cv::LineSegmentDetector on the CV_64F copy of the image — Gaussian blur, bilinear enlargement, the 2x2
level-line gradient and its angle — written from SURVEY.md Appendix A (item `createLineSegmentDetector(...)->detect`, steps 1-3) and
OpenCV's documented definitions, NOT from oracle/ocv_prims.hpp, oracle/line_oracle.hpp or csrc/lsd_f64.hip: vectorised numpy in
np.longdouble (float64 where longdouble is no wider), every sum in whatever order numpy takes.

  blur      taps exp(-i^2 / 2 sigma^2), i = -r .. r, normalised; sigma = sigma_scale for scale >= 1; r = ceil(sigma sqrt(2 * 3 * ln 10));
            BORDER_REFLECT_101 for any length (length 1: index 0; otherwise reflected until inside); rows, then columns
  resize    the position of a scaled pixel as OpenCV computes it: fx = float32((dx + 0.5) * (1 / scale) - 0.5), sx = floor(fx),
            weight float32(fx - sx); left / top clamp sx = 0, w = 0; right / bottom clamp sx = n - 1, w = 0
  gradient  gx = (D - A) + (B - C), gy = (D - A) - (B - C) of the 2x2 neighbourhood A B / C D, norm = sqrt((gx^2 + gy^2) / 4), the
            pixel has a level-line angle iff norm > rho = quant / sin(pi ang_th / 180); the last row and column never have one
  angle     atan2(gx, -gy) in degrees [0, 360): the 7th-order polynomial of fastAtan2 in float32, and the true arctangent

`front(..., **mutant)` also states the pass wrongly in five ways (see MUTANTS): the CPU test asserts that its comparison rejects each.

The case list of the LSD front tests — CPU (oracle against this file) and GPU (kernels against the oracle and against this file) —
lives here too: the sizes at which the strip and chunk logic of csrc/lsd_f64.hip has edges, and the tiny sizes."""
import math
import os
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
PI = math.pi
NOTDEF = -1024.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the two angle functions (scalars or arrays; a scalar comes back as a Python float)
# ---------------------------------------------------------------------------------------------------------------------------------
def fast_atan2_deg(y, x):
    """Appendix A: fastAtan2(y, x) in degrees, float32 arithmetic."""
    f = np.float32
    p1, p3, p5, p7 = (f(0.9997878412794807 * (180 / PI)), f(-0.3258083974640975 * (180 / PI)), f(0.1555786518463281 * (180 / PI)),
                      f(-0.04432655554792128 * (180 / PI)))
    x, y = np.asarray(x, dtype=f), np.asarray(y, dtype=f)
    ax, ay = np.abs(x), np.abs(y)
    eps = f(2.220446049250313e-16)
    flat = ax >= ay                                          # c = min / (max + eps); a = (..) * c, or 90 - (..) * c
    c = np.where(flat, ay, ax) / (np.where(flat, ax, ay) + eps)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(flat, a, f(90.0) - a)
    a = np.where(x < 0, f(180.0) - a, a)
    a = np.where(y < 0, f(360.0) - a, a)
    assert a.dtype == f
    return a if a.ndim else float(a)


def true_atan2_deg(y, x):
    a = np.degrees(np.arctan2(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)))
    a = np.where(a < 0, a + 360.0, a)
    return a if a.ndim else float(a)


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "textbook resize": dict(resize="textbook"),             # the position kept in double: wrong for OpenCV 3.x
    "BORDER_REFLECT": dict(border="reflect"),               # the edge pixel repeated
    "unnormalised taps": dict(normalise=False),
    "gy with the wrong sign": dict(gy_sign=-1),
    ">= rho defines": dict(define_at_rho=True),
}

Front = namedtuple("Front", "scaled norm defined angle_fast angle_true max_grad rho")


def lsd_rho(quant=2.0, ang_th=22.5):
    return quant / math.sin(PI * ang_th / 180.0)


def scaled_len(n, scale):
    return int(round(n * scale))                              # cvRound: nearest, ties to even — as Python's round


def border_index(i, n, border="101"):
    """Source index of position i (an int array, anywhere) on an axis of length n."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    if border == "101":                                       # .. 2 1 | 0 1 2 .. n-1 | n-2 n-3 ..: period 2n - 2
        m = np.mod(i, 2 * n - 2)
        return np.where(m >= n, 2 * n - 2 - m, m)
    m = np.mod(i, 2 * n)                                      # BORDER_REFLECT .. 1 0 | 0 1 .. n-1 | n-1 n-2 ..: period 2n
    return np.where(m >= n, 2 * n - 1 - m, m)


def gauss_taps(sigma_scale, scale, normalise=True):
    sigma = sigma_scale / scale if scale < 1 else sigma_scale
    r = int(math.ceil(sigma * math.sqrt(2 * 3 * math.log(10.0))))
    i = np.arange(-r, r + 1).astype(LD)
    k = np.exp(-(i * i) / (2 * LD(sigma) * LD(sigma)))
    return (k / k.sum() if normalise else k), r


def blur(img, taps, r, border="101"):
    src = np.asarray(img).astype(LD)
    h, w = src.shape
    rows = sum(taps[j + r] * src[:, border_index(np.arange(w) + j, w, border)] for j in range(-r, r + 1))
    return sum(taps[j + r] * rows[border_index(np.arange(h) + j, h, border), :] for j in range(-r, r + 1))


def resize_taps(n, scale, resize="float"):
    """(first source index, second source index, weight of the second) of every scaled position along an axis of n source pixels."""
    d = np.arange(scaled_len(n, scale)).astype(np.float64)
    if resize == "float":
        f = ((d + 0.5) * (1.0 / scale) - 0.5).astype(np.float32)
        s = np.floor(f)
        w = (f - s.astype(np.float32)).astype(np.float32)
    else:                                                     # the textbook: the position in double
        f = (d + 0.5) / scale - 0.5
        s = np.floor(f)
        w = f - s
    s = s.astype(np.int64)
    w = w.astype(LD)
    low, high = s < 0, s >= n - 1
    s = np.where(low, 0, np.where(high, n - 1, s))
    w = np.where(low | high, LD(0), w)
    return s, np.minimum(s + 1, n - 1), w


def enlarge(b, scale, resize="float"):
    h, w = b.shape
    x0, x1, wx = resize_taps(w, scale, resize)
    y0, y1, wy = resize_taps(h, scale, resize)
    top = b[y0][:, x0] * (1 - wx) + b[y0][:, x1] * wx
    bot = b[y1][:, x0] * (1 - wx) + b[y1][:, x1] * wx
    return top * (1 - wy)[:, None] + bot * wy[:, None]


def front(img, scale=1.2, sigma_scale=0.6, rho=None, resize="float", border="101", normalise=True, gy_sign=1, define_at_rho=False):
    """The scaled image, the norm plane (0 in the last row and column), which pixels have a level-line angle, both angles (NOTDEF
    where there is none) and the largest norm among the pixels that have one (None: there is none)."""
    rho = lsd_rho() if rho is None else rho
    taps, r = gauss_taps(sigma_scale, scale, normalise)
    I = enlarge(blur(img, taps, r, border), scale, resize)
    H, W = I.shape
    norm = np.zeros((H, W), LD)
    defined = np.zeros((H, W), bool)
    a_fast = np.full((H, W), NOTDEF, np.float32)
    a_true = np.full((H, W), NOTDEF, np.float64)
    if H > 1 and W > 1:
        A, B, C, D = I[:-1, :-1], I[:-1, 1:], I[1:, :-1], I[1:, 1:]
        gx, gy = (D - A) + (B - C), gy_sign * ((D - A) - (B - C))
        n = np.sqrt((gx * gx + gy * gy) / 4)
        norm[:-1, :-1] = n
        dfd = (n >= rho) if define_at_rho else (n > rho)
        defined[:-1, :-1] = dfd
        gxf, gyf = gx.astype(np.float64).astype(np.float32), gy.astype(np.float64).astype(np.float32)
        a_fast[:-1, :-1] = np.where(dfd, fast_atan2_deg(gxf, -gyf), np.float32(NOTDEF))
        a_true[:-1, :-1] = np.where(dfd, true_atan2_deg(gx.astype(np.float64), -gy.astype(np.float64)), NOTDEF)
    return Front(I, norm, defined, a_fast, a_true, norm[defined].max() if defined.any() else None, rho)


def angle_distance(a, b):
    """|a - b| on the circle, degrees."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound and the comparison
# ---------------------------------------------------------------------------------------------------------------------------------
# The largest |oracle - restatement| over the scaled and norm planes of the whole case list (chunk 64: 32 cases of 3 images, 0.46 M
# scaled pixels), measured with x87 long doubles by test_independent_lsd_front.py (which prints it), and 16 times that: the factor covers the
# spread of differently ordered sums on images that are not in the list.  The nearest real error, the resize with its position in
# double, is at 5e-4; T stays below 1e-9.
MEASURED_MAX = 1.7e-13
T = 16 * MEASURED_MAX
assert T < 1e-9
RHO_MARGIN = 1e-9          # a restatement pixel this close to rho is left out of the defined / undefined comparison: the list has none
ANGLE_POLY_TOL = 1e-3      # degrees, against the polynomial of the restatement's own float32 gradients: one float rounding of gx
                           # moves it by far less, a sign or argument error by degrees
ANGLE_TRUE_TOL = 0.3       # degrees, against the true arctangent: fastAtan2's published precision (tests/test_independent_checks.py)


def compare(want, scaled, norm, angle, max_grad, bound=T, what=""):
    """A plane set (scaled or None, norm, angle in degrees with NOTDEF, the largest norm or None / <= 0 for "none") against the
    restatement `want` (a Front).  Returns (the list of what is wrong — empty: they agree —, the largest plane difference seen, the
    number of pixels left out of the defined / undefined comparison)."""
    bad = []
    worst = 0.0

    def where(mask):
        y, x = np.argwhere(mask)[0]
        return "%d pixels, first (x %d, y %d)" % (int(mask.sum()), x, y)

    for name, got, ref in (("scaled", scaled, want.scaled), ("norm", norm, want.norm)):
        if got is None:
            continue
        if got.shape != ref.shape:
            bad.append("%s %s plane: shape %s, want %s" % (what, name, got.shape, ref.shape))
            return bad, float("inf"), 0
        if got.size == 0:
            continue
        d = np.abs(np.asarray(got).astype(LD) - ref)
        worst = max(worst, float(d.max()))
        if d.max() > bound:
            bad.append("%s %s plane differs by up to %.3g (bound %.3g): %s" % (what, name, float(d.max()), bound, where(d > bound)))
    angle = np.asarray(angle)
    got_def = angle != np.float32(NOTDEF)
    close = np.abs(want.norm - LD(want.rho)) < RHO_MARGIN
    close[-1, :] = False
    close[:, -1] = False
    wrong = (got_def != want.defined) & ~close
    if wrong.any():
        bad.append("%s defined / undefined differs: %s" % (what, where(wrong)))
    both = got_def & want.defined
    if both.any():
        for name, ref, tol in (("polynomial", want.angle_fast, ANGLE_POLY_TOL), ("true arctangent", want.angle_true, ANGLE_TRUE_TOL)):
            d = np.where(both, angle_distance(angle, ref), 0.0)
            if d.max() > tol:
                bad.append("%s angle is up to %.4g degrees from the %s (bound %g): %s" % (what, d.max(), name, tol, where(d > tol)))
    if got_def[-1, :].any() or got_def[:, -1].any() or np.any(norm[-1, :] != 0) or np.any(norm[:, -1] != 0):
        bad.append("%s the last row / column is not (undefined, norm 0)" % what)
    got_max = None if (max_grad is None or max_grad <= 0) else float(max_grad)
    if (got_max is None) != (want.max_grad is None):
        bad.append("%s largest norm: %r, want %r" % (what, got_max, want.max_grad))
    elif got_max is not None:
        worst = max(worst, float(abs(LD(got_max) - want.max_grad)))
        if abs(LD(got_max) - want.max_grad) > bound:
            bad.append("%s largest norm %r, want %r (bound %.3g)" % (what, got_max, float(want.max_grad), bound))
    return bad, worst, int(close.sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name w h scale sigma_scale")
DEFAULT_CHUNK = 64                                           # scaled rows per wave of the streaming form (capi_host.hpp LSD_FRONT_CHUNK)
WIDTHS = {53: 64, 54: 65, 107: 128, 75: 90}                  # source width -> scaled width at 1.2: one strip exactly; a second strip of
                                                             # one pixel; two full strips, pitch = width; pad columns 90 .. 95
TINY = [(7, 7), (7, 6), (6, 7), (6, 6), (4, 5), (3, 3), (2, 9), (9, 2), (1, 9), (1, 1)]      # (w, h); 7 x 7: the first the streaming form takes


def source_for(target, scale=1.2, at_least=False):
    """The source length whose scaled length is `target` (the smallest one that reaches it, with at_least)."""
    for n in range(1, 4096):
        if scaled_len(n, scale) == target or (at_least and scaled_len(n, scale) >= target):
            return n
    raise AssertionError("no source length scales to %d" % target)


def heights(chunk, scale=1.2):
    """Source heights whose scaled heights are below the chunk, the chunk, chunk + 1, and at least 3 chunks + 5."""
    below = source_for(max(chunk // 2, 9), scale, at_least=True)
    assert scaled_len(below, scale) < chunk
    return [below, source_for(chunk, scale), source_for(chunk + 1, scale), source_for(3 * chunk + 5, scale, at_least=True)]


def cases(chunk=DEFAULT_CHUNK):
    out = []
    for w in sorted(WIDTHS):
        assert scaled_len(w, 1.2) == WIDTHS[w]
        for h in heights(chunk):
            out.append(Case("%dx%d" % (w, h), w, h, 1.2, 0.6))
    for scale in (1.5, 2.0):
        h = source_for(chunk + 1, scale, at_least=True)
        out.append(Case("75x%d x%.1f" % (h, scale), 75, h, scale, 0.6))
    for w, h in TINY:
        out.append(Case("tiny %dx%d" % (w, h), w, h, 1.2, 0.6))
    for ss in (0.25, 0.5):                                   # blur radius 1 and 2: lsd_front64_tile<0>, no streaming form
        out.append(Case("75x%d sigma_scale %.2f" % (source_for(chunk + 1), ss), 75, source_for(chunk + 1), 1.2, ss))
    return out


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


_photo = []


def photo():
    if not _photo:
        _photo.append(np.load(os.path.join(ROOT, "tests", "golden", "real", "photos.npz"))["camera"])
    return _photo[0]


def batch(case):
    """Three images of different content (a wrong image stride shows in the second or third): seeded noise; the crop of the `camera`
    photograph at (100, 200), or other noise where the photograph is too small for it; a checkerboard."""
    h, w = case.h, case.w
    crop = photo()[100:100 + h, 200:200 + w]
    second = np.ascontiguousarray(crop) if crop.shape == (h, w) else noise(11 * h + w + 1, h, w)
    return np.stack([noise(7 * h + w, h, w), second, checker(h, w)])


def constant_batch():
    return np.full((3, 40, 53), 17, np.uint8)


def step_edge(h=40, w=53, at=26):
    """A vertical step edge, 40 on the left and 200 on the right, both sides wider than the blur."""
    img = np.full((h, w), 40, np.uint8)
    img[:, at:] = 200
    return img


# ---------------------------------------------------------------------------------------------------------------------------------
# what the oracle computed, and both references of a case (computed once, shared by the tests of a process, never modified)
# ---------------------------------------------------------------------------------------------------------------------------------
OraclePlanes = namedtuple("OraclePlanes", "scaled norm angle max_grad")


def oracle_front(po, img, scale=1.2, sigma_scale=0.6, **config):
    """oracle/line_oracle.hpp lsdDetect on one image: the scaled plane, the norm plane, the angle plane (degrees, NOTDEF) and the
    largest norm above rho (<= 0: none)."""
    from pli_slam_amd import capi
    cfg = capi.default_config(64, 64, orb_nfeatures=100, lsd_nfeatures=0, max_frames=1, lsd_scale=scale, lsd_sigma_scale=sigma_scale,
                              **config)
    fr = po.Frame(po.Config.from_buffer_copy(bytes(cfg)))
    fr.line_extract(0, img)
    return OraclePlanes(fr.lsd_scaled64(0), fr.lsd_modgrad(0), fr.lsd_angle(0), fr.lsd_max_grad(0))


_references = {}


def references(po, case):
    """[(image, OraclePlanes, Front)] of the case's batch."""
    if case not in _references:
        _references[case] = [(img, oracle_front(po, img, case.scale, case.sigma_scale), front(img, case.scale, case.sigma_scale))
                             for img in batch(case)]
        for _, o, f in _references[case]:
            for a in list(o[:3]) + list(f[:5]):
                a.setflags(write=False)
    return _references[case]


def unclaimed_norm_word(norm):
    """csrc/device_prims.hpp tx_unclaimed_norm_word: bit 31 (nobody has claimed the pixel) over the norm in 2^-22 fixed point, cut
    at 0x7FFF0000 — the owner word a front pass writes for the LAZY ids (tests/test_lazy_ids_cpu.py works with the same fixed point)."""
    fix = np.minimum(np.asarray(norm, dtype=np.float64) * 4194304.0, 2147418112.0).astype(np.int64)
    return (fix | 0x80000000).astype(np.uint32)
