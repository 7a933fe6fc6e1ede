"""Independent restatements of the two descriptor stages, for the checks in test_independent_descriptors*.py.

Written from the published algorithms (Rublee et al., "ORB: an efficient alternative to SIFT or SURF", ICCV 2011: intensity
centroid and steered BRIEF; Zhang & Koch, "An efficient and robust line segment matching approach based on LBD descriptor and
pairwise geometric consistency", JVCIR 2013: the line band descriptor) and from what the reference documents about them
(src/ORBextractor.cc:75-145,451-467; Thirdparty/line_descriptor/src/binary_descriptor_custom.cpp:74-107,217-259,401-412,
1026-1340).  Nothing here is taken from oracle/: the disk is built from its definition, the moments are sums over the disk's
cells (not the reference's row walk), and everything that is not part of the DEFINITION of a sample position is computed
in float64.  numpy only (the GPU tests import this file)."""
import ctypes
import ctypes.util
import math
import os

import numpy as np

F32 = np.float32
U32 = 2.0 ** -24                        # unit roundoff of float32
HALF_PATCH = 15                         # ORBextractor.cc:71
PATTERN_INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pli_orb_pattern.inc")
# (float)(CV_PI / 180.f): the division is done in double, ORBextractor.cc:104
FACTOR_PI = F32(math.pi / 180.0)

# LBD band pairs whose 8 statistics are compared bit by bit (binary_descriptor_custom.cpp:74-107): every pair (i, j), i < j,
# of the 9 bands with j - i <= 5 when i <= 1, and all pairs above band 1 otherwise -- 32 pairs, listed in this order.
LBD_COMBINATIONS = np.array([
    (0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6),
    (2, 3), (2, 4), (2, 5), (2, 6), (2, 7), (2, 8), (3, 4), (3, 5), (3, 6), (3, 7), (3, 8),
    (4, 5), (4, 6), (4, 7), (4, 8), (5, 6), (5, 7), (5, 8), (6, 7), (6, 8), (7, 8)], np.int64)
NUM_BANDS, BAND_WIDTH = 9, 7            # BinaryDescriptor::Params defaults (widthOfBand_ = 7), 63-row support region


# ------------------------------------------------------------------------------------------------------------------------------
# ORB: intensity centroid and steered BRIEF
# ------------------------------------------------------------------------------------------------------------------------------
def orb_pattern():
    """The 256 point pairs (x0, y0, x1, y1) of include/pli_orb_pattern.inc, (256, 4) int64."""
    txt = open(PATTERN_INC).read()
    body = "\n".join(l for l in txt.splitlines() if not l.lstrip().startswith("//"))
    vals = np.array([int(t) for t in body.replace("\n", "").split(",") if t.strip()], np.int64)
    assert vals.size == 1024
    return vals.reshape(256, 4)


def umax_table(r=HALF_PATCH):
    """u_max[v], v = 0..r: the half-width of row v of the digital disk of radius r.  Below 45 degrees a row ends at the rounded
    circle, round(sqrt(r^2 - v^2)); above it the disk is made symmetric under transposition, so the half-width of row v is the
    last column u whose own row reaches v: max{u : u_max[u] >= v} (ORBextractor.cc:451-467 builds the same table)."""
    lo = [int(round(math.sqrt(r * r - v * v))) for v in range(r + 1)]
    vmin = int(math.ceil(r * math.sqrt(2.0) / 2))
    return np.array([lo[v] if v < vmin else max(u for u in range(r + 1) if lo[u] >= v) for v in range(r + 1)], np.int64)


def disk_offsets(r=HALF_PATCH):
    """(u, v) of every cell of the disk: |u| <= u_max[|v|]."""
    um = umax_table(r)
    uu, vv = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1))
    inside = np.abs(uu) <= um[np.abs(vv)]
    return uu[inside], vv[inside]


def ic_moments(level, x, y):
    """Integer moments m_01 = sum v I(x+u, y+v) and m_10 = sum u I(x+u, y+v) over the radius-15 disk around each (x, y)."""
    level = np.asarray(level)
    x, y = np.atleast_1d(np.asarray(x, np.int64)), np.atleast_1d(np.asarray(y, np.int64))
    u, v = disk_offsets()
    assert (x - HALF_PATCH >= 0).all() and (y - HALF_PATCH >= 0).all()
    assert (x + HALF_PATCH < level.shape[1]).all() and (y + HALF_PATCH < level.shape[0]).all()
    I = level[y[:, None] + v[None, :], x[:, None] + u[None, :]].astype(np.int64)
    return I @ v, I @ u


_libm = None


def _libm_f32():
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for f in (_libm.cosf, _libm.sinf):
            f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    return _libm


def cos_sin_f32(x, trig):
    """float32 cos and sin of the float32 x: "cr" the correctly rounded values (float)cos((double)x); "cosf" this machine's libm
    cosf / sinf (what the reference's unqualified cos(float) becomes under `using namespace std;`)."""
    x = F32(x)
    if trig == "cr":
        return F32(math.cos(float(x))), F32(math.sin(float(x)))
    if trig == "cosf":
        m = _libm_f32()
        return F32(m.cosf(float(x))), F32(m.sinf(float(x)))
    raise ValueError(trig)


def _round_half_even(v):
    return np.rint(v).astype(np.int64)


def _round_ties_down(v):
    return np.ceil(v - v.dtype.type(0.5)).astype(np.int64)


def steered_brief(blur_level, x, y, angle_deg, trig, pattern=None, swap_ab=False, ties="even"):
    """Steered BRIEF of the keypoints (x, y, angle in degrees) of one blurred pyramid level.

    Bit i compares the blurred image at the two points of pair i, rotated by the keypoint angle: t0 < t1 with the point (px, py)
    taken at row round(px sin + py cos), column round(px cos - py sin) from the keypoint (ORBextractor.cc:106-145; rows grow
    downwards).  Computed twice:
      * float32 with the reference's operation order: angle * factorPI, then a = cos, b = sin per `trig`, products and one
        sum each without fused multiply-add, rounding half to even (cvRound);
      * float64 from the exact angle.
    Returns (bits32, bits64, margin): (n, 256) bool, (n, 256) bool and the smallest distance in px of the four float64 sample
    coordinates of the bit from a rounding tie.  pattern / swap_ab / ties: deliberate mistakes for the mutation tests."""
    P = orb_pattern() if pattern is None else np.asarray(pattern, np.int64)
    blur = np.asarray(blur_level)
    x, y = np.atleast_1d(np.asarray(x, np.int64)), np.atleast_1d(np.asarray(y, np.int64))
    ang = np.atleast_1d(np.asarray(angle_deg, F32))
    n = len(x)
    a32, b32 = np.zeros(n, F32), np.zeros(n, F32)
    for i in range(n):
        a32[i], b32[i] = cos_sin_f32(F32(ang[i] * FACTOR_PI), trig)
    if swap_ab:
        a32, b32 = b32, a32
    rnd = _round_half_even if ties == "even" else _round_ties_down
    px, py = P[:, 0::2], P[:, 1::2]                                             # (256, 2): point 0 and point 1 of each pair
    a, b = a32[:, None, None], b32[:, None, None]
    row32 = px.astype(F32) * b + py.astype(F32) * a
    col32 = px.astype(F32) * a - py.astype(F32) * b
    rad = np.radians(ang.astype(np.float64))
    a64, b64 = np.cos(rad)[:, None, None], np.sin(rad)[:, None, None]
    row64 = px * b64 + py * a64
    col64 = px * a64 - py * b64

    def sample(r, c):
        yy, xx = y[:, None, None] + r, x[:, None, None] + c
        assert (yy >= 0).all() and (xx >= 0).all() and (yy < blur.shape[0]).all() and (xx < blur.shape[1]).all()
        t = blur[yy, xx].astype(np.int32)
        return t[:, :, 0] < t[:, :, 1]
    bits32 = sample(rnd(row32), rnd(col32))
    bits64 = sample(_round_half_even(row64), _round_half_even(col64))
    tie = lambda v: np.abs(v - (np.floor(v) + 0.5))
    margin = np.minimum(tie(row64), tie(col64)).min(axis=2)
    return bits32, bits64, margin


def pack_bits(bits):
    """(n, 256) bool -> (n, 32) u8, bit k of byte i = bit 8 i + k (desc[i] |= (t0 < t1) << k)."""
    return np.packbits(np.asarray(bits, bool).reshape(-1, 32, 8), axis=2, bitorder="little").reshape(-1, 32)


# ------------------------------------------------------------------------------------------------------------------------------
# LBD
# ------------------------------------------------------------------------------------------------------------------------------
def lbd_weights(exchange=False):
    """Gaussian weights of BinaryDescriptor's constructor (binary_descriptor_custom.cpp:217-259), float64, integer-division
    quirks kept: local f_l over 3 bands, centre (3*7 - 1) / 2 = 10, sigma (2*7 + 1) / 2 = 7 (integer division, not 7.5);
    global f_g over the 63 rows, centre and sigma (9*7 - 1) / 2 = 31.  exchange: the two sigmas swapped (a mutation)."""
    uL, sL = (BAND_WIDTH * 3 - 1) // 2, (BAND_WIDTH * 2 + 1) // 2
    uG = (NUM_BANDS * BAND_WIDTH - 1) // 2
    sG = uG
    if exchange:
        sL, sG = sG, sL
    gl = np.exp(-(np.arange(3 * BAND_WIDTH) - uL) ** 2 / (2.0 * sL * sL))
    gg = np.exp(-(np.arange(NUM_BANDS * BAND_WIDTH) - uG) ** 2 / (2.0 * sG * sG))
    return gl, gg


def lbd_sample_positions(kl, W, H, trig):
    """(rows, cols) of the 63 x numOfPixels support-region samples, int64: the reference's float32 walk, which is part of the
    descriptor's definition (binary_descriptor_custom.cpp:1118-1182): direction (dL0, dL1) = cos / sin of the float angle per
    `trig`, the start point -dL * halfWidth + (dL1, -dL0) * halfHeight + middle, rows stepped by (-dL1, +dL0) and samples by
    (+dL0, +dL1) in sequential float32 sums, std::round (half away from zero), clamped to the image."""
    L = int(kl["numOfPixels"])
    hw, hh = F32((L - 1) // 2), F32((NUM_BANDS * BAND_WIDTH - 1) // 2)
    dL0, dL1 = cos_sin_f32(kl["angle"], trig)
    midX = F32(0.5 * float(F32(kl["sPointInOctaveX"]) + F32(kl["ePointInOctaveX"])))
    midY = F32(0.5 * float(F32(kl["sPointInOctaveY"]) + F32(kl["ePointInOctaveY"])))
    x0 = F32(F32(F32(-dL0) * hw) + F32(dL1 * hh)) + midX
    y0 = F32(F32(F32(-dL1) * hw) - F32(dL0 * hh)) + midY
    nrow = NUM_BANDS * BAND_WIDTH
    sx0 = np.cumsum(np.concatenate([[x0], np.full(nrow - 1, -dL1, F32)]).astype(F32), dtype=F32)   # sequential float32 sums
    sy0 = np.cumsum(np.concatenate([[y0], np.full(nrow - 1, dL0, F32)]).astype(F32), dtype=F32)
    sx = np.cumsum(np.concatenate([sx0[:, None], np.full((nrow, L - 1), dL0, F32)], axis=1), axis=1, dtype=F32)
    sy = np.cumsum(np.concatenate([sy0[:, None], np.full((nrow, L - 1), dL1, F32)], axis=1), axis=1, dtype=F32)

    def round_away(v):
        v = v.astype(np.float64)                     # exact: |v| + 0.5 of a float32 below 2^15 is exact in float64
        return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)
    cols = np.clip(round_away(sx), 0, W - 1)
    rows = np.clip(round_away(sy), 0, H - 1)
    return rows, cols


def lbd_vector64(dx, dy, kl, trig="cr", exchange_weights=False, clip=True, std_mean_term=True):
    """The 72-float LBD of one keyline in float64 after the float32 sampling walk (lbd_sample_positions): gradients projected
    on the line direction dL and its clockwise normal dO = (-dL1, dL0), positive and negative parts summed per row and scaled
    by the global weight of the row; every row feeds its own band and the two neighbours with the local weights; per band the
    weighted mean and standard deviation of each of the 4 quantities (divided by 14 rows for the two outer bands, 21 for the
    others); the means and the stds normalised separately to unit length, clipped at 0.4, and the whole vector renormalised
    (binary_descriptor_custom.cpp:1130-1340).  The float64 variance is never negative beyond rounding (Cauchy-Schwarz over
    the band's 14 / 21 terms), so it is clamped at 0.  The keyword switches are mutations for the tests."""
    H, W = dx.shape
    rows, cols = lbd_sample_positions(kl, W, H, trig)
    th = float(F32(kl["angle"]))
    c, s = math.cos(th), math.sin(th)
    gx, gy = dx[rows, cols].astype(np.float64), dy[rows, cols].astype(np.float64)
    gL = gx * c + gy * s
    gO = -gx * s + gy * c
    gl, gg = lbd_weights(exchange_weights)
    R = np.stack([np.where(gL > 0, gL, 0).sum(1), -np.where(gL > 0, 0, gL).sum(1),
                  np.where(gO > 0, gO, 0).sum(1), -np.where(gO > 0, 0, gO).sum(1)], 1) * gg[:, None]      # (63, 4)
    S1, S2 = np.zeros((NUM_BANDS, 4)), np.zeros((NUM_BANDS, 4))
    for h in range(NUM_BANDS * BAND_WIDTH):
        b, k = h // BAND_WIDTH, h % BAND_WIDTH
        for bb, w in ((b, gl[k + BAND_WIDTH]), (b - 1, gl[k + 2 * BAND_WIDTH]), (b + 1, gl[k])):
            if 0 <= bb < NUM_BANDS:
                S1[bb] += w * R[h]
                S2[bb] += w * w * R[h] ** 2
    invN = np.array([1.0 / 14 if b in (0, NUM_BANDS - 1) else 1.0 / 21 for b in range(NUM_BANDS)])[:, None]
    mean = S1 * invN
    var = S2 * invN - (mean * mean if std_mean_term else 0.0)
    std = np.sqrt(np.maximum(var, 0.0))
    v = np.concatenate([mean, std], 1)            # per band: 4 means (pgdL, ngdL, pgdO, ngdO), then the 4 stds
    m, sd = v[:, :4], v[:, 4:]
    v = np.concatenate([m / math.sqrt((m * m).sum()), sd / math.sqrt((sd * sd).sum())], 1).ravel()
    if clip:
        v = np.minimum(v, 0.4)
    return v / math.sqrt((v * v).sum())


def lbd_bits(vec, combinations=None):
    """LBD binarisation (binary_descriptor_custom.cpp:401-412,662-666): byte k compares the 8 statistics of band pair k,
    bit i = f1[i] > f2[i].  vec (n, 72) or (72,).  Returns ((n, 32) u8, (n, 256) margin |f1 - f2|)."""
    comb = LBD_COMBINATIONS if combinations is None else np.asarray(combinations)
    v = np.atleast_2d(np.asarray(vec, np.float64)).reshape(-1, NUM_BANDS, 8)
    f1, f2 = v[:, comb[:, 0], :], v[:, comb[:, 1], :]                        # (n, 32, 8)
    return pack_bits((f1 > f2).reshape(-1, 256)), np.abs(f1 - f2).reshape(-1, 256)


def lbd_error_bound(length):
    """Absolute bound on |float32 LBD entry - lbd_vector64 entry| for a line of `length` samples per row.

    The float32 computation is a chain of sequential sums: a row of `length` projected gradients, a band of 21 weighted rows,
    the normalisation sums of 36 squares each and the renormalisation sum of 72, each followed by O(1) roundings.  Rounding
    errors of a sum of n terms behave as independent zero-mean variables, so its relative error stays below lambda sqrt(n) u
    with probability 1 - 2 exp(-lambda^2 / 2) (Higham & Mary, SIAM J. Sci. Comput. 41(5), 2019); lambda = 4 here.  The
    final entries are at most 1 in size.  A std amplifies the relative error of its band sums by about (1 + mean^2 / var) / 2;
    the local weights, which run from exp(-100 / 98) = 0.36 to 1 over the band's rows, keep that below 4 unless the band is
    flat.  So 16 sqrt(n) u summed over the four sums: 8.6e-5 at 5000 samples, the longest line of a 4095 x 4095 image."""
    n = math.sqrt(length) + math.sqrt(21) + math.sqrt(36) + math.sqrt(72)
    return 16 * n * U32


# ------------------------------------------------------------------------------------------------------------------------------
# The checks, on one pyramid level's keypoints / one image's keylines (oracle or kernel outputs alike)
# ------------------------------------------------------------------------------------------------------------------------------
TIE_MARGIN = 1e-4


def check_orb_level(level, blur, lx, ly, angle, desc, trig, fast_atan2, **mutation):
    """Keypoints (lx, ly) in level coordinates with their table angle and 32-byte descriptors.  Returns a dict: `fail`, a list
    of what does not hold (empty = all good), and counts: `disagree` (float64 bits that differ from the float32 bits, all at a
    tie margin below TIE_MARGIN when the check holds), `near_ties` (bits with a margin below TIE_MARGIN), `flat` (patches
    with m_01 = m_10 = 0)."""
    fail = []
    lx, ly = np.asarray(lx, np.int64), np.asarray(ly, np.int64)
    angle = np.asarray(angle, F32)
    out = {"fail": fail, "n": len(lx), "disagree": 0, "near_ties": 0, "flat": 0}
    if not len(lx):
        return out
    m01, m10 = ic_moments(level, lx, ly)
    want = np.array([fast_atan2(float(a), float(b)) for a, b in zip(m01, m10)], F32)
    bad = np.flatnonzero(want.view(np.int32) != angle.view(np.int32))
    if bad.size:
        fail.append("angle != fastAtan2(moments) at %d keypoints, first %s" % (bad.size, bad[:5].tolist()))
    ref = np.degrees(np.arctan2(m01.astype(np.float64), m10.astype(np.float64))) % 360.0
    d = np.abs(ref - angle.astype(np.float64))
    d = np.minimum(d, 360.0 - d)
    if d.max() > 0.3:
        fail.append("angle off atan2 by %.4f deg" % d.max())
    out["flat"] = int(((m01 == 0) & (m10 == 0)).sum())
    bits32, bits64, margin = steered_brief(blur, lx, ly, angle, trig, **mutation)
    bad = np.flatnonzero((pack_bits(bits32) != np.asarray(desc, np.uint8)).any(1))
    if bad.size:
        fail.append("float32 steered BRIEF != descriptor at %d keypoints, first %s" % (bad.size, bad[:5].tolist()))
    dis = bits32 != bits64
    out["disagree"], out["near_ties"] = int(dis.sum()), int((margin < TIE_MARGIN).sum())
    if (margin[dis] >= TIE_MARGIN).any():
        fail.append("float64 bits differ away from a rounding tie (margin %.3g)" % margin[dis].max())
    return out


def check_lbd(dx, dy, keylines, lbd_float, ldesc, trig, combinations=None, **mutation):
    """Keylines with their float LBD vectors (n, 72) and descriptors (n, 32) on the Sobel planes dx, dy.  Returns a dict:
    `fail`, `undecided` (bits whose float64 margin is within 4 bounds, not checked) and `worst` (largest error / bound)."""
    fail, und, worst = [], 0, 0.0
    dx, dy = np.asarray(dx), np.asarray(dy)
    for i, kl in enumerate(keylines):
        v = lbd_vector64(dx, dy, kl, trig, **mutation)
        bound = lbd_error_bound(int(kl["numOfPixels"]))
        if bound > 1e-4:
            fail.append("line %d: bound %.3g above 1e-4" % (i, bound))
        err = np.abs(v - np.asarray(lbd_float[i], np.float64)).max()
        worst = max(worst, err / bound)
        if not err <= bound:
            fail.append("line %d: float LBD off by %.3g > bound %.3g" % (i, err, bound))
        bits, margin = lbd_bits(v, combinations)
        sure = margin[0] > 4 * bound
        got = np.unpackbits(np.asarray(ldesc[i], np.uint8), bitorder="little").astype(bool)
        want = np.unpackbits(bits[0], bitorder="little").astype(bool)
        if (got[sure] != want[sure]).any():
            fail.append("line %d: %d decided LBD bits differ" % (i, int((got[sure] != want[sure]).sum())))
        und += int((~sure).sum())
    return {"fail": fail, "n": len(keylines), "undecided": und, "worst": worst}


def level_dims(width, height, scale_factor, nlevels):
    """(w, h) of every pyramid level: cvRound(size * 1 / scale) with the scales as float32 products (ORBextractor.cc:414-426,
    1156-1158)."""
    sc, dims = F32(1.0), []
    for l in range(nlevels):
        if l:
            sc = F32(sc * F32(scale_factor))
        inv = F32(F32(1.0) / sc)
        dims.append((int(np.rint(F32(width) * inv)), int(np.rint(F32(height) * inv))))
    return dims


def constructed_image(W=376, H=240, seed=3):
    """Bright bars along all four borders (support regions clamped at the image edge), axis-aligned and 45-degree bars,
    textured blocks whose corners sit near the 19-px edge margin of pyramid levels 0-3 (at 19 x 1.2^l px from the border),
    and isolated bright pixels: the keypoint on one has a flat patch (m_01 = m_10 = 0)."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 60, np.uint8)
    img[:3, :] = 220; img[-3:, :] = 220; img[:, :3] = 200; img[:, -3:] = 200
    img[40:44, 60:W - 60] = 250                                                  # horizontal bar
    img[60:H - 60, 100:103] = 10                                                 # vertical bar
    for k in range(min(120, H - 120, W - 200)):                                  # 45-degree bar
        img[70 + k:74 + k, 180 + k] = 240
    for l in range(4):
        o = int(round(19 * 1.2 ** l)) + (1 if l == 0 else 0)
        for x0, y0 in ((o, o), (W - o - 21, o), (o, H - o - 21), (W - o - 21, H - o - 21)):
            img[y0:y0 + 21, x0:x0 + 21] = rng.integers(0, 256, (21, 21), dtype=np.uint8)
    img[H - 45:H - 24, W // 2:W // 2 + 21] = rng.integers(0, 256, (21, 21), dtype=np.uint8)
    for x, y in ((50, 120), (150, 200), (W - 50, 120)):
        img[y, x] = 255
    return img
