"""The float64 restatement of the undistortion family (tests/helpers_undistort.py) judged on its own, without the library: against
the definitional forward Brown model, which does not share the iteration, on a TUM-like and a EuRoC-like camera; its edge cases;
and the figures a first sketch of it gave, which an implementation has to reproduce.

The residual of a point is the larger of |dx| and |dy| between the grid point and the re-distortion of its undistorted position,
in pixels.  (That is the figure the sketch reported: 0.110 px and 0.286 px.  The Euclidean residuals of the same points are 0.142
and 0.291 px.  The TUM maximum lies at the corner (640, 0), the EuRoC one at the edge point (752, 244).)"""
import numpy as np
import pytest

import helpers_undistort as hu

# the sketch's figures, as printed: maxima to 3 decimals, medians to one digit, the bounds as float32 prints
SKETCH = {
    "TUM": dict(cam=hu.TUM, max_res=0.110, med_res=8e-6, bounds=(10.801185, 626.04785, 14.668615, 473.3119), outside=827, n=19481),
    "EUROC": dict(cam=hu.EUROC, max_res=0.286, med_res=2e-3, bounds=(-135.79564, 895.5073, -92.875015, 565.5531), outside=70, n=22869),
}


def residual(cam, grid, un):
    d = np.abs(hu.forward_brown(un, cam) - grid.astype(np.float64))
    return d.max(axis=1)


@pytest.mark.parametrize("name", sorted(SKETCH))
def test_restatement_reproduces_the_sketch_and_inverts_the_forward_model(name):
    S = SKETCH[name]
    values, (W, H) = S["cam"]
    cam = hu.camera(values)
    grid = hu.pixel_grid(W, H)
    assert len(grid) == S["n"]
    un = hu.undistort_points(grid, cam)
    assert np.isfinite(un).all()
    res = residual(cam, grid, un)
    worst = grid[res.argmax()]
    msg = "%s: largest re-distortion residual %.6f px at (%g, %g), median %.3g px" % (name, res.max(), worst[0], worst[1], np.median(res))
    print(msg)
    # the maxima are given to three decimals and the medians to one digit: a restatement of the same function agrees to half a unit
    # of the last printed place (measured: TUM 0.110294 / 8.45e-6, EuRoC 0.286048 / 2.13e-3)
    assert abs(res.max() - S["max_res"]) <= 0.0005, msg
    assert abs(np.median(res) - S["med_res"]) <= 0.5 * 10 ** np.floor(np.log10(S["med_res"])), msg
    # the worst point lies on the image's edge, where the five steps have the farthest to go
    assert worst[0] in (0, W) or worst[1] in (0, H), msg
    b = hu.image_bounds(cam, W, H)
    assert b.dtype == np.float32
    assert [np.format_float_positional(v, unique=True) for v in b] == [np.format_float_positional(np.float32(v), unique=True) for v in S["bounds"]], b
    cell = hu.pos_in_grid(un, b)
    assert int((cell < 0).sum()) == S["outside"]                 # both exits of PosInGrid are taken
    inside = cell[cell >= 0]
    assert inside.max() < hu.GRID_COLS * hu.GRID_ROWS and len(inside) == S["n"] - S["outside"]


@pytest.mark.parametrize("name", sorted(SKETCH))
def test_principal_point_and_far_points(name):
    values, _ = SKETCH[name]["cam"]
    cam = hu.camera(values)
    pp = np.array([[cam[2], cam[3]]], np.float32)
    assert hu.undistort_points(pp, cam).tobytes() == pp.tobytes()          # r2 = 0: every delta is 0 and icdist is 1
    far = hu.undistort_points(np.array(hu.FAR_POINTS, np.float32), cam)
    assert np.isfinite(far).all(), far


@pytest.mark.parametrize("name", sorted(SKETCH))
def test_k1_zero_is_a_copy_whatever_the_other_coefficients(name):
    values, (W, H) = SKETCH[name]["cam"]
    v = list(values)
    v[4] = 0.0
    cam = hu.camera(v)
    assert cam[5] != 0 and cam[6] != 0 and cam[7] != 0
    grid = hu.pixel_grid(W, H, 16)
    assert hu.undistort_points(grid, cam).tobytes() == grid.tobytes()
    assert hu.image_bounds(cam, W, H).tolist() == [0, W, 0, H]
    assert hu.undistort_points(grid, None).tobytes() == grid.tobytes()


@pytest.mark.parametrize("name", sorted(SKETCH))
def test_k3_zero_is_the_four_coefficient_call(name):
    values, (W, H) = SKETCH[name]["cam"]
    v = list(values)
    v[8] = 0.0
    cam = hu.camera(v)
    pts = np.concatenate([hu.pixel_grid(W, H), np.array(hu.FAR_POINTS, np.float32)])
    assert hu.undistort_points(pts, cam, ncoef=5).tobytes() == hu.undistort_points(pts, cam, ncoef=4).tobytes()


def test_pos_in_grid_rounds_halves_away_from_zero_and_rejects_what_no_int_holds():
    b = np.array([0, 64, 0, 48], np.float32)                               # one pixel per cell
    pts = np.array([[0.5, 0.5], [0.49999997, 1.5], [-0.4, 0], [-0.5, 0], [63.4, 47.4], [63.5, 0], [0, 47.5],
                    [np.nan, 1], [1, np.inf], [-np.inf, 1], [3e9, 1]], np.float32)
    assert hu.pos_in_grid(pts, b).tolist() == [1 * 48 + 1, 0 * 48 + 2, 0, -1, 63 * 48 + 47, -1, -1, -1, -1, -1, -1]


def test_stereo_from_rgbd_reads_the_distorted_pixel_and_writes_from_the_undistorted_x():
    depth = np.zeros((4, 6), np.float32)
    depth[1, 2], depth[1, 3], depth[2, 2] = 2.0, 4.0, -1.0
    kp = np.array([[2.9, 1.9], [3.0, 1.0], [2.5, 2.5], [0.5, 0.5], [6.0, 1.0], [-0.5, 1.0]], np.float32)
    un = kp + np.float32(1.25)                                             # "undistorted" x in another pixel
    ur, dp = hu.stereo_from_rgbd(kp, un, depth, 8.0)
    assert dp.tolist() == [2.0, 4.0, -1.0, -1.0, -1.0, -1.0]
    assert ur[:2].tolist() == [np.float32(2.9) + np.float32(1.25) - 4.0, 3.0 + 1.25 - 2.0] and (ur[2:] == -1).all()
