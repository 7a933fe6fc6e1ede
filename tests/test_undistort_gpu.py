"""pli_set_pinhole_distortion and pli_undistort_points against the float64 restatement of tests/helpers_undistort.py, byte for byte,
on xy_un and on cell, for a TUM-like and a EuRoC-like camera: the 4-pixel grids with their far edges, seeded random points around
the image, points far outside it, the wave and block edges of n, the k1 == 0 gate and the removal of the camera."""
import numpy as np
import pytest

import helpers_undistort as hu

pytestmark = pytest.mark.gpu

CAMERAS = {"TUM": hu.TUM, "EUROC": hu.EUROC}


@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    made = {}

    def frontend(name):
        if name not in made:
            (_, (W, H)) = CAMERAS[name]
            made[name] = Frontend(capi.default_config(W, H, orb_nfeatures=200, lsd_nfeatures=20))
        return made[name]
    yield capi, frontend
    for fe in made.values():
        fe.close()


@pytest.fixture(scope="module")
def points():
    """name -> (all points, the restatement's xy_un, the restatement's cell, bounds): computed once."""
    out = {}
    for name, (values, (W, H)) in CAMERAS.items():
        cam = hu.camera(values)
        rng = np.random.default_rng(7)
        rnd = np.stack([rng.uniform(-50, W + 50, 4096), rng.uniform(-50, H + 50, 4096)], axis=1).astype(np.float32)
        pts = np.concatenate([hu.pixel_grid(W, H), rnd, np.array(hu.FAR_POINTS, np.float32), np.array([[cam[2], cam[3]]], np.float32)])
        b = hu.image_bounds(cam, W, H)
        un = hu.undistort_points(pts, cam)
        out[name] = (pts, un, hu.pos_in_grid(un, b), b)
    return out


def _differing(got, want):
    bad = np.flatnonzero((got.reshape(len(got), -1).view(np.uint32) != want.reshape(len(want), -1).view(np.uint32)).any(axis=1))
    return "%d rows differ, first %s: device %s, restatement %s" % (len(bad), bad[:4], got[bad[:4]].tolist(), want[bad[:4]].tolist())


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_bounds_points_and_cells_equal_the_restatement(lib, points, name):
    capi, frontend = lib
    fe = frontend(name)
    values, (W, H) = CAMERAS[name]
    pts, want_un, want_cell, want_b = points[name]
    b = fe.set_pinhole_distortion(values)
    assert b.tobytes() == want_b.tobytes(), (b, want_b)
    un, cell = fe.undistort_points(pts)
    assert un.tobytes() == want_un.tobytes(), _differing(un, want_un)
    assert cell.tobytes() == want_cell.tobytes(), _differing(cell, want_cell)
    assert (cell < 0).any() and (cell >= 0).any() and np.isfinite(un).all()
    un2, none = fe.undistort_points(pts, with_cell=False)                   # cell == NULL
    assert none is None and un2.tobytes() == want_un.tobytes()
    # the capi.PinholeDistortion form of the camera is the same call
    assert fe.set_pinhole_distortion(capi.PinholeDistortion(*[float(v) for v in values])).tobytes() == want_b.tobytes()


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_wave_and_block_edges_of_n(lib, points, name):
    _, frontend = lib
    fe = frontend(name)
    fe.set_pinhole_distortion(CAMERAS[name][0])
    pts, want_un, want_cell, _ = points[name]
    start = len(pts) - 4096 - 4 - 100              # the tail of the grid, the random points behind it
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        un, cell = fe.undistort_points(pts[start:start + n])
        assert un.shape == (n, 2) and cell.shape == (n,)
        assert un.tobytes() == want_un[start:start + n].tobytes() and cell.tobytes() == want_cell[start:start + n].tobytes(), n


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_k1_zero_and_no_camera_copy_their_input(lib, points, name):
    _, frontend = lib
    fe = frontend(name)
    values, (W, H) = CAMERAS[name]
    pts = points[name][0]
    image = np.array([0, W, 0, H], np.float32)
    want_cell = hu.pos_in_grid(pts, image)
    gated = list(values)
    gated[4] = 0.0                                  # k2, p1, p2 (and k3) stay non-zero
    for cam in (gated, None):
        fe.set_pinhole_distortion(values)           # from a real camera each time: the state is replaced, not kept
        b = fe.set_pinhole_distortion(cam)
        assert b.tobytes() == image.tobytes(), b
        un, cell = fe.undistort_points(pts)
        assert un.tobytes() == pts.tobytes(), (cam, _differing(un, pts))
        assert cell.tobytes() == want_cell.tobytes()
