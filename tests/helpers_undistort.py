"""The undistortion family of the single-camera Frame constructors, restated in float64 numpy from the C text (not from the library):

  undistort_points   cv::undistortPoints(mat, mat, K, mDistCoef, cv::Mat(), K) of OpenCV 3.3.1 (cvUndistortPoints, CV_32FC2, no R,
                     P = K, no tilt): five fixed-point steps, no convergence test, everything in double, K and the coefficients
                     converted from float, the result rounded to float once.  Behind the reference's gate (Frame.cc:874-878,
                     :909-913): with k1 == 0 the points are copied, whatever the other coefficients.
  image_bounds       Frame::ComputeImageBounds (Frame.cc:947-974)
  pos_in_grid        Frame::PosInGrid (Frame.cc:845-855) as posX * 48 + posY, -1 where it returns false
  stereo_from_rgbd   Frame::ComputeStereoFromRGBD (Frame.cc:1309-1330) with the library's in-image guard

The arrays hold one point per row and every operation is element-wise: each expression is the C expression, in its association,
zero terms included, so a row is computed exactly as the scalar loop computes it (numpy's float64 +, -, *, / are IEEE operations;
nothing here sums along an axis).  Conversions float32 -> float64 stand where the C text converts.

forward_brown is NOT derived from the above: it is the definitional Brown-Conrady model (normalised undistorted point -> distorted
pixel), which the tests use to judge the five-step inverse by its re-distortion residual.
"""
import numpy as np

GRID_COLS, GRID_ROWS = 64, 48           # FRAME_GRID_COLS, FRAME_GRID_ROWS (Frame.h)

# (fx, fy, cx, cy, k1, k2, p1, p2, k3), image size.  k3 = 0 stands for a 4-coefficient mDistCoef.
TUM = ((517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314), (640, 480))
EUROC = ((458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0), (752, 480))
FAR_POINTS = ((5000.0, 4000.0), (-3000.0, -2000.0), (1e6, 1e6))


def camera(values):
    """The nine parameters as the float32 values the C structs hold."""
    c = np.asarray(values, np.float32).reshape(9)
    return c


def scaled(values, s):
    """The camera of an image resized by s: fx, fy, cx, cy scale, the coefficients (of normalised coordinates) do not."""
    c = np.asarray(values, np.float64).copy()
    c[:4] *= s
    return camera(c)


def undistort_points(xy, cam, ncoef=5):
    """xy: n x 2 float32 pixels -> n x 2 float32.  cam: camera() or None (no camera: a copy).  ncoef = 4 restates the call with a
    4-coefficient mDistCoef (k[4] = 0 like k[5..11]); with k3 = 0 both are the same function."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    if cam is None or cam[4] == np.float32(0):                  # Frame.cc:874 `mDistCoef.at<float>(0)==0.0`
        return xy.copy()
    fx, fy, cx, cy = (np.float64(v) for v in cam[:4])
    k = np.zeros(12, np.float64)
    k[:ncoef] = np.asarray(cam[4:4 + ncoef], np.float64)
    ifx, ify = 1. / fx, 1. / fy
    # RR = K . I in double (the products with the identity's ones and zeros are exact)
    RR = ((fx, np.float64(0), cx), (np.float64(0), fy, cy), (np.float64(0), np.float64(0), np.float64(1)))
    with np.errstate(all="ignore"):
        x = xy[:, 0].astype(np.float64)
        y = xy[:, 1].astype(np.float64)
        x = (x - cx) * ifx
        y = (y - cy) * ify
        x0, y0 = x, y
        for _ in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = (x0 - deltaX) * icdist
            y = (y0 - deltaY) * icdist
        xx = RR[0][0] * x + RR[0][1] * y + RR[0][2]
        yy = RR[1][0] * x + RR[1][1] * y + RR[1][2]
        ww = 1. / (RR[2][0] * x + RR[2][1] * y + RR[2][2])
        out = np.empty_like(xy)
        out[:, 0] = (xx * ww).astype(np.float32)
        out[:, 1] = (yy * ww).astype(np.float32)
    return out


def _min(a, b):     # std::min(a, b)
    return b if b < a else a


def _max(a, b):     # std::max(a, b)
    return b if a < b else a


def image_bounds(cam, W, H):
    """(mnMinX, mnMaxX, mnMinY, mnMaxY) as float32."""
    if cam is None or cam[4] == np.float32(0):
        return np.array([0, W, 0, H], np.float32)
    m = undistort_points(np.array([[0, 0], [W, 0], [0, H], [W, H]], np.float32), cam)
    return np.array([_min(m[0, 0], m[2, 0]), _max(m[1, 0], m[3, 0]), _min(m[0, 1], m[1, 1]), _max(m[2, 1], m[3, 1])], np.float32)


def _roundf(v):
    """round() of a float argument: halves away from zero.  |v| - floor(|v|) is exact in float32."""
    a = np.abs(v)
    f = np.floor(a)
    f = np.where(a - f >= np.float32(0.5), f + np.float32(1), f)
    return np.copysign(f, v).astype(np.float32)


def pos_in_grid(xy_un, bounds):
    """posX * 48 + posY per row, -1 where PosInGrid returns false.  The comparison is made on the rounded FLOAT, before the
    conversion to int, which gives the reference's answer wherever that conversion is defined and false where it is not."""
    xy_un = np.ascontiguousarray(xy_un, np.float32).reshape(-1, 2)
    b = np.asarray(bounds, np.float32)
    with np.errstate(all="ignore"):
        winv = np.float32(GRID_COLS) / (b[1] - b[0])
        hinv = np.float32(GRID_ROWS) / (b[3] - b[2])
        px = _roundf((xy_un[:, 0] - b[0]) * winv)
        py = _roundf((xy_un[:, 1] - b[2]) * hinv)
        ok = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    cell = np.full(len(xy_un), -1, np.int32)
    cell[ok] = px[ok].astype(np.int32) * GRID_ROWS + py[ok].astype(np.int32)
    return cell


def stereo_from_rgbd(kp_xy, kp_un_xy, depth, bf):
    """(mvuRight, mvDepth): d at (int)v, (int)u of the DISTORTED keypoint, mvuRight from the UNDISTORTED x, in float; a keypoint
    outside the depth image (undefined in the reference) gets -1, -1."""
    kp_xy = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    kp_un_xy = np.ascontiguousarray(kp_un_xy, np.float32).reshape(-1, 2)
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    n = len(kp_xy)
    ur = np.full(n, -1, np.float32)
    dp = np.full(n, -1, np.float32)
    for i in range(n):
        u, v = int(kp_xy[i, 0]), int(kp_xy[i, 1])            # int() truncates like cv::Mat::at<float>(float, float)
        if not (0 <= u < W and 0 <= v < H):
            continue
        d = depth[v, u]
        if d > 0:
            dp[i] = d
            ur[i] = kp_un_xy[i, 0] - np.float32(bf) / d
    return ur, dp


def forward_brown(xy_un, cam):
    """The definitional forward model in float64: undistorted pixel -> normalised point -> distorted pixel,
    x_d = x (1 + k1 r^2 + k2 r^4 + k3 r^6) + 2 p1 x y + p2 (r^2 + 2 x^2), y_d likewise with p1 and p2 exchanged."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (float(v) for v in cam)
    p = np.asarray(xy_un, np.float64).reshape(-1, 2)
    x = (p[:, 0] - cx) / fx
    y = (p[:, 1] - cy) / fy
    r2 = x ** 2 + y ** 2
    radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x ** 2)
    yd = y * radial + p1 * (r2 + 2 * y ** 2) + 2 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


def pixel_grid(W, H, step=4):
    """The step-pixel grid including the far edges: 0..W and 0..H."""
    xs = np.arange(0, W + 1, step, dtype=np.float32)
    ys = np.arange(0, H + 1, step, dtype=np.float32)
    g = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
    return np.ascontiguousarray(g, np.float32)
