"""Independent float64 references for tests/test_undistort.py: the
radial-tangential model evaluated directly per pixel (no running sums), a
float64 bilinear interpolation with a zero border, and the cameras the tests
use.  Nothing here imports the code under test."""
import functools

import numpy as np

# EuRoC MH_01 cam0 (752 x 480) and TUM freiburg1 (640 x 480): fx fy cx cy, D
EUROC = ((458.654, 457.296, 367.215, 248.375),
         (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05), 752, 480)
TUM_FR1 = ((517.3, 516.5, 318.6, 255.3), (0.2624, -0.9531, -0.0054, 0.0026, 1.1633), 640, 480)
CAMERAS = {"euroc": EUROC, "tum_fr1": TUM_FR1}


def K_of(f4, scale=1.0):
    fx, fy, cx, cy = (v / scale for v in f4)
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def coeffs8(D):
    d = np.zeros(8)
    d[:len(D)] = D
    return d


def distort64(x, y, K, D):
    """Ideal normalised coordinates -> distorted pixels of camera K (OpenCV's
    published model, k1 k2 p1 p2 k3 k4 k5 k6), float64."""
    k1, k2, p1, p2, k3, k4, k5, k6 = coeffs8(D)
    r2 = x * x + y * y
    radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]


def five_iterations64(pts, K, D):
    """cv2's point undistortion, one point at a time in Python floats: five
    fixed-point steps x <- (x0 - tangential(x)) / radial(x) from the
    normalised distorted point.  [N,2] float64 normalised coordinates."""
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in coeffs8(D))
    out = []
    for u, v in np.asarray(pts, dtype=np.float64):
        x0, y0 = (float(u) - K[0, 2]) / K[0, 0], (float(v) - K[1, 2]) / K[1, 1]
        x, y = x0, y0
        for _ in range(5):
            r2 = x * x + y * y
            radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
            if radial < 0:
                x, y = x0, y0
                break
            dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            x, y = (x0 - dx) / radial, (y0 - dy) / radial
        out.append((x, y))
    return np.array(out)


def direct_maps(K, D, K_new, W, H):
    """The undistortion maps by direct evaluation at inv(K_new) (j, i, 1):
    float64 [H,W] each, no accumulation along the row."""
    iR = np.linalg.inv(K_new)
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    X = iR[0, 0] * j + iR[0, 1] * i + iR[0, 2]
    Y = iR[1, 0] * j + iR[1, 1] * i + iR[1, 2]
    Wn = iR[2, 0] * j + iR[2, 1] * i + iR[2, 2]
    return distort64(X / Wn, Y / Wn, K, D)


def ulp32(v):
    """The spacing of float32 at |v| (1 ulp of the value)."""
    return np.spacing(np.abs(np.asarray(v)).astype(np.float32)).astype(np.float64)


def quantised_coords(m):
    """cv2's 1/32-pixel quantisation of a float32 map, stated independently:
    round-half-even of v * 32 as Python's round() does it, the integer part
    saturated to the short range.  Returns (integer part, fraction in 1/32)
    as int64 arrays."""
    flat = [round(float(v) * 32.0) for v in np.asarray(m, np.float32).ravel()]
    s = np.array(flat, dtype=np.int64).reshape(np.shape(m))
    return np.clip(np.floor_divide(s, 32), -32768, 32767), np.mod(s, 32)


def bilinear64(img, mapx, mapy):
    """Float64 bilinear interpolation of a uint8 [H,W(,C)] image at the
    quantised coordinates (ix + fx / 32, iy + fy / 32), zero outside the
    image.  Every product is exact in float64 (weights are multiples of
    1/1024, values are bytes)."""
    H, W = img.shape[:2]
    src = img.reshape(H, W, -1).astype(np.float64)
    ix, fx = quantised_coords(mapx)
    iy, fy = quantised_coords(mapy)
    ax, ay = fx / 32.0, fy / 32.0

    def tap(y, x):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        v = src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        return v * ok[..., None]
    out = (((1 - ax) * (1 - ay))[..., None] * tap(iy, ix) + (ax * (1 - ay))[..., None] * tap(iy, ix + 1)
           + ((1 - ax) * ay)[..., None] * tap(iy + 1, ix) + (ax * ay)[..., None] * tap(iy + 1, ix + 1))
    return out[..., 0] if img.ndim == 2 else out


@functools.lru_cache(maxsize=None)
def noise_u8(h, w, c, seed):
    """A uniform-noise uint8 image [h,w,c] ([h,w] for c = 0), read-only."""
    shape = (h, w, c) if c else (h, w)
    a = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    a.setflags(write=False)
    return a


def edge_case_maps(W=53, H=37, seed=3):
    """The hand-built [H,W] maps of the device edge-case test for a W x H
    source: row 0 integer coordinates; row 1 the rounding ties; rows 2-4 the
    last column, the last row and both; row 5 negative halves; row 6 just
    past the last column; rows 7-8 +-2^20; the rest random in range (a margin
    outside the image included)."""
    rng = np.random.default_rng(seed)
    mx = rng.uniform(-2.0, W + 1.0, (H, W)).astype(np.float32)
    my = rng.uniform(-2.0, H + 1.0, (H, W)).astype(np.float32)
    j = np.arange(W, dtype=np.float32)
    mx[0], my[0] = j, np.float32(5.0)
    mx[1, 0::2], mx[1, 1::2], my[1] = 3.015625, 3.046875, 7.046875     # * 32 = 96.5, 97.5
    mx[2], my[2] = W - 1, (j % H) + np.float32(0.25)                   # ix = W-1: p01 outside
    mx[3], my[3] = (j % W) + np.float32(0.75), H - 1                   # iy = H-1: p10 outside
    mx[4], my[4] = W - 1 + (j % 2) * np.float32(0.5), H - 1 + (j % 3) * np.float32(0.25)
    mx[5, 0::3], mx[5, 1::3], mx[5, 2::3] = -0.5, -1.0, -1.5
    my[5] = np.where(j % 2 == 0, np.float32(-0.5), np.float32(4.5))
    mx[6], my[6] = W - 1 + 1 / 32, (j % H)
    mx[7], my[7] = 2.0 ** 20, 3.0
    mx[8, 0::2], mx[8, 1::2] = -2.0 ** 20, 4.0
    my[8, 0::2], my[8, 1::2] = 3.0, -2.0 ** 20
    mx[9, :4] = (-17 / 32, W - 1 - 17 / 32, 0.0, -1 / 32)
    return np.ascontiguousarray(mx), np.ascontiguousarray(my)
