"""Camera calibration and lens undistortion (splatt3r_slam/dataloader.py:
277-317, `Intrinsics`): the optimal new camera matrix, the undistortion maps
and the per-frame 8-bit bilinear remap.

The reference calls cv2.getOptimalNewCameraMatrix, cv2.initUndistortRectifyMap
and cv2.remap.  cv2 is not a dependency here: the three functions are
restated below in numpy (float64, once per camera), and the per-frame remap
runs on the device (include/s3u.h, csrc/undistort.hip) with `remap_u8` as its
bit-exact host oracle.

The restatements follow the text of OpenCV 4.x, calib3d (undistort.dispatch.cpp
`cvUndistortPointsInternal`, calibration.cpp `icvGetRectangles` and
`getOptimalNewCameraMatrix`, undistort.simd.hpp `initUndistortRectifyMap`)
and imgproc (imgwarp.cpp `remap`, 8-bit INTER_LINEAR).  No copy of OpenCV is
on the build machine, so parity with cv2 is unpinned -- the standing SURVEY
§8(c) gives the rasterizer and lietorch: the arithmetic is written down from
the published source and checked against independent float64 evaluations
(tests/test_undistort.py); one test compares with cv2 itself where it is
installed.  Coefficient vectors of length 4, 5 or 8 (k1 k2 p1 p2 [k3 [k4 k5
k6]]); thin-prism and tilt terms are out of scope.

Importing this module does not initialise the GPU.
"""
from __future__ import annotations

import threading
import warnings

import numpy as np
import torch

from splatt3r_amd import _lib
from splatt3r_amd.config import config

INTER_BITS = 5                      # cv2: maps are quantised to 1/32 pixel
INTER_TAB_SIZE = 1 << INTER_BITS
MAP_LIMIT = float(1 << 20)          # |map| <= 2^20 keeps v * 32 inside int32
_GRID = 9                           # icvGetRectangles: N = 9


# ------------------------------------------------------- distortion model --
def _coeffs(D) -> np.ndarray:
    """k1 k2 p1 p2 k3 k4 k5 k6 as float64[8] from a vector of length 4, 5 or 8."""
    d = np.asarray(D, dtype=np.float64).reshape(-1)
    if d.size not in (4, 5, 8):
        raise ValueError(f"distortion coefficients: expected 4, 5 or 8 values "
                         f"(k1 k2 p1 p2 [k3 [k4 k5 k6]]), got {d.size}")
    out = np.zeros(8)
    out[:d.size] = d
    return out


def _K(K) -> np.ndarray:
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"camera matrix: expected 3x3, got {K.shape}")
    return K


def undistort_points(pts, K, D, P=None) -> np.ndarray:
    """cvUndistortPointsInternal: pixel points [N,2] (stored as float32) ->
    ideal points, normalised, or in the pixels of `P` when given.  Exactly 5
    fixed-point iterations in double; float32 [N,2] out."""
    K = _K(K)
    k1, k2, p1, p2, k3, k4, k5, k6 = _coeffs(D)
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ifx, ify = 1.0 / fx, 1.0 / fy          # the C code multiplies by the reciprocal
    x0 = (pts[:, 0] - cx) * ifx
    y0 = (pts[:, 1] - cy) * ify
    x, y = x0.copy(), y0.copy()
    live = np.ones(x.shape, bool)          # points that have not hit icdist < 0
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        neg = live & (icdist < 0)
        x[neg], y[neg] = x0[neg], y0[neg]
        live &= ~neg
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = np.where(live, (x0 - dx) * icdist, x)
        y = np.where(live, (y0 - dy) * icdist, y)
    if P is not None:
        P = _K(np.asarray(P, dtype=np.float64)[:3, :3])
        x, y = P[0, 0] * x + P[0, 2], P[1, 1] * y + P[1, 2]
    return np.stack([x, y], 1).astype(np.float32)


def distort_points(xy, K, D) -> np.ndarray:
    """The forward model: normalised ideal points [N,2] -> distorted pixels
    of camera K, float64 (initUndistortRectifyMap's expression per point)."""
    K = _K(K)
    k1, k2, p1, p2, k3, k4, k5, k6 = _coeffs(D)
    xy = np.asarray(xy, dtype=np.float64)
    x, y = xy[..., 0], xy[..., 1]
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    u = K[0, 0] * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + K[0, 2]
    v = K[1, 1] * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + K[1, 2]
    return np.stack([u, v], -1)


def get_rectangles(K, D, P, W: int, H: int):
    """icvGetRectangles: the 9x9 grid over the image, undistorted; (inner,
    outer) as (x, y, w, h).  inner: the largest rectangle inside the
    undistorted image (max over the first column / row, min over the last);
    outer: the bounding box.  The points are float32 (CV_32FC2) and so are the
    extents' differences."""
    f32 = np.float32
    g = np.arange(_GRID, dtype=np.float32)
    px = g * f32(W - 1) / f32(_GRID - 1)
    py = g * f32(H - 1) / f32(_GRID - 1)
    pts = np.stack(np.meshgrid(px, py), -1).reshape(-1, 2)      # row-major: y outer, x inner
    p = undistort_points(pts, K, D, P).reshape(_GRID, _GRID, 2)
    iX0, iX1 = p[:, 0, 0].max(), p[:, -1, 0].min()
    iY0, iY1 = p[0, :, 1].max(), p[-1, :, 1].min()
    oX0, oX1 = p[..., 0].min(), p[..., 0].max()
    oY0, oY1 = p[..., 1].min(), p[..., 1].max()
    inner = tuple(float(v) for v in (iX0, iY0, f32(iX1 - iX0), f32(iY1 - iY0)))
    outer = tuple(float(v) for v in (oX0, oY0, f32(oX1 - oX0), f32(oY1 - oY0)))
    return inner, outer


def get_optimal_new_camera_matrix(K, D, size, alpha: float = 0.0, new_size=None,
                                  center: bool = False) -> np.ndarray:
    """cv2.getOptimalNewCameraMatrix (the matrix only; the valid-pixel ROI the
    reference discards is not computed).  size, new_size: (W, H)."""
    K = _K(K)
    W, H = int(size[0]), int(size[1])
    nW, nH = (W, H) if new_size is None or tuple(new_size) == (0, 0) else map(int, new_size)
    alpha = float(alpha)
    M = K.copy()
    if center:
        cx0, cy0 = M[0, 2], M[1, 2]
        cx, cy = (nW - 1) * 0.5, (nH - 1) * 0.5
        inner, outer = get_rectangles(K, D, K, W, H)

        def four(r):
            return (cx / (cx0 - r[0]), cy / (cy0 - r[1]),
                    cx / (r[0] + r[2] - cx0), cy / (r[1] + r[3] - cy0))
        s0, s1 = max(four(inner)), min(four(outer))
        s = s0 * (1 - alpha) + s1 * alpha
        M[0, 0] *= s
        M[1, 1] *= s
        M[0, 2] = cx
        M[1, 2] = cy
        return M
    inner, outer = get_rectangles(K, D, None, W, H)

    def fit(r):
        fx, fy = (nW - 1) / r[2], (nH - 1) / r[3]
        return fx, fy, -fx * r[0], -fy * r[1]
    v0, v1 = fit(inner), fit(outer)
    fx, fy, cx, cy = (a * (1 - alpha) + b * alpha for a, b in zip(v0, v1))
    M[0, 0], M[1, 1], M[0, 2], M[1, 2] = fx, fy, cx, cy
    return M


def init_undistort_rectify_map(K, D, K_new, size):
    """cv2.initUndistortRectifyMap(K, D, None, K_new, (W, H), CV_32FC1):
    float32 mapx, mapy [H, W], the distorted source pixel of every pixel of
    the new camera.  The row start is i * iR[:,1] + iR[:,2] and every pixel
    adds iR[:,0] to a running double, as the C loop does."""
    K, K_new = _K(K), _K(K_new)
    k1, k2, p1, p2, k3, k4, k5, k6 = _coeffs(D)
    W, H = int(size[0]), int(size[1])
    if W <= 0 or H <= 0:
        raise ValueError(f"map size {W} x {H} is not positive")
    iR = np.linalg.inv(K_new)
    i = np.arange(H, dtype=np.float64)[:, None]

    def running(r):
        a = np.empty((H, W))
        a[:, :1] = i * iR[r, 1] + iR[r, 2]
        a[:, 1:] = iR[r, 0]
        return np.cumsum(a, axis=1)           # sequential: ((a0 + d) + d) + ...
    _x, _y, _w = running(0), running(1), running(2)
    w = 1.0 / _w
    x, y = _x * w, _y * w
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    u = K[0, 0] * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + K[0, 2]
    v = K[1, 1] * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + K[1, 2]
    return u.astype(np.float32), v.astype(np.float32)


# ------------------------------------------------------------------ remap --
def check_maps(mapx, mapy) -> tuple:
    """The maps as the kernel needs them: float32 [H,W], same shape, finite,
    |v| <= 2^20.  Raises ValueError; returns the (out_h, out_w) shape."""
    for name, m in (("mapx", mapx), ("mapy", mapy)):
        if not isinstance(m, np.ndarray) or m.dtype != np.float32:
            raise ValueError(f"{name}: expected a float32 numpy array, got "
                             f"{getattr(m, 'dtype', type(m).__name__)}")
        if m.ndim != 2 or m.size == 0:
            raise ValueError(f"{name}: expected a non-empty [H,W] array, got shape {m.shape}")
        if not np.all(np.isfinite(m)):
            raise ValueError(f"{name}: holds NaN or infinity")
        if np.abs(m).max() > MAP_LIMIT:
            raise ValueError(f"{name}: |value| exceeds 2^20")
    if mapx.shape != mapy.shape:
        raise ValueError(f"mapx {mapx.shape} and mapy {mapy.shape} differ in shape")
    return mapx.shape


def _quantise(m: np.ndarray):
    """cvRound(v * 32) (ties to even; the product is exact in float32), the
    integer part saturated to the short range, the 5-bit fraction."""
    s = np.rint(m * np.float32(INTER_TAB_SIZE)).astype(np.int64)
    return np.clip(s >> INTER_BITS, -32768, 32767), s & (INTER_TAB_SIZE - 1)


def remap_u8(img: np.ndarray, mapx: np.ndarray, mapy: np.ndarray) -> np.ndarray:
    """cv2.remap(img, mapx, mapy, INTER_LINEAR) with BORDER_CONSTANT 0 for a
    uint8 image [H,W] or [H,W,C], in integer arithmetic: the oracle of
    s3u_remap.  Returns [out_h, out_w(, C)] uint8."""
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError("remap_u8: expected a uint8 [H,W] or [H,W,C] numpy array")
    check_maps(mapx, mapy)
    H, W = img.shape[:2]
    ix, fx = _quantise(mapx)
    iy, fy = _quantise(mapy)
    src = img.reshape(H, W, -1).astype(np.int64)

    def tap(y, x):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        v = src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        return np.where(ok[..., None], v, 0)
    T = INTER_TAB_SIZE
    acc = (((T - fx) * (T - fy))[..., None] * tap(iy, ix) + (fx * (T - fy))[..., None] * tap(iy, ix + 1)
           + ((T - fx) * fy)[..., None] * tap(iy + 1, ix) + (fx * fy)[..., None] * tap(iy + 1, ix + 1)
           + (1 << (2 * INTER_BITS - 1))) >> (2 * INTER_BITS)
    out = acc.astype(np.uint8)
    return out[..., 0] if img.ndim == 2 else out


def _as_frames(img_u8):
    """A uint8 image or batch as a [B,H,W,C] tensor (C = 1 or 3) and whether
    the input was a batch.  [H,W] and [H,W,1] are greyscale."""
    if isinstance(img_u8, np.ndarray):
        if img_u8.dtype != np.uint8:
            raise RuntimeError(f"remap: expected uint8, got {img_u8.dtype}")
        if not img_u8.flags["C_CONTIGUOUS"]:
            raise RuntimeError("remap: input must be contiguous")
        with warnings.catch_warnings():       # a read-only array is fine: it is only read
            warnings.simplefilter("ignore", UserWarning)
            t = torch.from_numpy(img_u8)
    elif torch.is_tensor(img_u8):
        if img_u8.dtype != torch.uint8:
            raise RuntimeError(f"remap: expected uint8, got {img_u8.dtype}")
        _lib.require_contig("remap", img_u8)
        t = img_u8
    else:
        raise RuntimeError(f"remap: expected a numpy array or a tensor, got "
                           f"{type(img_u8).__name__}")
    if t.dim() == 2:
        t = t[..., None]
    if t.dim() not in (3, 4) or t.shape[-1] not in (1, 3):
        raise RuntimeError("remap: expected [H,W], [H,W,C] or [B,H,W,C] with C = 1 or 3, got "
                           f"{tuple(img_u8.shape)}")
    if t.numel() == 0:
        raise RuntimeError(f"remap: empty input {tuple(img_u8.shape)}")
    return (t, True) if t.dim() == 4 else (t[None], False)


class UndistortMap:
    """A validated pair of remap maps for H x W source frames, with its
    device copies (uploaded once per device)."""

    def __init__(self, mapx, mapy, W: int, H: int):
        self.out_h, self.out_w = check_maps(mapx, mapy)
        self.W, self.H = int(W), int(H)
        if self.W <= 0 or self.H <= 0 or self.W > 32767 or self.H > 32767:
            raise ValueError(f"source size {self.H} x {self.W}: expected 1 .. 32767")
        self.mapx = np.ascontiguousarray(mapx)
        self.mapy = np.ascontiguousarray(mapy)
        self._device: dict = {}
        self._lock = threading.Lock()

    def on_device(self, dev: torch.device):
        """(mapx, mapy) on `dev`, uploaded on first use (as ingest._on_device
        keeps its tables; here the copies live and die with the map)."""
        k = (dev.type, dev.index)
        t = self._device.get(k)
        if t is None:
            with self._lock:
                t = self._device.get(k)
                if t is None:
                    # the default stream's copy completes before .to returns (the
                    # source is pageable), so any stream may read it afterwards
                    with torch.cuda.stream(torch.cuda.default_stream(dev)):
                        t = self._device[k] = tuple(torch.from_numpy(m.copy()).to(dev)
                                                    for m in (self.mapx, self.mapy))
        return t

    def remap_host(self, img: np.ndarray) -> np.ndarray:
        if img.shape[:2] != (self.H, self.W):
            raise ValueError(f"remap: the maps are for {self.H} x {self.W} frames, got {img.shape[:2]}")
        return remap_u8(img, self.mapx, self.mapy)

    def remap_device(self, img_u8, device="cuda", stream=None):
        """s3u_remap of a [H,W], [H,W,C] or [B,H,W,C] uint8 image (C = 1 or
        3; numpy or tensor, host or device) -> ([B,out_h,out_w,3] uint8 device
        tensor, whether the input was a batch).  The upload and the launch go
        to `stream` (default: the current stream); nothing waits for them."""
        from splatt3r_amd import ingest
        src, batched = _as_frames(img_u8)
        B, H, W, C = src.shape
        if (H, W) != (self.H, self.W):
            raise ValueError(f"remap: the maps are for {self.H} x {self.W} frames, got {H} x {W}")
        dev = src.device if src.is_cuda else ingest._cuda_device(device)
        mx, my = self.on_device(dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(st):
            if not src.is_cuda:
                src = src.to(dev, non_blocking=True)
            dst = torch.empty((B, self.out_h, self.out_w, 3), dtype=torch.uint8, device=dev)
            _lib.call("s3u_remap", src.data_ptr(), B, H, W, C, mx.data_ptr(), my.data_ptr(),
                      self.out_h, self.out_w, dst.data_ptr(), st.cuda_stream)
        return dst, batched


class Intrinsics:
    """dataloader.py:277-317.  K_orig: the calibrated matrix, K: the optimal
    new matrix of the undistorted image, K_frame: K in the pixels of the
    network's input (after resize_img's resize and centre crop)."""

    def __init__(self, img_size, W, H, K_orig, K, distortion, mapx, mapy):
        self.img_size = img_size
        self.W, self.H = int(W), int(H)
        self.K_orig = K_orig
        self.K = K
        self.distortion = distortion
        self.mapx = mapx
        self.mapy = mapy
        self._map = UndistortMap(mapx, mapy, self.W, self.H)
        if (self._map.out_h, self._map.out_w) != (self.H, self.W):
            raise ValueError(f"maps of shape {mapx.shape} for a {self.H} x {self.W} camera")
        from splatt3r_amd.ingest import ingest_geometry
        # resize_img(np.zeros((H, W, 3)), img_size, return_transformation=True)[1]
        scale_w, scale_h, half_crop_w, half_crop_h = ingest_geometry(self.H, self.W, img_size)[3]
        self.K_frame = self.K.copy()
        self.K_frame[0, 0] = self.K[0, 0] / scale_w
        self.K_frame[1, 1] = self.K[1, 1] / scale_h
        self.K_frame[0, 2] = self.K[0, 2] / scale_w - half_crop_w
        self.K_frame[1, 2] = self.K[1, 2] / scale_h - half_crop_h

    def remap(self, img, device=None, stream=None):
        """cv2.remap(img, mapx, mapy, INTER_LINEAR).  A host array with no
        `device`: the numpy restatement, same layout out as in ([H,W] or
        [H,W,C]).  A device tensor, or any image with `device=`: the HIP
        kernel; the result is a device tensor with three channels
        ([H,W,3], or [B,H,W,3] for a batch), a greyscale input replicated."""
        if device is None and not (torch.is_tensor(img) and img.is_cuda):
            if torch.is_tensor(img):
                return torch.from_numpy(self._map.remap_host(img.numpy()))
            return self._map.remap_host(img)
        out, batched = self._map.remap_device(img, device if device is not None else "cuda", stream)
        return out if batched else out[0]

    def remap_device(self, img_u8, device="cuda", stream=None):
        return self._map.remap_device(img_u8, device, stream)

    @staticmethod
    def from_calib(img_size, W, H, calib, always_undistort=False):
        """calib: fx fy cx cy [k1 k2 p1 p2 [k3 [k4 k5 k6]]].  None when
        config use_calib is off and always_undistort is false."""
        if not config["use_calib"] and not always_undistort:
            return None
        calib = np.asarray(calib, dtype=np.float64).reshape(-1)
        fx, fy, cx, cy = calib[:4]
        distortion = np.zeros(4)
        if len(calib) > 4:
            distortion = np.array(calib[4:])
        _coeffs(distortion)                                   # length 4, 5 or 8
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        center = config["dataset"]["center_principle_point"]
        K_opt = get_optimal_new_camera_matrix(K, distortion, (W, H), 0, (W, H), center=center)
        mapx, mapy = init_undistort_rectify_map(K, distortion, K_opt, (W, H))
        return Intrinsics(img_size, W, H, K, K_opt, distortion, mapx, mapy)
