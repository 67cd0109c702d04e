"""Device-side frame ingest (include/s3i.h): a raw uint8 HxWx3 frame goes to
the device once and one HIP launch produces what the host path
(splatt3r_utils.resize_img: PIL resize + centre crop + ImgNorm) produces,
bit for bit -- the normalised [B,3,h,w] float32 tensor and the cropped uint8
image -- for a batch of frames.

The host side here is the geometry (resize_img's size / filter / crop rule)
and Pillow's per-axis resample tables (libImaging/Resample.c
precompute_coeffs + normalize_coeffs_8bpc): int32 coefficients scaled by
2^22 and the source window of every output sample.  Pillow's 8-bit resample
is integer arithmetic on those tables, so the kernel reproduces it exactly;
ImgNorm is a 256-entry table built with the host path's own expression.

Importing this module does not initialise the GPU.
"""
from __future__ import annotations

import math
import threading
import warnings

import numpy as np
import torch

from splatt3r_amd import _lib

LANCZOS = "lanczos"
BICUBIC = "bicubic"
PRECISION_BITS = 22            # Pillow: 32 - 8 - 2

# --------------------------------------------------------------- geometry --
def ingest_geometry(in_h: int, in_w: int, size: int, square_ok: bool = False):
    """resize_img's rule (splatt3r_utils.py:646-693) for an in_h x in_w
    frame: ((W, H) resized size, filter, (x0, y0, x1, y1) crop box in the
    resized image, the return_transformation tuple)."""
    assert size in (224, 512)
    W1, H1 = int(in_w), int(in_h)
    long_edge = round(size * max(W1 / H1, H1 / W1)) if size == 224 else size
    S = max(W1, H1)
    filt = LANCZOS if S > long_edge else BICUBIC
    W, H = (int(round(x * long_edge / S)) for x in (W1, H1))
    cx, cy = W // 2, H // 2
    if size == 224:
        half = min(cx, cy)
        box = (cx - half, cy - half, cx + half, cy + half)
    else:
        halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
        if not square_ok and W == H:
            halfh = 3 * halfw / 4
        box = (cx - halfw, cy - halfh, cx + halfw, cy + halfh)
    box = tuple(int(round(v)) for v in box)            # PIL.Image.crop
    cw, ch = box[2] - box[0], box[3] - box[1]
    return (W, H), filt, box, (W1 / W, H1 / H, (W - cw) / 2, (H - ch) / 2)


def resize_depth(depth_hw, size: int = 512) -> np.ndarray:
    """A depth image [H, W] brought to the geometry resize_img gives the
    camera image of the same size (ingest_geometry: resize, then centre
    crop), sampled nearest on the host: output pixel (x, y) of the resized
    image takes source pixel (floor((x + 0.5) in_w / W), floor((y + 0.5)
    in_h / H)), Pillow's NEAREST rule.  Depth is never blended across a
    discontinuity, and an invalid value (0) stays what it is.  float32."""
    d = np.asarray(depth_hw)
    if d.ndim != 2:
        raise ValueError(f"resize_depth: depth must be [H, W], got {d.shape}")
    in_h, in_w = d.shape
    (W, H), _, box, _ = ingest_geometry(in_h, in_w, size)
    xs = np.minimum(((np.arange(box[0], box[2]) + 0.5) * (in_w / W)).astype(np.int64), in_w - 1)
    ys = np.minimum(((np.arange(box[1], box[3]) + 0.5) * (in_h / H)).astype(np.int64), in_h - 1)
    return np.ascontiguousarray(d[ys[:, None], xs[None, :]], dtype=np.float32)


# ----------------------------------------------------------------- tables --
def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTERS = {LANCZOS: (_lanczos, 3.0), BICUBIC: (_bicubic, 2.0)}
_TABLES: dict = {}
_DEVICE: dict = {}
_cache_lock = threading.Lock()       # _TABLES
_device_lock = threading.Lock()      # _DEVICE (never held together with _cache_lock)


def resample_tables(in_size: int, out_size: int, filter: str):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis:
    (coeffs int32 [out_size, ksize], bounds int32 [out_size, 2] = (xmin,
    count)).  Python doubles and math.sin (libm, as Pillow's C code), in
    Pillow's order of operations.  Cached; the arrays are read-only."""
    key = (int(in_size), int(out_size), filter)
    got = _TABLES.get(key)
    if got is not None:
        return got
    in_size, out_size = key[:2]
    fn, support = _FILTERS[filter]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    coeffs = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        # C's (int) truncates toward zero, as Python's int()
        coeffs[xx, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        bounds[xx] = (xmin, xmax)
    coeffs.setflags(write=False)
    bounds.setflags(write=False)
    with _cache_lock:
        got = _TABLES.setdefault(key, (coeffs, bounds))
    return got


def norm_lut() -> torch.Tensor:
    """ImgNorm of every byte, with the host path's expression (resize_img:
    (uint8.astype(float32) / 255.0 - 0.5) / 0.5)."""
    return (torch.arange(256, dtype=torch.float32) / 255.0 - 0.5) / 0.5


def unit_lut() -> torch.Tensor:
    """uint8 / 255.0 as float32 (create_frame's Frame.uimg)."""
    return torch.arange(256, dtype=torch.float32) / 255.0


def _on_device(dev: torch.device, key, make):
    """The device copy of a host table: uploaded once per device."""
    k = (dev.type, dev.index, key)
    t = _DEVICE.get(k)
    if t is None:
        with _device_lock:
            t = _DEVICE.get(k)
            if t is None:
                # the default stream's copy completes before .to returns (the
                # source is pageable), so any stream may read it afterwards
                with torch.cuda.stream(torch.cuda.default_stream(dev)):
                    t = _DEVICE[k] = make().contiguous().to(dev)
    return t


def _device_tables(dev, in_size, out_size, filt):
    # the host tables first: resample_tables takes the cache lock itself, so
    # it must not run inside _on_device's
    k, b = resample_tables(in_size, out_size, filt)
    key = (in_size, out_size, filt)
    return (_on_device(dev, key + ("k",), lambda: torch.from_numpy(k.copy())),
            _on_device(dev, key + ("b",), lambda: torch.from_numpy(b.copy())))


def unit_image(uimg_u8: torch.Tensor) -> torch.Tensor:
    """A device uint8 image as float32 / 255.0, with the host's quotients
    (the device's division by a scalar multiplies by a reciprocal)."""
    return _on_device(uimg_u8.device, "unit", unit_lut)[uimg_u8.long()]


_TWO_LAUNCH = False


def set_path(path: int) -> None:
    """Testing hook (s3i_set_path): 0 = automatic, 1 = always the two-launch
    path with the uint8 intermediate in a workspace.  Same results."""
    global _TWO_LAUNCH
    _lib.lib().s3i_set_path(int(path))
    _TWO_LAUNCH = int(path) == 1


# ------------------------------------------------------- public interface --
def _check_input(img_u8):
    if isinstance(img_u8, np.ndarray):
        if img_u8.dtype != np.uint8:
            raise RuntimeError(f"resize_img_device: expected uint8, got {img_u8.dtype}")
        if not img_u8.flags["C_CONTIGUOUS"]:
            raise RuntimeError("resize_img_device: input must be contiguous")
        with warnings.catch_warnings():       # a read-only array is fine: it is only read
            warnings.simplefilter("ignore", UserWarning)
            t = torch.from_numpy(img_u8)
    elif torch.is_tensor(img_u8):
        if img_u8.dtype != torch.uint8:
            raise RuntimeError(f"resize_img_device: expected uint8, got {img_u8.dtype}")
        _lib.require_contig("resize_img_device", img_u8)
        t = img_u8
    else:
        raise RuntimeError(f"resize_img_device: expected a numpy array or a tensor, "
                           f"got {type(img_u8).__name__}")
    if t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise RuntimeError("resize_img_device: expected [H,W,3] or [B,H,W,3], got "
                           f"{tuple(t.shape)}")
    if t.numel() == 0:
        raise RuntimeError(f"resize_img_device: empty input {tuple(t.shape)}")
    return t if t.dim() == 4 else t[None]


def _cuda_device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"resize_img_device runs on the GPU only, got device {dev}")
    return _lib._dev(dev)


def resize_img_device(img_u8, size, square_ok=False, return_transformation=False,
                      device="cuda", stream=None, undistort=None):
    """resize_img on the device.  img_u8: uint8 [H,W,3] or [B,H,W,3], numpy
    array or tensor, on the host or the device (a device tensor decides the
    device).  Returns resize_img's dict: img float32 [B,3,h,w] and
    unnormalized_img uint8 [B,h,w,3] ([h,w,3] for a 3-D input) on the device,
    true_shape np.int32 [[h, w]] * B; with return_transformation also its
    tuple.  The upload and the launch go to `stream` (default: the current
    stream); nothing waits for them.

    undistort: an intrinsics.Intrinsics (or UndistortMap).  The frame is then
    first undistorted on the device (s3u_remap, include/s3u.h: cv2.remap with
    the camera's maps) and the result ingested, both on `stream`; the input
    may then also be greyscale ([H,W], [H,W,1] or [B,H,W,1])."""
    if undistort is not None:
        src, batched = undistort.remap_device(img_u8, device, stream)
    else:
        src = _check_input(img_u8)
        batched = img_u8.ndim == 4
    dev = src.device if src.is_cuda else _cuda_device(device)
    B, in_h, in_w, _ = src.shape
    (W, H), filt, box, tr = ingest_geometry(in_h, in_w, size, square_ok)
    cw, ch = box[2] - box[0], box[3] - box[1]
    if cw <= 0 or ch <= 0:
        raise RuntimeError(f"resize_img_device: a {in_h}x{in_w} frame leaves an empty "
                           f"{ch}x{cw} crop at size {size}")
    resample = (W, H) != (in_w, in_h)       # PIL.Image.resize: same size is a copy
    hk = hb = vk = vb = None
    h_ks = v_ks = 0
    if resample and W != in_w:
        hk, hb = _device_tables(dev, in_w, W, filt)
        h_ks = hk.shape[1]
    if resample and H != in_h:
        vk, vb = _device_tables(dev, in_h, H, filt)
        v_ks = vk.shape[1]
    lut = _on_device(dev, "norm", norm_lut)
    L = _lib.lib()
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(st):
        if not src.is_cuda:
            src = src.to(dev, non_blocking=True)
        img = torch.empty((B, 3, ch, cw), dtype=torch.float32, device=dev)
        uimg = torch.empty((B, ch, cw, 3), dtype=torch.uint8, device=dev)
        ws = None
        if hk is not None and (_TWO_LAUNCH or
                               not L.s3i_fused_fits(in_h, in_w, h_ks, W, v_ks, H)):
            ws = torch.empty(L.s3i_workspace_bytes(B, in_h, W), dtype=torch.uint8, device=dev)
        _lib.call("s3i_ingest", src.data_ptr(), B, in_h, in_w,
                  _lib.ptr(hk), _lib.ptr(hb), h_ks, W, _lib.ptr(vk), _lib.ptr(vb), v_ks, H,
                  box[0], box[1], cw, ch, lut.data_ptr(), img.data_ptr(), uimg.data_ptr(),
                  _lib.ptr(ws), st.cuda_stream)
    res = dict(img=img, true_shape=np.int32([[ch, cw]] * B),
               unnormalized_img=uimg if batched else uimg[0])
    if return_transformation:
        return res, tr
    return res
