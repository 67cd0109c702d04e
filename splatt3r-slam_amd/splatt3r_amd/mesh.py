"""TSDF fusion and triangle-mesh extraction (include/s3f.h, csrc/tsdf_mesh.hip).

  TSDFVolume               a dense volume on the device: integrate depth maps
                           (s3f_integrate, a batch of views per launch),
                           extract the zero level set by marching tetrahedra
                           (s3f_mesh_count / s3f_mesh_emit)
  rasterizer_intrinsics    the pinhole the Gaussian rasterizer really renders
                           with (SharedGaussians.extract_mesh feeds it to the
                           fusion)

The reference has no counterpart in scope (its TSDF code lives in
mast3r/cloud_opt); the definition is include/s3f.h and
tests/tsdf_mesh_ref64.py restates it in float64.  There is no torch fallback.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from splatt3r_amd import _lib

# s3f.h: 7 nx ny nz < 2^31 (edge ids are 32-bit)
ABI_MAX_VOXELS = (2 ** 31 - 1) // 7


def _dims_for(extent, voxel: float):
    return tuple(int(math.ceil(max(float(e), 0.0) / voxel - 1e-9)) + 1 for e in extent)


def grid_for_bounds(lo, hi, voxel: float, max_voxels: Optional[int] = None):
    """(origin, dims) of the lattice of spacing `voxel` that covers the box
    lo..hi: origin = lo, ceil(extent / voxel) + 1 points per axis.  Raises
    ValueError, naming the voxel count and the smallest voxel size that would
    fit, when the lattice exceeds the ABI's limit (7 nx ny nz < 2^31) or
    max_voxels."""
    lo = [float(v) for v in lo]
    hi = [float(v) for v in hi]
    voxel = float(voxel)
    if not (math.isfinite(voxel) and voxel > 0):
        raise ValueError(f"voxel must be finite and > 0, got {voxel}")
    if not all(math.isfinite(v) for v in lo + hi) or any(h < l for l, h in zip(lo, hi)):
        raise ValueError(f"bad bounds {lo} .. {hi}")
    extent = [h - l for l, h in zip(lo, hi)]
    limit = ABI_MAX_VOXELS if max_voxels is None else min(int(max_voxels), ABI_MAX_VOXELS)
    dims = _dims_for(extent, voxel)
    count = dims[0] * dims[1] * dims[2]
    if count > limit:
        a, b = voxel, voxel
        while math.prod(_dims_for(extent, b)) > limit:      # grow to a size that fits
            a, b = b, b * 2
        for _ in range(60):                                  # bisect down to the smallest
            m = 0.5 * (a + b)
            if math.prod(_dims_for(extent, m)) > limit:
                a = m
            else:
                b = m
        raise ValueError(f"a {dims[0]} x {dims[1]} x {dims[2]} volume has {count} voxels, more "
                         f"than the {limit} allowed; the smallest voxel size that fits these "
                         f"bounds is {b:.6g}")
    return tuple(lo), dims


def rasterizer_intrinsics(settings) -> torch.Tensor:
    """The 3 x 3 pixel intrinsics a GaussianRasterizationSettings renders
    with.  The rasterizer does not see K: it projects through a symmetric
    frustum, ndc = x / (z tanfov) (the projection matrix of
    render.get_projection_matrix), and raster_math.hpp's ndc2pix puts pixel
    centres at ((ndc + 1) S - 1) / 2.  Hence, at integer pixel centres,
    fx = W / (2 tanfovx), fy = H / (2 tanfovy), cx = (W - 1) / 2,
    cy = (H - 1) / 2 (the principal-point offset of K is ignored, SURVEY
    A12)."""
    H, W = int(settings.image_height), int(settings.image_width)
    return torch.tensor([[W / (2.0 * float(settings.tanfovx)), 0.0, (W - 1) / 2.0],
                         [0.0, H / (2.0 * float(settings.tanfovy)), (H - 1) / 2.0],
                         [0.0, 0.0, 1.0]], dtype=torch.float32)


class TSDFVolume:
    """A dense truncated-signed-distance volume on the device.

    Give either `dims` = (nx, ny, nz) with `origin` (the world position of the
    centre of voxel (0, 0, 0)), or `bounds` = (lo, hi), an axis-aligned world
    box (grid_for_bounds).  `voxel` and `trunc` are in world units;
    trunc defaults to 4 voxels, the usual convention, and w_max to 64, a
    common choice; nobody has tuned either here.  Memory: 20 bytes a voxel
    (tsdf, weight, rgb), plus 6 a voxel while extract() runs."""

    def __init__(self, dims=None, voxel: float = None, bounds=None, origin=(0.0, 0.0, 0.0),
                 trunc: Optional[float] = None, w_max: float = 64.0, device="cuda",
                 max_voxels: Optional[int] = None):
        if voxel is None:
            raise ValueError("TSDFVolume: voxel is required")
        if (dims is None) == (bounds is None):
            raise ValueError("TSDFVolume: give exactly one of dims and bounds")
        voxel = float(voxel)
        if not (math.isfinite(voxel) and voxel > 0):
            raise ValueError(f"TSDFVolume: voxel must be finite and > 0, got {voxel}")
        if bounds is not None:
            origin, dims = grid_for_bounds(bounds[0], bounds[1], voxel, max_voxels)
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 1:
            raise ValueError(f"TSDFVolume: dims must be three positive integers, got {dims}")
        count = dims[0] * dims[1] * dims[2]
        limit = ABI_MAX_VOXELS if max_voxels is None else min(int(max_voxels), ABI_MAX_VOXELS)
        if count > limit:
            raise ValueError(f"TSDFVolume: {dims[0]} x {dims[1]} x {dims[2]} = {count} voxels, "
                             f"more than the {limit} allowed")
        trunc = 4.0 * voxel if trunc is None else float(trunc)
        w_max = float(w_max)
        for name, v in (("trunc", trunc), ("w_max", w_max)):
            if not (math.isfinite(v) and v > 0):
                raise ValueError(f"TSDFVolume: {name} must be finite and > 0, got {v}")
        self.dims = dims
        # the float32 values the kernels receive
        f32 = lambda v: float(np.float32(v))
        self.origin = tuple(f32(o) for o in origin)
        if len(self.origin) != 3 or not all(math.isfinite(o) for o in self.origin):
            raise ValueError(f"TSDFVolume: bad origin {origin}")
        self.voxel, self.trunc, self.w_max = f32(voxel), f32(trunc), f32(w_max)
        self.device = torch.device(device)
        nx, ny, nz = dims
        self.tsdf = torch.ones(nz, ny, nx, device=self.device)
        self.weight = torch.zeros(nz, ny, nx, device=self.device)
        self.rgb = torch.zeros(3, nz, ny, nx, device=self.device)
        self._ws = torch.empty(0, dtype=torch.float64, device=self.device)

    def reset(self):
        """Back to a fresh volume: tsdf = 1, weight = 0, rgb = 0."""
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        self.rgb.zero_()

    def _f32(self, name, t, shape):
        t = torch.as_tensor(t)
        if name != "T_WC":
            _lib.require_cuda(t)    # the maps: no silent host-to-device copy
        if t.numel() != math.prod(shape):
            raise ValueError(f"TSDFVolume.integrate: {name} has shape {tuple(t.shape)}, "
                             f"expected {tuple(shape)}")
        return t.to(self.device, torch.float32).reshape(shape).contiguous()

    def integrate(self, depth, T_WC, K, color=None, weight=None):
        """Fuse one view or a batch (s3f_integrate, one launch for the batch,
        the volume read and written once): depth [H, W] or [V, H, W] z-depth in
        camera units (0, negative and non-finite pixels are holes), T_WC
        [4, 4] or [V, 4, 4] camera-to-world similarities (s R | t), K [3, 3]
        (shared) or [V, 3, 3] pixel intrinsics with integer indices at pixel
        centres, color [3, H, W] or [V, 3, H, W] in [0, 1], weight [H, W] or
        [V, H, W] per-pixel weights (default 1).  Device tensors; runs on the
        current stream, no host read."""
        depth = torch.as_tensor(depth)
        if depth.dim() not in (2, 3):
            raise ValueError(f"TSDFVolume.integrate: depth must be [H, W] or [V, H, W], "
                             f"got {tuple(depth.shape)}")
        H, W = depth.shape[-2:]
        V = 1 if depth.dim() == 2 else depth.shape[0]
        if V == 0:
            return
        depth = self._f32("depth", depth, (V, H, W))
        T = self._f32("T_WC", T_WC, (V, 4, 4))
        K = torch.as_tensor(K).to(self.device, torch.float32)
        if K.numel() == 9:
            K = K.reshape(1, 3, 3).expand(V, 3, 3)
        K = K.reshape(V, 3, 3).contiguous()
        color = None if color is None else self._f32("color", color, (V, 3, H, W))
        wmap = None if weight is None else self._f32("weight", weight, (V, H, W))
        need = int(_lib.lib().s3f_integrate_workspace_bytes(V))
        if self._ws.numel() * 8 < need:
            self._ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            _lib.call("s3f_integrate", self.tsdf.data_ptr(), self.weight.data_ptr(),
                      self.rgb.data_ptr(), nx, ny, nz, *self.origin, self.voxel, self.trunc,
                      self.w_max, depth.data_ptr(), _lib.ptr(color), _lib.ptr(wmap), K.data_ptr(),
                      T.data_ptr(), V, H, W, self._ws.data_ptr(), self._ws.numel() * 8,
                      _lib.stream(self.device))

    def extract(self, w_min: float = 1.0):
        """The zero level set as a triangle mesh (marching tetrahedra over the
        cells whose 8 corners have weight >= w_min; the default 1.0, "every
        corner seen once at unit weight", is untuned).  Returns (verts [nv, 3]
        float32, colors [nv, 3] float32, faces [nt, 3] int32) on the device;
        an empty mesh has nv = nt = 0.  Two phases with one host read of the
        two counts in between; the scratch is freed on return."""
        nx, ny, nz = self.dims
        dev = self.device
        lib = _lib.lib()
        need = int(lib.s3f_mesh_workspace_bytes(nx, ny, nz))
        ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.call("s3f_mesh_count", self.tsdf.data_ptr(), self.weight.data_ptr(), nx, ny, nz,
                      float(w_min), counts.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                      _lib.stream(dev))
            nv, nt = counts.tolist()
            verts = torch.empty(nv, 3, device=dev)
            cols = torch.empty(nv, 3, device=dev)
            faces = torch.empty(nt, 3, dtype=torch.int32, device=dev)
            _lib.call("s3f_mesh_emit", self.tsdf.data_ptr(), self.rgb.data_ptr(), nx, ny, nz,
                      *self.origin, self.voxel, nv, nt, verts.data_ptr() if nv else None,
                      cols.data_ptr() if nv else None, faces.data_ptr() if nt else None, nv, nt,
                      ws.data_ptr(), ws.numel() * 8, _lib.stream(dev))
        return verts, cols, faces
