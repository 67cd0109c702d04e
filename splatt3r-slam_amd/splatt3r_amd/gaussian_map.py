"""World-space Gaussian map and its full-map render (SURVEY §8 A11 append /
A14, §8(f) f2).

  SharedGaussians          splatt3r_slam/frame.py:357-463
  should_append_gaussians  main.py:54-73
  render_map               splatt3r_slam/visualization.py:467-600
                           (_render_gs_interactive, minus the GL viewport)

The reference keeps the map in shared-memory torch tensors behind a
multiprocessing lock and appends with boolean-mask indexing; here the map is
a device structure-of-arrays with a device-side count (include/s3w.h
s3w_map): `append` takes the [n, 13] world records of
`splatt3r_utils.world_records` (or the 4-tuple of `gaussians_to_world`) and
runs the opacity filter, the FIFO half-eviction and the truncating copy as
three stream-ordered HIP launches with no host sync.  The map is the
all-gather target of the pair-batch shard (pairs.py): any rank can render
any view.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np
import torch

from splatt3r_amd import _abi, _lib
from splatt3r_amd import compact as _compact

S3wMap = _abi.structs["s3w_map"]    # include/s3w.h

# the viz clear colour (visualization.py:523-525)
VIZ_BG = (0.118, 0.137, 0.149)


class SharedGaussians:
    """frame.py:357-463 on the device: same fields, same append semantics."""

    def __init__(self, manager=None, max_gaussians: int = 4 * 1024 * 1024, device="cuda",
                 compact_voxel: Optional[float] = None, max_keyframes: int = 512):
        """max_keyframes: rows the anchor table starts with (`anchors`, the
        pose each keyframe's Gaussians are expressed under, all unset; it
        grows when a keyframe index exceeds it).  Nothing reads the table
        until `reanchor` is called.

        compact_voxel None: the reference's policy, a full map evicts its
        oldest half.  A voxel size (world units; nobody has tuned it): an
        append that could find the map full first merges the Gaussians that
        share a voxel (`compact`), and the eviction is left for a map that
        merging cannot shrink.  The object then keeps a host-side upper bound
        of its count (every append adds its n_max; clear, load_ply, refine,
        compact and n_gaussians make it exact), and an append compacts first
        when bound + n_max > max_gaussians and the bound has grown by at least
        max_gaussians // 8 since the last compaction's result (0 before the
        first; clear and load_ply put that back to 0): no host read until the
        map could be full, and no compaction per append of a map that stays
        full.  The bound never exceeds max_gaussians, so after a compaction
        that leaves more than 7/8 of max_gaussians the rule cannot be met
        again: the map then evicts as the reference does, also after the
        eviction has made room, until clear, load_ply or an explicit compact()
        with a smaller result."""
        del manager  # single process per GPU: no multiprocessing manager/lock
        self.max_gaussians = int(max_gaussians)
        if compact_voxel is not None:
            compact_voxel, _ = _compact.check_grid(compact_voxel, (0.0, 0.0, 0.0),
                                                   "SharedGaussians")
        self.compact_voxel = compact_voxel
        self.n_compactions = 0     # compact() calls that ran the merge
        self._bound = 0            # host upper bound of the count (compact_voxel only)
        self._compacted_to = 0     # the last compaction's result
        self.device = torch.device(device)
        cap = self.max_gaussians
        z = lambda *s, dt=torch.float32: torch.zeros(*s, device=self.device, dtype=dt)
        self.means = z(cap, 3)
        self.cov_triu = z(cap, 6)
        self.colors = z(cap, 3)
        self.opacities = z(cap)
        self.kf_id = z(cap, dt=torch.int32)
        self._n = z(1, dt=torch.int64)
        self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)
        # re-anchoring (include/s3a.h): the pose table, the per-keyframe
        # deltas' workspace, the {moved, held} counters
        self.anchors = z(max(1, int(max_keyframes)), 8)
        self._ws_anchor = torch.empty(0, dtype=torch.float64, device=self.device)
        self._tally = z(2, dt=torch.int64)
        self._c = S3wMap(self.means.data_ptr(), self.cov_triu.data_ptr(), self.colors.data_ptr(),
                         self.opacities.data_ptr(), self.kf_id.data_ptr(), self._n.data_ptr(),
                         cap)

    @property
    def n_gaussians(self) -> int:
        """Host read of the device count (synchronises the stream)."""
        n = int(self._n.item())
        self._bound = n
        return n

    def _workspace(self, n):
        need = int(_lib.lib().s3w_map_append_workspace_bytes(n))
        if self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def append_records(self, records: torch.Tensor, count: torch.Tensor, kf_idx: int,
                       opacity_threshold: float = 0.05):
        """records [n_max, 13] (means 3, cov_triu 6, colour 3, opacity),
        count: device int64 [1] of valid rows (s3w_gaussians_to_world)."""
        _lib.require_cuda(records, count)
        n_max = records.shape[0]
        if n_max == 0:
            return
        if self.compact_voxel is not None:
            if (self._bound + n_max > self.max_gaussians
                    and self._bound - self._compacted_to >= self.max_gaussians // 8):
                self.compact(self.compact_voxel)
            self._bound = min(self._bound + n_max, self.max_gaussians)
        records = records.float().contiguous()
        ws = self._workspace(n_max)
        _lib.call("s3w_map_append", ctypes.byref(self._c), records.data_ptr(), count.data_ptr(),
                  n_max, float(opacity_threshold), int(kf_idx), ws.data_ptr(),
                  _lib.stream(self.device))

    def append(self, means, cov_triu, colors, opacities, kf_idx: int,
               opacity_threshold: float = 0.05):
        """frame.py:388-443 with the reference's 4-tuple arguments."""
        n = means.shape[0]
        if n == 0:
            return
        rec = torch.cat([means.reshape(n, 3), cov_triu.reshape(n, 6), colors.reshape(n, 3),
                         opacities.reshape(n, 1)], 1).float().contiguous()
        cnt = torch.full((1,), n, dtype=torch.int64, device=rec.device)
        self.append_records(rec, cnt, kf_idx, opacity_threshold)

    def get_all(self):
        """(means, cov_triu, colors, opacities) sliced to [:n], or None."""
        n = self.n_gaussians
        if n == 0:
            return None
        return self.means[:n], self.cov_triu[:n], self.colors[:n], self.opacities[:n]

    def clear(self):
        self._n.zero_()
        self._bound = self._compacted_to = 0
        self.anchors.zero_()     # every keyframe unset

    # ---- re-anchoring (include/s3a.h) ----
    def _anchor_rows(self, n_kf: int):
        """The anchor table with at least n_kf rows (reallocate and copy)."""
        have = self.anchors.shape[0]
        if n_kf > have:
            grown = torch.zeros(max(n_kf, 2 * have), 8, device=self.device)
            grown[:have] = self.anchors
            self.anchors = grown
        return self.anchors

    def set_anchor(self, kf_idx: int, T_WC=None):
        """Record that the Gaussians labelled kf_idx are expressed under the
        pose T_WC (a lietorch.Sim3 of one pose or 8 floats [t, q xyzw, s]):
        one 8-float device copy.  None unsets the row."""
        kf_idx = int(kf_idx)
        if kf_idx < 0:
            raise ValueError(f"SharedGaussians.set_anchor: kf_idx {kf_idx} < 0")
        if T_WC is None:
            if kf_idx < self.anchors.shape[0]:
                self.anchors[kf_idx].zero_()
            return
        row = (T_WC.data if hasattr(T_WC, "data") and not torch.is_tensor(T_WC) else T_WC)
        row = torch.as_tensor(row, dtype=torch.float32).reshape(8)
        self._anchor_rows(kf_idx + 1)[kf_idx].copy_(row, non_blocking=True)

    def reanchor(self, poses, count: bool = False):
        """Move every Gaussian with its keyframe (s3a_map_reanchor): `poses`,
        [n_kf, 8] or a lietorch.Sim3 of n_kf poses, are the keyframes' current
        poses; a Gaussian labelled k < n_kf whose anchor row differs from
        poses[k] gets mu' = t_n + M (mu - t_o), Sigma' = M Sigma M^T with
        M = (s_n / s_o) R_n R_o^T, and the anchor rows take the poses.  An
        unset anchor adopts its pose and moves nothing; an invalid pose
        (non-finite, s <= 0, zero quaternion) holds its keyframe.  Colours,
        opacities, kf_id and the count are not written.  Two launches on the
        current stream.  count=True returns (rows moved, keyframes held), one
        host read; otherwise None and no host read."""
        rows = poses.data if hasattr(poses, "data") and not torch.is_tensor(poses) else poses
        rows = rows.reshape(-1, 8)
        _lib.require_cuda(rows)
        n_kf = rows.shape[0]
        if n_kf == 0:
            return (0, 0) if count else None
        rows = rows.to(self.device, torch.float32).contiguous()
        anchors = self._anchor_rows(n_kf)
        need = int(_lib.lib().s3a_reanchor_workspace_bytes(n_kf))
        if self._ws_anchor.numel() * 8 < need:
            self._ws_anchor = torch.empty((need + 7) // 8, dtype=torch.float64,
                                          device=self.device)
        tally = self._tally if count else None
        with torch.cuda.device(self.device):
            _lib.call("s3a_map_reanchor", ctypes.byref(self._c), anchors.data_ptr(),
                      rows.data_ptr(), n_kf, tally.data_ptr() if count else None,
                      tally[1:].data_ptr() if count else None, self._ws_anchor.data_ptr(),
                      self._ws_anchor.numel() * 8, _lib.stream(self.device))
        if count:
            moved, held = tally.tolist()
            return moved, held
        return None

    # ---- compaction (include/s3v.h, splatt3r_amd.compact) ----
    def compact(self, voxel: float, origin=(0.0, 0.0, 0.0)) -> int:
        """Merge the Gaussians whose centres share a voxel of side `voxel` on
        the grid through `origin`, in place: s3v_merge into scratch buffers,
        the five fields copied back, the device count set.  The map stays
        oldest-first and kf_id non-decreasing where it was (a merged Gaussian
        takes the place and the kf_id of its oldest member).  One host read,
        of the new count, which is returned; an empty map returns 0.

        The scratch (the five merged fields, s3v_merge's `first` and `group`,
        which it requires and this method does not use, and its workspace,
        about 110 bytes a row in all) is sized by the host bound of the count
        where the map keeps one (compact_voxel given).  Without one the count
        is known on the device only, so the scratch and the launch grids
        cover max_gaussians rows whatever the map holds (0.47 GB at the
        default 4 Mi; blocks past the count return at once), and an empty map
        is found empty by the pass, not before it.  The scratch is freed on
        return."""
        voxel, origin = _compact.check_grid(voxel, origin, "SharedGaussians.compact")
        # rows that may be live: the host bound where it is kept, else all
        n_max = self.max_gaussians
        if self.compact_voxel is not None:
            n_max = min(self._bound, n_max)
        if n_max == 0:
            return 0
        fields = (self.means, self.cov_triu, self.colors, self.opacities, self.kf_id)
        dev = self.device
        outs = tuple(torch.empty((n_max, *f.shape[1:]), device=dev, dtype=f.dtype)
                     for f in fields)
        first = torch.empty(n_max, device=dev, dtype=torch.int64)
        group = torch.empty(n_max, device=dev, dtype=torch.int64)
        tally = torch.zeros(2, device=dev, dtype=torch.int64)
        _compact.launch_merge(fields, self._n, n_max, voxel, origin, outs, first, group, tally,
                              _compact.workspace(n_max, dev))
        m = int(tally[0].item())
        for f, o in zip(fields, outs):
            f[:m] = o[:m]
        self._n.copy_(tally[:1])
        self.n_compactions += 1
        self._bound = self._compacted_to = m
        return m

    # ---- floaters and plain point clouds (include/s3k.h, splatt3r_amd.nn) ----
    def remove_outliers(self, k: int = 16, std_ratio: float = 2.0, cell=None) -> int:
        """Remove the Gaussians whose centre lies far from its neighbours
        (nn.outlier_mask over means[:n]: the mean distance to the k nearest
        other centres exceeds the map's mean by std_ratio sample standard
        deviations), in place: the survivors of the five fields move down in
        their order (gathered into scratch, copied back, as compact() copies
        back), the device count is set, and the host bound and the last
        compaction's result are lowered to it.  `anchors` is untouched.  k
        and std_ratio are the customary values of statistical outlier
        removal, not tuned here; cell is the search grid's cell size (default:
        nn.default_grid).  Two host reads of its own, the count before and
        the survivors after (the search grid's bounding box is a third,
        nn.default_grid).  Returns the rows removed; an empty map returns 0."""
        from splatt3r_amd import nn
        n = self.n_gaussians
        if n == 0:
            return 0
        keep = nn.outlier_mask(self.means[:n], k, std_ratio, cell)
        src = keep.nonzero().squeeze(1)
        m = src.numel()
        for f in (self.means, self.cov_triu, self.colors, self.opacities, self.kf_id):
            f[:m] = f[:n][src]
        self._n.fill_(m)
        self._bound = m
        self._compacted_to = min(self._compacted_to, m)
        return n - m

    def load_points(self, points, colors, kf_idx: int = -1, k: int = 3, opacity: float = 0.1,
                    scale_min: float = 1e-7) -> int:
        """Replace the map's content by a plain point cloud (a saved
        reconstruction, a ground-truth scan, evaluate.load_ply's result):
        points [n, 3] float32 and colors [n, 3] in [0, 1], device tensors.
        Every point becomes an isotropic Gaussian as 3DGS initialises one
        from a point cloud: covariance max(s, scale_min) I with s the mean
        squared distance to its k nearest other points (nn.knn_scale; a point
        with no neighbour takes scale_min), the given opacity and kf_id =
        kf_idx.  Rows with a non-finite coordinate are dropped, and the first
        max_gaussians of the rest are taken.  Returns the count."""
        from splatt3r_amd import nn
        fn = "SharedGaussians.load_points"
        points = nn._points(points, "points", fn)
        if not torch.is_tensor(colors) or colors.shape != points.shape:
            raise ValueError(f"{fn}: colors must be a tensor of points' shape "
                             f"{tuple(points.shape)}")
        _lib.require_cuda(colors)
        ok = torch.isfinite(points).all(1)
        points = points[ok][:self.max_gaussians].contiguous()
        colors = colors[ok][:self.max_gaussians].float()
        n = points.shape[0]
        self.clear()
        if n == 0:
            return 0
        var = nn.knn_scale(points, k)
        floor = torch.full_like(var[:1], float(scale_min))         # scale_min as a float32
        var = torch.maximum(torch.where(torch.isfinite(var), var, floor), floor)
        self.means[:n] = points
        self.cov_triu[:n] = 0.0
        for col in (0, 3, 5):                      # xx, yy, zz
            self.cov_triu[:n, col] = var
        self.colors[:n] = colors
        self.opacities[:n] = float(opacity)
        self.kf_id[:n] = int(kf_idx)
        self._n.fill_(n)
        self._bound = n
        return n

    # ---- 3DGS splat .ply (include/s3w.h, evaluate.write_splat_ply) ----
    def to_splats(self, n: Optional[int] = None, scale_min: float = 1e-7) -> torch.Tensor:
        """The first n Gaussians (default: all, a host read of the count) as
        [n, 17] splat rows on the device.  With an explicit n there is no
        host read; rows at and past the map's count are then left zero."""
        if n is None:
            n = self.n_gaussians
            rows = torch.empty(n, 17, device=self.device)
        else:
            n = min(int(n), self.max_gaussians)
            rows = torch.zeros(n, 17, device=self.device)
        _lib.call("s3w_map_to_splats", self.means.data_ptr(), self.cov_triu.data_ptr(),
                  self.colors.data_ptr(), self.opacities.data_ptr(), self._n.data_ptr(), n,
                  float(scale_min), rows.data_ptr(), _lib.stream(self.device))
        return rows

    def save_ply(self, path) -> int:
        """Write the map as a binary splat .ply: one kernel, one device-to-host
        copy of the [n, 17] block, one file write.  Returns n."""
        from splatt3r_amd.evaluate import write_splat_ply
        rows = self.to_splats().cpu().numpy()
        write_splat_ply(path, rows)
        return len(rows)

    def load_ply(self, path, kf_idx: int = -1) -> int:
        """Replace the map's content by a splat .ply (this project's or one
        trained elsewhere; DC colour only, `f_rest_*` ignored).  Every
        Gaussian gets kf_id = kf_idx.  Raises ValueError, leaving the map
        untouched, if the file holds more than max_gaussians.  Returns n."""
        from splatt3r_amd.evaluate import SPLAT_REQUIRED, read_splat_ply
        props = read_splat_ply(path)
        rows14 = np.stack([props[p] for p in SPLAT_REQUIRED], 1).astype(np.float32)
        n = len(rows14)
        if n > self.max_gaussians:
            raise ValueError(f"{path} holds {n} Gaussians, the map at most {self.max_gaussians}")
        dev_rows = torch.from_numpy(np.ascontiguousarray(rows14)).to(self.device)
        _lib.call("s3w_map_from_splats", ctypes.byref(self._c), dev_rows.data_ptr() if n else None,
                  n, int(kf_idx), _lib.stream(self.device))
        self._bound, self._compacted_to = n, 0
        return n

    # ---- photometric refinement (include/s3o.h, splatt3r_amd.refine) ----
    def refine(self, images, T_WC, K, iters, density=None, **kw):
        """Fit the map to `images` ([V, 3, H, W] in [0, 1]) seen from `T_WC`
        ([V, 4, 4] camera-to-world) with intrinsics `K`: to_splats,
        refine.refine_splats (which takes **kw), s3w_map_from_splats.

        density None: the count and every Gaussian's kf_id are kept.  With a
        refine.DensityControl (its capacity defaults to max_gaussians) the
        passes prune, clone and split: the count becomes the number of rows
        left, and every row takes the kf_id of the Gaussian density.origin
        traces it to, so children inherit and, rows keeping their order, kf_id
        stays non-decreasing where it was.

        A surviving Gaussian whose row no step touched (outside every view's
        frustum, with the default sparse step) keeps its fields bit for bit:
        the row round trip is not bit-exact, so its result is taken only where
        the row differs from the row it started as.
        Returns the per-step losses (device tensor [iters]), or None for an
        empty map."""
        from splatt3r_amd.refine import refine_splats
        n = self.n_gaussians
        if n == 0:
            return None
        if density is not None:
            if density.capacity is None:
                density.capacity = self.max_gaussians
            if density.capacity > self.max_gaussians:
                raise ValueError(f"SharedGaussians.refine: density capacity {density.capacity} "
                                 f"exceeds max_gaussians {self.max_gaussians}")
        rows17 = self.to_splats(n)
        before = torch.cat([rows17[:, :3], rows17[:, 6:]], 1).contiguous()
        rows14, history = refine_splats(before, images, T_WC, K, iters, density=density, **kw)
        m = rows14.shape[0]
        fields = (self.means, self.cov_triu, self.colors, self.opacities, self.kf_id)
        if density is None:
            changed = (rows14 != before).any(1)
            old = [f[:n].clone() for f in fields]
        else:
            # the Gaussian each row started as (itself, or its ancestor)
            origin = density.origin
            src = torch.where(origin >= 0, origin, ~origin).long()
            changed = (origin < 0) | (rows14 != before[src]).any(1)
            old = [f[:n][src] for f in fields]
        # s3w_map_from_splats overwrites kf_id and sets the count
        _lib.call("s3w_map_from_splats", ctypes.byref(self._c), rows14.data_ptr() if m else None,
                  m, -1, _lib.stream(self.device))
        for f, o in zip(fields[:4], old):
            keep = changed if f.dim() == 1 else changed[:, None]
            f[:m] = torch.where(keep, f[:m], o)
        self.kf_id[:m] = old[4]
        self._bound = m
        return history

    def refine_pose(self, image, T_WC, K, iters, near: float = 0.1, **kw):
        """Localise one view against the map: fit the camera-to-world pose
        `T_WC` [4, 4] to `image` ([3, H, W] in [0, 1]) with intrinsics `K`,
        the map rendered as render_map feeds the rasterizer (s3w_map_scale,
        cov3D_precomp, colors_precomp) and the pose gradient taken in its
        covariance form (refine.localise, which takes **kw: poses, mask, the
        loss weights, far, bg).  The map is read only: its five fields keep
        their bits.  Returns (T_WC float64 [4, 4] on the device, the per-step
        losses [iters]), or None for an empty map."""
        from splatt3r_amd.refine import localise
        n = self.n_gaussians
        if n == 0:
            return None
        s = float(1 / torch.full((1,), float(near)))   # camera_settings' float32 factor
        sc_means = torch.empty(n, 3, device=self.device)
        sc_cov = torch.empty(n, 6, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("s3w_map_scale", self.means.data_ptr(), self.cov_triu.data_ptr(),
                      self._n.data_ptr(), n, s, s * s, sc_means.data_ptr(), sc_cov.data_ptr(),
                      _lib.stream(self.device))
        return localise(sc_means, sc_cov, self.colors[:n], self.opacities[:n, None], image, T_WC, K,
                        iters, near=near, **kw)

    # ---- surface extraction (include/s3f.h, splatt3r_amd.mesh) ----
    @torch.no_grad()
    def render_depths(self, T_WC, K, H, W, alpha_min: float = 0.5, near: float = 0.1,
                      far: float = 1000.0, n: Optional[int] = None):
        """What extract_mesh fuses: the map rendered from the V camera-to-world
        poses T_WC [V, 4, 4] as refine_pose and render_map feed the rasterizer
        (s3w_map_scale, cov3D_precomp, colors_precomp, the cameras of
        refine._cameras, return_depth=True).  Returns (depth [V, H, W] in each
        view's camera units: depth / alpha where alpha >= alpha_min, else 0,
        with the scale-invariant factor undone; color [V, 3, H, W] clamped to
        [0, 1]; K_r [3, 3], the rasterizer's own pinhole,
        mesh.rasterizer_intrinsics), or None for an empty map."""
        from diff_gaussian_rasterization import GaussianRasterizer
        from splatt3r_amd.mesh import rasterizer_intrinsics
        from splatt3r_amd.refine import _cameras
        if n is None:
            n = self.n_gaussians
        if n == 0:
            return None
        dev = self.device
        T_WC = torch.as_tensor(T_WC).reshape(-1, 4, 4)
        with torch.cuda.device(dev):
            settings, s = _cameras(T_WC, K, H, W, near, far, None, dev)
            sc_means = torch.empty(n, 3, device=dev)
            sc_cov = torch.empty(n, 6, device=dev)
            _lib.call("s3w_map_scale", self.means.data_ptr(), self.cov_triu.data_ptr(),
                      self._n.data_ptr(), n, s, s * s, sc_means.data_ptr(), sc_cov.data_ptr(),
                      _lib.stream(dev))
            depths, colors = [], []
            for st in settings:
                out = GaussianRasterizer(st)(
                    means3D=sc_means, means2D=torch.zeros_like(sc_means), shs=None,
                    colors_precomp=self.colors[:n], opacities=self.opacities[:n, None],
                    cov3D_precomp=sc_cov, return_depth=True)
                depth, alpha = out[2], out[3]
                depths.append(torch.where(alpha >= alpha_min, depth / alpha,
                                          torch.zeros_like(depth)) / s)
                colors.append(out[0].clamp(0, 1))
            return (torch.stack(depths).contiguous(), torch.stack(colors).contiguous(),
                    rasterizer_intrinsics(settings[0]))

    @torch.no_grad()
    def render_depth_alpha(self, T_WC, K, H, W, near: float = 0.1, far: float = 1000.0,
                           n: Optional[int] = None):
        """render_depths' render without its division and threshold, for
        splatt3r_amd.depth: (depth [V, H, W] = sum z alpha T with the
        scale-invariant factor undone, i.e. in each view's camera units, alpha
        [V, H, W] = sum alpha T), or None for an empty map.  depth / alpha is
        the expected depth where alpha is large enough to trust."""
        from diff_gaussian_rasterization import GaussianRasterizer
        from splatt3r_amd.refine import _cameras
        if n is None:
            n = self.n_gaussians
        if n == 0:
            return None
        dev = self.device
        T_WC = torch.as_tensor(T_WC).reshape(-1, 4, 4)
        with torch.cuda.device(dev):
            settings, s = _cameras(T_WC, K, H, W, near, far, None, dev)
            sc_means = torch.empty(n, 3, device=dev)
            sc_cov = torch.empty(n, 6, device=dev)
            _lib.call("s3w_map_scale", self.means.data_ptr(), self.cov_triu.data_ptr(),
                      self._n.data_ptr(), n, s, s * s, sc_means.data_ptr(), sc_cov.data_ptr(),
                      _lib.stream(dev))
            depths, alphas = [], []
            for st in settings:
                out = GaussianRasterizer(st)(
                    means3D=sc_means, means2D=torch.zeros_like(sc_means), shs=None,
                    colors_precomp=self.colors[:n], opacities=self.opacities[:n, None],
                    cov3D_precomp=sc_cov, return_depth=True)
                depths.append(out[2] / s)
                alphas.append(out[3])
            return torch.stack(depths).contiguous(), torch.stack(alphas).contiguous()

    @torch.no_grad()
    def extract_mesh(self, T_WC, K, H, W, voxel, bounds=None, alpha_min: float = 0.5,
                     near: float = 0.1, far: float = 1000.0, w_min: float = 1.0,
                     view_batch: int = 16, **volume_kw):
        """A triangle mesh of the map's surface: depth and colour rendered
        from the map at the views T_WC [V, 4, 4] (camera-to-world (s R | t),
        intrinsics K, H x W; render_depths), fused into a mesh.TSDFVolume of
        spacing `voxel` (view_batch views per launch) and extracted by
        marching tetrahedra.  The fusion projects with the rasterizer's own
        pinhole, not K (mesh.rasterizer_intrinsics).

        bounds None: the axis-aligned box of the map's means (one host read),
        padded by the truncation distance.  A box that needs more voxels than
        the ABI's limit or `max_voxels` (a volume_kw, like trunc and w_max)
        raises ValueError naming the count and the smallest voxel that fits.
        The map is read only: its five fields keep their bits.  Returns
        (verts [nv, 3], colors [nv, 3] in [0, 1], faces [nt, 3] int32) on the
        device, or None for an empty map or no view."""
        from splatt3r_amd.mesh import TSDFVolume
        n = self.n_gaussians
        T_WC = torch.as_tensor(T_WC).reshape(-1, 4, 4)
        if n == 0 or T_WC.shape[0] == 0:
            return None
        voxel = float(voxel)
        trunc = float(volume_kw.get("trunc") or 4.0 * voxel)
        if bounds is None:
            lo, hi = torch.aminmax(self.means[:n], dim=0)
            lo, hi = torch.stack([lo, hi]).tolist()
            bounds = ([v - trunc for v in lo], [v + trunc for v in hi])
        with torch.cuda.device(self.device):
            vol = TSDFVolume(bounds=bounds, voxel=voxel, device=self.device, **volume_kw)
            step = max(1, int(view_batch))
            for a in range(0, T_WC.shape[0], step):
                depth, color, K_r = self.render_depths(T_WC[a:a + step], K, H, W, alpha_min, near,
                                                       far, n=n)
                vol.integrate(depth, T_WC[a:a + step], K_r, color=color)
            return vol.extract(w_min=w_min)


def splats_from_cov(means, cov_triu, colors, opacities, scale_min: float = 1e-7) -> torch.Tensor:
    """[n, 17] splat rows (include/s3w.h s3w_map_to_splats) of n Gaussians
    given as device tensors: means [n, 3], cov_triu [n, 6], colors [n, 3],
    opacities [n] or [n, 1]."""
    _lib.require_cuda(means, cov_triu, colors, opacities)
    n = means.shape[0]
    prep = lambda t, w: t.reshape(n, w).float().contiguous()
    means, cov_triu, colors, opacities = (prep(means, 3), prep(cov_triu, 6), prep(colors, 3),
                                          prep(opacities, 1))
    rows = torch.empty(n, 17, device=means.device)
    with torch.cuda.device(means.device):
        _lib.call("s3w_map_to_splats", means.data_ptr(), cov_triu.data_ptr(), colors.data_ptr(),
                  opacities.data_ptr(), None, n, float(scale_min), rows.data_ptr(),
                  _lib.stream(means.device))
    return rows


def should_append_gaussians(add_new_kf: bool, frame_idx: int, current_T_WC,
                            last_append_T_WC, last_append_frame_idx: int,
                            min_translation: float, min_frame_gap: int) -> bool:
    """main.py:54-73."""
    if add_new_kf:
        return True
    if last_append_T_WC is None:
        return True
    if (frame_idx - last_append_frame_idx) < min_frame_gap:
        return False
    t_cur = current_T_WC.matrix()[0, :3, 3]
    t_last = last_append_T_WC.matrix()[0, :3, 3]
    return torch.linalg.norm(t_cur - t_last).item() >= min_translation


def viz_camera(T_WC_cv: np.ndarray, render_w: int, render_h: int, vfov_deg: float,
               near: float = 0.05, far: float = 100.0):
    """The camera of _render_gs_interactive (visualization.py:490-561) for an
    OpenCV camera-to-world pose: returns (tanfovx, tanfovy, viewmatrix,
    projmatrix, campos, scale) with the scale-invariant factor 1/near, using
    the same torch ops as the reference (get_fov, get_projection_matrix).
    Host tensors; `render_map` moves them to the device."""
    from splatt3r_amd.render import get_fov, get_projection_matrix
    vfov_rad = math.radians(vfov_deg)
    fy = render_h / (2.0 * math.tan(vfov_rad / 2.0))
    fx = fy
    cx, cy = render_w / 2.0, render_h / 2.0
    K_norm = torch.tensor([[fx / render_w, 0, cx / render_w], [0, fy / render_h, cy / render_h],
                           [0, 0, 1]], dtype=torch.float32).unsqueeze(0)
    near_t = torch.tensor([near], dtype=torch.float32)
    far_t = torch.tensor([far], dtype=torch.float32)
    fov_xy = get_fov(K_norm)
    fov_x, fov_y = fov_xy[0, 0], fov_xy[0, 1]
    tan_fov_x = (0.5 * fov_x).tan().item()
    tan_fov_y = (0.5 * fov_y).tan().item()
    inv_near = 1.0 / near_t
    ext = torch.from_numpy(np.asarray(T_WC_cv, np.float32)).unsqueeze(0).clone()
    ext[..., :3, 3] *= inv_near[:, None]
    proj = get_projection_matrix(near_t * inv_near, far_t * inv_near, fov_x.unsqueeze(0),
                                 fov_y.unsqueeze(0))
    proj_t = proj[0].T
    view_t = ext[0].inverse().T
    full_proj = view_t @ proj_t
    return (tan_fov_x, tan_fov_y, view_t.contiguous(), full_proj.contiguous(),
            ext[0, :3, 3].contiguous(), inv_near.item(), (inv_near ** 2).item())


def gl_to_cv_T_WC(T_CW_gl: np.ndarray) -> np.ndarray:
    """visualization.py:490-499: OpenGL world-to-camera -> OpenCV
    camera-to-world."""
    cv2gl = np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)
    return np.linalg.inv(cv2gl @ np.asarray(T_CW_gl, np.float32))


@torch.inference_mode()
def render_map(gmap: SharedGaussians, T_WC_cv: np.ndarray, render_w: int, render_h: int,
               vfov_deg: float, bg=VIZ_BG, n: Optional[int] = None, clamp: bool = True,
               camera=None, return_depth=False):
    """Full-map render (visualization.py:467-600): every Gaussian of the map
    rasterized with colors_precomp from an OpenCV camera-to-world pose.
    Returns the [3, H, W] image (clamped to [0, 1] like the viz when clamp);
    with return_depth, (image, depth [H, W], alpha [H, W]) from the same
    blend pass: depth = sum z_i alpha_i T_i in world units, alpha =
    sum alpha_i T_i (neither is clamped).
    `camera`: a precomputed viz_camera tuple (the host camera math is torch
    CPU code whose last bit depends on the host's vector ISA)."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    dev = gmap.device
    if n is None:
        n = gmap.n_gaussians
    if n == 0:
        return None
    tx, ty, view_t, full_proj, campos, s, s2 = (
        camera if camera is not None else viz_camera(T_WC_cv, render_w, render_h, vfov_deg))
    sc_means = torch.empty(n, 3, device=dev)
    sc_cov = torch.empty(n, 6, device=dev)
    _lib.call("s3w_map_scale", gmap.means.data_ptr(), gmap.cov_triu.data_ptr(),
              gmap._n.data_ptr(), n, float(s), float(s2), sc_means.data_ptr(), sc_cov.data_ptr(),
              _lib.stream(dev))
    st = GaussianRasterizationSettings(
        image_height=render_h, image_width=render_w, tanfovx=tx, tanfovy=ty,
        bg=torch.tensor(bg, dtype=torch.float32, device=dev), scale_modifier=1.0,
        viewmatrix=view_t.to(dev), projmatrix=full_proj.to(dev), sh_degree=0,
        campos=campos.to(dev), prefiltered=False, debug=False)
    out = GaussianRasterizer(st)(means3D=sc_means, means2D=torch.zeros_like(sc_means),
                                 shs=None, colors_precomp=gmap.colors[:n],
                                 opacities=gmap.opacities[:n, None],
                                 cov3D_precomp=sc_cov, return_depth=return_depth)
    image = out[0].clamp(0, 1) if clamp else out[0]
    if return_depth:
        # the rasterizer ran on means * s: depth back in world units
        return image, out[2] / float(s), out[3]
    return image
