"""Exact nearest neighbour on the device, distance statistics and area-uniform
mesh sampling (include/s3k.h, csrc/nn_search.hip): what the geometry scores of
evaluate.eval_reconstruction are reductions of.

  PointGrid     a uniform grid over reference points; .query(q) -> (idx, dist),
                .knn(q, k) -> the k nearest rows and their mean distances
  nearest, knn  build a grid and query it once
  knn_scale     mean squared distance to the k nearest other points (3DGS's
                point-cloud initialisation)
  outlier_mask  statistical outlier removal (map floaters)
  dist_stats    count, sum, sum of squares, count within a threshold, maximum
  sample_mesh   stratified area-uniform samples of a triangle mesh

The result of a query is bit for bit that of a scan of every reference row
(smallest squared distance in double, ties to the smallest index), whatever
the grid.  The reference has no counterpart.  The default cell size,
2 (volume / n)^(1/3), is a starting point nobody has tuned.

Importing this module does not initialise the GPU.
"""
from __future__ import annotations

import ctypes
import math

import torch

from splatt3r_amd import _abi, _lib

MAX_CELLS = _abi.constants["S3K_MAX_CELLS"]
MAX_K = _abi.constants["S3K_MAX_K"]
KNN_OUTPUTS = ("idx", "dist", "mean", "mean_sq")     # s3k_knn's order


def _points(t, name: str, fn: str) -> torch.Tensor:
    """t as a contiguous float32 device tensor [n, 3]; raises otherwise."""
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{fn}: {name} must be a tensor of shape [n, 3]")
    if t.dtype != torch.float32:
        raise TypeError(f"{fn}: {name} must be float32, got {t.dtype}")
    _lib.require_cuda(t)
    return t.contiguous()


def _bytes(n: int, device) -> torch.Tensor:
    # at least one byte: a data pointer the ABI's null checks accept
    return torch.empty(max(int(n), 1), device=device, dtype=torch.uint8)


def default_grid(ref: torch.Tensor, cell=None, max_cells: int = 1 << 24):
    """(origin, cell, dims) of the grid PointGrid builds over ref: origin the
    bounding-box minimum of the finite rows, cell 2 (volume / n)^(1/3) unless
    given (over the axes with an extent; 1 when there is none), doubled until
    the dims fit max_cells.  One host read of six numbers."""
    max_cells = int(max_cells)
    if not 1 <= max_cells <= MAX_CELLS:
        raise ValueError(f"PointGrid: max_cells must be in [1, 2^27], got {max_cells}")
    if cell is not None:
        cell = float(cell)
        if not (cell > 0.0 and math.isfinite(cell)):
            raise ValueError(f"PointGrid: cell must be > 0 and finite, got {cell}")
    ok = torch.isfinite(ref).all(1)
    n = int(ok.sum())
    if n == 0:
        return (0.0, 0.0, 0.0), 1.0 if cell is None else cell, (1, 1, 1)
    kept = ref[ok].double()
    lo, hi = kept.min(0).values.tolist(), kept.max(0).values.tolist()
    ext = [h - l for l, h in zip(lo, hi)]
    if cell is None:
        live = [e for e in ext if e > 0.0]
        cell = 2.0 * (math.prod(live) / n) ** (1.0 / len(live)) if live else 1.0
        if not (cell > 0.0 and math.isfinite(cell)):
            cell = max(live) if live and math.isfinite(max(live)) else 1.0
    while True:
        # the quotient is clamped as a float: a huge extent over a tiny cell is inf
        dims = tuple(int(min(math.floor(min(e / cell, float(MAX_CELLS))) + 1, MAX_CELLS))
                     for e in ext)
        if dims[0] * dims[1] * dims[2] <= max_cells:
            return tuple(lo), cell, dims
        cell *= 2.0


class PointGrid:
    """A uniform grid over ref [n, 3] (float32 device tensor, n < 2^31) for
    exact nearest-neighbour queries.  cell: the cell size (default: see
    default_grid); origin and dims may be given too (then nothing is read
    back).  `dropped` is a device int64 scalar: the rows left out because a
    coordinate was not finite."""

    def __init__(self, ref, cell=None, max_cells: int = 1 << 24, origin=None, dims=None):
        fn = "PointGrid"
        self.ref = _points(ref, "ref", fn)
        dev = self.ref.device
        if origin is None or dims is None:
            if origin is not None or dims is not None:
                raise ValueError(f"{fn}: give origin and dims together, with cell")
            origin, cell, dims = default_grid(self.ref, cell, max_cells)
        elif cell is None:
            raise ValueError(f"{fn}: origin and dims need cell")
        self.origin = tuple(float(v) for v in origin)
        self.cell = float(cell)
        self.dims = tuple(int(v) for v in dims)
        if len(self.origin) != 3 or len(self.dims) != 3:
            raise ValueError(f"{fn}: origin and dims must have three entries")
        self.n = self.ref.shape[0]
        self._org = (ctypes.c_double * 3)(*self.origin)
        need = int(_lib.lib().s3k_grid_workspace_bytes(self.n, *self.dims))
        self._grid = _bytes(need, dev)
        self._dropped = torch.zeros(1, device=dev, dtype=torch.int64)
        with torch.cuda.device(dev):
            _lib.call("s3k_grid_build", self.ref.data_ptr() if self.n else None, self.n, self._org,
                      self.cell, *self.dims, self._grid.data_ptr(), self._grid.numel(),
                      self._dropped.data_ptr(), _lib.stream(dev))
        self.dropped = self._dropped[0]

    @torch.no_grad()
    def query(self, q, max_dist: float = math.inf):
        """(idx [m] int32, dist [m] float32) of the nearest reference row of
        every row of q [m, 3]; only rows within max_dist count.  idx -1 and
        dist +inf where there is none or the query row is not finite."""
        fn = "PointGrid.query"
        q = _points(q, "q", fn)
        if q.device != self.ref.device:
            raise ValueError(f"{fn}: q is on {q.device}, the grid on {self.ref.device}")
        max_dist = float(max_dist)
        if not max_dist >= 0.0:
            raise ValueError(f"{fn}: max_dist must be >= 0 or +inf, got {max_dist}")
        dev, m = q.device, q.shape[0]
        idx = torch.empty(m, device=dev, dtype=torch.int32)
        dist = torch.empty(m, device=dev, dtype=torch.float32)
        ws = _bytes(int(_lib.lib().s3k_query_workspace_bytes(m)), dev)
        with torch.cuda.device(dev):
            _lib.call("s3k_query", self._grid.data_ptr(), self._grid.numel(), self.n, self._org,
                      self.cell, *self.dims, q.data_ptr() if m else None, m, max_dist,
                      idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream(dev))
        return idx, dist

    @torch.no_grad()
    def knn(self, q, k: int, max_dist: float = math.inf, exclude_self: bool = False,
            want=("idx", "dist")) -> dict:
        """The k nearest reference rows (1 <= k <= 32) of every row of q
        [m, 3], in ascending (distance, index) order; only rows within
        max_dist count.  Returns a dict of the outputs named in `want`
        (KNN_OUTPUTS): idx [m, k] int32 and dist [m, k] float32 (-1 and +inf
        in the slots past the last neighbour), mean and mean_sq [m] float32
        (the mean distance and mean squared distance to the neighbours found,
        +inf when there is none).  An output not asked for is not written.
        exclude_self: q is the grid's own points, and row j is not its own
        neighbour (by index; needs m <= n)."""
        fn = "PointGrid.knn"
        q = _points(q, "q", fn)
        if q.device != self.ref.device:
            raise ValueError(f"{fn}: q is on {q.device}, the grid on {self.ref.device}")
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"{fn}: k must be in 1 .. {MAX_K}, got {k}")
        max_dist = float(max_dist)
        if not max_dist >= 0.0:
            raise ValueError(f"{fn}: max_dist must be >= 0 or +inf, got {max_dist}")
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(w not in KNN_OUTPUTS for w in want):
            raise ValueError(f"{fn}: want must name at least one of {KNN_OUTPUTS}, got {want}")
        dev, m = q.device, q.shape[0]
        if exclude_self and m > self.n:
            raise ValueError(f"{fn}: exclude_self with {m} queries for {self.n} rows")
        out = {}
        for name in KNN_OUTPUTS:
            if name in want:
                shape = (m, k) if name in ("idx", "dist") else (m,)
                out[name] = torch.empty(shape, device=dev, dtype=torch.int32 if name == "idx"
                                        else torch.float32)
        if m == 0:              # empty tensors have no address to pass
            return {name: out[name] for name in want}
        ptrs = [out[name].data_ptr() if name in out else None for name in KNN_OUTPUTS]
        ws = _bytes(int(_lib.lib().s3k_knn_workspace_bytes(m)), dev)
        with torch.cuda.device(dev):
            _lib.call("s3k_knn", self._grid.data_ptr(), self._grid.numel(), self.n, self._org,
                      self.cell, *self.dims, q.data_ptr() if m else None, m, k,
                      1 if exclude_self else 0, max_dist, *ptrs, ws.data_ptr(), ws.numel(),
                      _lib.stream(dev))
        return {name: out[name] for name in want}


QUERY_MODES = {"sorted": 0, "unsorted": 1, "wave": 2}


def set_query_mode(mode: str = "sorted") -> None:
    """How PointGrid.query walks from now on, process-wide (measurements only:
    every mode returns the same bits): "sorted" (queries in cell order, one
    thread each; the default), "unsorted" (their own order) or "wave" (cell
    order, one wave per query)."""
    _lib.lib().s3k_set_query_mode(QUERY_MODES[mode])


def nearest(q, ref, max_dist: float = math.inf, **kw):
    """PointGrid(ref, **kw).query(q, max_dist)."""
    return PointGrid(ref, **kw).query(q, max_dist)


def knn(q, ref, k: int, max_dist: float = math.inf, exclude_self: bool = False,
        want=("idx", "dist"), **kw) -> dict:
    """PointGrid(ref, **kw).knn(q, k, max_dist, exclude_self, want)."""
    return PointGrid(ref, **kw).knn(q, k, max_dist, exclude_self, want)


def knn_scale(points, k: int = 3, **kw) -> torch.Tensor:
    """[n] float32: every point's mean squared distance to its k nearest other
    points, what 3DGS's point-cloud initialisation takes as a Gaussian's
    squared scale (simple_knn.distCUDA2, k = 3).  +inf for a point with no
    neighbour.  simple-knn is no dependency of this project: the two follow
    the same definition, but their parity is not pinned by any test."""
    return PointGrid(points, **kw).knn(points, k, exclude_self=True, want=("mean_sq",))["mean_sq"]


@torch.no_grad()
def outlier_mask(points, k: int = 16, std_ratio: float = 2.0, cell=None) -> torch.Tensor:
    """Statistical outlier removal: keep [n] bool, True for the points to keep.
    With d_i the mean distance of point i to its k nearest other points and
    mu, sigma the mean and the sample standard deviation (c - 1) of the
    finite d_i, a point is kept when d_i <= mu + std_ratio sigma; a point
    with a non-finite coordinate is never kept.  With fewer than two finite
    d_i every finite point is kept.

    The search is s3k_knn; the threshold is a few torch ops in double on the
    device from dist_stats' sums (mu = S1 / c, var = max(0, S2 - S1 mu) /
    (c - 1)), and nothing of it is read back.  k and std_ratio are the
    customary values, not tuned here.  The sample standard deviation follows
    Open3D's remove_statistical_outlier; Open3D is no dependency of this
    project, so parity with it is not pinned by any test."""
    grid = PointGrid(points, cell=cell)
    mean = grid.knn(grid.ref, k, exclude_self=True, want=("mean",))["mean"]
    stats = dist_stats(mean, math.inf)
    c, s1, s2 = stats[0], stats[1], stats[2]
    mu = s1 / c
    var = torch.clamp_min(s2 - s1 * mu, 0.0) / (c - 1.0)
    thr = mu + float(std_ratio) * torch.sqrt(var)
    keep = torch.isfinite(mean) & (mean.double() <= thr)
    return torch.where(c < 2.0, torch.isfinite(grid.ref).all(1), keep)


STAT_NAMES = ("count", "sum", "sum_sq", "within", "max")


@torch.no_grad()
def dist_stats(dist, threshold: float) -> torch.Tensor:
    """Over the finite entries of dist [m] (float32 device tensor): their
    count, sum, sum of squares, the count of entries <= threshold and the
    maximum (-inf when there is none), as a device float64 tensor [5]
    (STAT_NAMES).  Sums in double in an order m alone fixes: two calls give
    the same bits.  Nothing is read back."""
    fn = "dist_stats"
    if not torch.is_tensor(dist) or dist.dim() != 1:
        raise ValueError(f"{fn}: dist must be a tensor of shape [m]")
    if dist.dtype != torch.float32:
        raise TypeError(f"{fn}: dist must be float32, got {dist.dtype}")
    threshold = float(threshold)
    if math.isnan(threshold):
        raise ValueError(f"{fn}: threshold is NaN")
    _lib.require_cuda(dist)
    dist = dist.contiguous()
    dev, m = dist.device, dist.shape[0]
    out = torch.empty(5, device=dev, dtype=torch.float64)
    ws = torch.empty(max(int(_lib.lib().s3k_dist_stats_workspace_bytes(m)) // 8, 1), device=dev,
                     dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.call("s3k_dist_stats", dist.data_ptr() if m else None, m, threshold, out.data_ptr(),
                  ws.data_ptr(), ws.numel() * 8, _lib.stream(dev))
    return out


@torch.no_grad()
def sample_mesh(verts, faces, n: int, seed: int = 0, counters: bool = False):
    """n area-uniform samples of the mesh verts [V, 3] float32, faces [F, 3]
    int32 (device tensors): (points [n, 3] float32, face [n] int32), one
    stratified sample per stratum of the cumulative area, a function of
    (mesh, n, seed) alone.  A face with an index out of range or a non-finite
    area counts as area 0.  Raises ValueError when the mesh has no area (one
    host read of two counters).  counters=True appends (bad, total): the
    faces left out and the total integer weight."""
    fn = "sample_mesh"
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{fn}: faces must be a tensor of shape [F, 3]")
    if faces.dtype != torch.int32:
        raise TypeError(f"{fn}: faces must be int32, got {faces.dtype}")
    verts = _points(verts, "verts", fn)
    _lib.require_cuda(faces)
    n, seed = int(n), int(seed)
    if n < 0:
        raise ValueError(f"{fn}: n must be >= 0, got {n}")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{fn}: seed must fit 64 bits")
    if faces.device != verts.device:
        raise ValueError(f"{fn}: verts and faces are on different devices")
    faces = faces.contiguous()
    dev, F = verts.device, faces.shape[0]
    points = torch.empty(n, 3, device=dev, dtype=torch.float32)
    face = torch.empty(n, device=dev, dtype=torch.int32)
    tally = torch.zeros(2, device=dev, dtype=torch.int64)
    ws = _bytes(int(_lib.lib().s3k_sample_workspace_bytes(F)), dev)
    with torch.cuda.device(dev):
        _lib.call("s3k_sample_mesh", verts.data_ptr() if verts.shape[0] else None, verts.shape[0],
                  faces.data_ptr() if F else None, F, n, seed, points.data_ptr(), face.data_ptr(),
                  tally.data_ptr(), tally.data_ptr() + 8, ws.data_ptr(), ws.numel(),
                  _lib.stream(dev))
    bad, total = tally.tolist()
    if total == 0:
        raise ValueError(f"{fn}: the mesh has no area ({F} faces, {bad} of them invalid)")
    return (points, face, bad, total) if counters else (points, face)
