"""Photometric refinement of Gaussian splats (include/s3o.h): fit the map's
3DGS parameter rows to the images they came from.

  activate       rows14 -> the five tensors GaussianRasterizer takes (one HIP
                 launch, csrc/splat_opt.hip k_splat_activate)
  SplatAdam      the fused chain rule + Adam step over the rows (one HIP
                 launch, k_splat_adam), sparse over the Gaussians a view did
                 not touch
  refine_splats  the loop: activate, render, photometric loss, backward, step
  render_splats  the images that loop compares against its targets
  DepthControl   a depth term for that loop: the rendered depth against target
                 depth (splatt3r_amd.depth, include/s3z.h)
  pose_gradient  dL/dpose of one view, reduced from the rasterizer's
                 per-Gaussian gradients (include/s3x.h, csrc/pose_grad.hip)
  PoseControl    Adam on the camera twists, fused with the retraction and the
                 camera rewrite (one HIP launch per step, k_pose_step)
  refine_poses   the loop with the map fixed and only the poses moving;
                 localise: the same for one view of cov3D_precomp Gaussians

The reference has no counterpart (its training optimises network weights,
never Gaussians).  The parametrisation is INRIA 3DGS's, which the project's
.ply already uses: a row is x y z, f_dc_0..2, logit opacity, log scale_0..2,
rot w x y z (raw); the optimiser is torch.optim.Adam without weight decay or
amsgrad, one learning rate per parameter group.

Importing this module does not initialise the GPU.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import torch

from splatt3r_amd import _abi, _lib

GROUPS = ("means", "f_dc", "opacity", "scale", "rotation")


S3oAdam = _abi.structs["s3o_adam"]              # include/s3o.h
S3dParams = _abi.structs["s3d_params"]          # include/s3d.h
S3xPoseAdam = _abi.structs["s3x_pose_adam"]     # include/s3x.h

COUNTS = ("pruned", "cloned", "split", "denied")


def _f32(x: float) -> float:
    return ctypes.c_float(float(x)).value


def _check_rows(rows14, fn):
    if not torch.is_tensor(rows14) or rows14.dtype != torch.float32:
        raise TypeError(f"{fn}: rows14 must be a float32 tensor")
    if rows14.dim() != 2 or rows14.shape[1] != 14:
        raise ValueError(f"{fn}: rows14 must be [n, 14], got {tuple(rows14.shape)}")
    _lib.require_cuda(rows14)
    _lib.require_contig(fn, rows14)


@torch.no_grad()
def activate(rows14: torch.Tensor, render_scale: float = 1.0):
    """The rasterizer inputs of [n, 14] parameter rows, with the
    scale-invariant factor `render_scale` (1 / near, as render_map and
    camera_settings apply it): means3D [n, 3] = s xyz, shs [n, 1, 3] = f_dc,
    opacities [n, 1] = sigmoid(logit), scales [n, 3] = s exp(log scale),
    rotations [n, 4] = q / |q| (r, x, y, z; a zero quaternion is the
    identity).  The tensors carry no autograd history: give them
    requires_grad_() and hand their gradients to SplatAdam.step."""
    _check_rows(rows14, "activate")
    n = rows14.shape[0]
    dev = rows14.device
    e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    out = e(n, 3), e(n, 1, 3), e(n, 1), e(n, 3), e(n, 4)
    with torch.cuda.device(dev):
        _lib.call("s3o_activate", rows14.data_ptr() if n else None, n, float(render_scale),
                  *[t.data_ptr() if n else None for t in out], _lib.stream(dev))
    return out


class SplatAdam:
    """Adam over [n, 14] splat parameter rows, the chain rule through the
    activations fused into the step (include/s3o.h s3o_adam_step).

    The learning rates are 3DGS's defaults (means 1.6e-4, f_dc 2.5e-3, opacity
    0.05, scale 5e-3, rotation 1e-3).  Nobody has tuned them for this map:
    3DGS scales its position rate by the scene extent and decays it, neither
    of which is done here.

    `rows14` is updated in place.  betas and eps are rounded to float32, the
    ABI's type; the bias corrections 1 - beta1^t and sqrt(1 - beta2^t) are
    computed on the host in double from the rounded values.
    """

    def __init__(self, rows14: torch.Tensor, lr_means: float = 1.6e-4, lr_f_dc: float = 2.5e-3,
                 lr_opacity: float = 0.05, lr_scale: float = 5e-3, lr_rotation: float = 1e-3,
                 betas=(0.9, 0.999), eps: float = 1e-15):
        _check_rows(rows14, "SplatAdam")
        self.lr = tuple(_f32(v) for v in (lr_means, lr_f_dc, lr_opacity, lr_scale, lr_rotation))
        self.betas = (_f32(betas[0]), _f32(betas[1]))
        self.eps = _f32(eps)
        if any(not (v >= 0.0 and math.isfinite(v)) for v in self.lr):
            raise ValueError(f"SplatAdam: learning rates must be >= 0 and finite, got {self.lr}")
        if not all(0.0 <= b < 1.0 for b in self.betas):
            raise ValueError(f"SplatAdam: betas must be in [0, 1), got {self.betas}")
        if not (self.eps > 0.0 and math.isfinite(self.eps)):
            raise ValueError(f"SplatAdam: eps must be > 0 (as float32), got {eps}")
        self.rows14 = rows14
        self.exp_avg = torch.zeros_like(rows14)
        self.exp_avg_sq = torch.zeros_like(rows14)
        self._skipped = torch.zeros(1, dtype=torch.int32, device=rows14.device)
        self.t = 0

    @property
    def skipped(self) -> int:
        """Rows skipped so far because their gradient held a NaN or an Inf
        (a host read of the device counter: synchronises the stream)."""
        return int(self._skipped.item())

    @torch.no_grad()
    def step(self, grads: Sequence[torch.Tensor], radii: Optional[torch.Tensor] = None,
             render_scale: float = 1.0) -> None:
        """One step.  grads: the gradients of activate()'s five tensors, in
        its order (means3D, shs, opacities, scales, rotations).  radii: the
        rasterizer's int32 [n] output of the same forward; rows with
        radii <= 0 and their moments are left untouched (3DGS's sparse Adam).
        None: every row is stepped."""
        n = self.rows14.shape[0]
        dev = self.rows14.device
        if len(grads) != 5:
            raise ValueError("SplatAdam.step: grads must be the five gradients of activate()")
        want = ((n, 3), (n, 1, 3), (n, 1), (n, 3), (n, 4))
        gs = []
        for g, shape, name in zip(grads, want, ("means3D", "shs", "opacities", "scales",
                                                "rotations")):
            if g is None:
                raise ValueError(f"SplatAdam.step: no gradient for {name}")
            if g.dtype != torch.float32 or g.numel() != math.prod(shape):
                raise ValueError(f"SplatAdam.step: d_{name} must be float32 {shape}, got "
                                 f"{g.dtype} {tuple(g.shape)}")
            _lib.require_cuda(g)
            g = g.contiguous()
            # a view into a wider tensor may start off the 16 bytes d_rotations needs
            gs.append(g.clone() if g.data_ptr() % 16 else g)
        if radii is not None:
            if radii.dtype != torch.int32 or tuple(radii.shape) != (n,):
                raise ValueError(f"SplatAdam.step: radii must be int32 [{n}]")
            _lib.require_cuda(radii)
            radii = radii.contiguous()
        self.t += 1
        hp = S3oAdam((ctypes.c_float * 5)(*self.lr), self.betas[0], self.betas[1], self.eps,
                     1.0 - self.betas[0] ** self.t, math.sqrt(1.0 - self.betas[1] ** self.t),
                     float(render_scale))
        p = lambda t: t.data_ptr() if n else None
        with torch.cuda.device(dev):
            _lib.call("s3o_adam_step", p(self.rows14), p(self.exp_avg), p(self.exp_avg_sq), n,
                      *[p(g) for g in gs], None if radii is None else p(radii),
                      ctypes.byref(hp), self._skipped.data_ptr(), _lib.stream(dev))

    @torch.no_grad()
    def densify(self, stats, params, cap: int):
        """One density pass (densify_splats) over the rows and both moment
        arrays; the optimiser's three tensors are swapped for the results (new
        rows start with zero moments, the step count is shared).  Returns
        (origin, counts)."""
        rows, m, v, origin, counts = densify_splats(self.rows14, self.exp_avg, self.exp_avg_sq,
                                                    stats, params, cap)
        self.rows14, self.exp_avg, self.exp_avg_sq = rows, m, v
        return origin, counts

    @torch.no_grad()
    def reset_opacity(self, opacity: float = 0.01) -> None:
        """3DGS's opacity reset: every logit becomes min(logit, logit(opacity))
        and the opacity column of both moment arrays zero, in place."""
        reset_opacity(self.rows14, self.exp_avg, self.exp_avg_sq, opacity)


# ------------------------------------------------ density control (s3d.h) --
def new_stats(n: int, device):
    """Zeroed (grad_accum float32 [n], denom int32 [n], max_radii int32 [n])."""
    return (torch.zeros(n, device=device, dtype=torch.float32),
            torch.zeros(n, device=device, dtype=torch.int32),
            torch.zeros(n, device=device, dtype=torch.int32))


def _check_stats(stats, n, fn):
    if len(stats) != 3:
        raise ValueError(f"{fn}: stats must be (grad_accum, denom, max_radii)")
    for t, dt, name in zip(stats, (torch.float32, torch.int32, torch.int32),
                           ("grad_accum", "denom", "max_radii")):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (n,):
            raise ValueError(f"{fn}: {name} must be a {dt} tensor of shape [{n}]")
        _lib.require_cuda(t)
        _lib.require_contig(fn, t)


def as_params(params) -> S3dParams:
    """An S3dParams from itself or from a mapping with the keys grad_threshold,
    split_scale, min_opacity, max_scale, max_screen_radius, seed and pass (the
    last four default to 0)."""
    if isinstance(params, S3dParams):
        return params
    p = dict(params)
    unknown = set(p) - {"grad_threshold", "split_scale", "min_opacity", "max_scale",
                        "max_screen_radius", "seed", "pass"}
    if unknown:
        raise ValueError(f"density params: unknown keys {sorted(unknown)}")
    vals = [float(p[k]) for k in ("grad_threshold", "split_scale", "min_opacity")]
    vals.append(float(p.get("max_scale", 0.0)))
    if any(math.isnan(v) for v in vals):
        raise ValueError("density params: a threshold is NaN")
    seed, pass_ = int(p.get("seed", 0)), int(p.get("pass", 0))
    if not (0 <= seed < 2 ** 64 and 0 <= pass_ < 2 ** 32):
        raise ValueError("density params: seed must fit 64 bits and pass 32, unsigned")
    return S3dParams(*vals, int(p.get("max_screen_radius", 0)), seed, pass_)


@torch.no_grad()
def accumulate_stats(d_means2D: torch.Tensor, radii: torch.Tensor, stats) -> None:
    """Add one step to the density statistics (include/s3d.h s3d_accumulate):
    d_means2D [n, 3] is the gradient the rasterizer's backward leaves on its
    means2D argument, radii [n] the same forward's int32 radii."""
    n = radii.shape[0]
    if d_means2D.dtype != torch.float32 or tuple(d_means2D.shape) != (n, 3):
        raise ValueError(f"accumulate_stats: d_means2D must be float32 [{n}, 3]")
    if radii.dtype != torch.int32 or radii.dim() != 1:
        raise ValueError("accumulate_stats: radii must be int32 [n]")
    _check_stats(stats, n, "accumulate_stats")
    _lib.require_cuda(d_means2D, radii)
    d_means2D, radii = d_means2D.contiguous(), radii.contiguous()
    if n == 0:
        return
    with torch.cuda.device(radii.device):
        _lib.call("s3d_accumulate", d_means2D.data_ptr(), radii.data_ptr(), n,
                  *[t.data_ptr() for t in stats], _lib.stream(radii.device))


@torch.no_grad()
def densify_splats(rows14, exp_avg, exp_avg_sq, stats, params, cap: int):
    """One density pass (include/s3d.h s3d_densify): prune, clone and split
    the rows and their two Adam moment arrays, out of place.  stats:
    (grad_accum, denom, max_radii); params: an S3dParams or a mapping
    (as_params); cap: the most rows the result may have, >= n.

    Returns (rows14, exp_avg, exp_avg_sq, origin, counts): the three [n_out,
    14] arrays, origin int32 [n_out] (i for a kept row or a clone's original,
    ~i for a clone's copy or a split child) and counts, a dict of pruned,
    cloned, split and denied.  One host read: n_out and the counts, in one
    copy."""
    _check_rows(rows14, "densify_splats")
    n = rows14.shape[0]
    dev = rows14.device
    for t, name in ((exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (n, 14):
            raise ValueError(f"densify_splats: {name} must be float32 [{n}, 14]")
        _lib.require_cuda(t)
        _lib.require_contig("densify_splats", t)
    _check_stats(stats, n, "densify_splats")
    hp = as_params(params)
    cap = int(cap)
    if cap < n:
        raise ValueError(f"densify_splats: cap {cap} < n {n}")
    # no row has more than two outputs, so a capacity past 2 n never binds
    cap = min(cap, 2 * n)
    e = lambda: torch.empty(cap, 14, device=dev, dtype=torch.float32)
    out = e(), e(), e()
    origin = torch.empty(cap, device=dev, dtype=torch.int32)
    if n == 0:
        return (*out, origin, dict.fromkeys(COUNTS, 0))
    # n_out (int64) and the four int32 counts share one buffer: one host read
    tally = torch.zeros(3, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        need = int(_lib.lib().s3d_workspace_bytes(n))
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        _lib.call("s3d_densify", rows14.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n,
                  *[t.data_ptr() for t in stats], ctypes.byref(hp), cap,
                  *[t.data_ptr() for t in out], origin.data_ptr(), tally.data_ptr(),
                  tally.data_ptr() + 8, ws.data_ptr(), need, _lib.stream(dev))
    host = tally.cpu()
    n_out = int(host[0])
    counts = dict(zip(COUNTS, host[1:].view(torch.int32).tolist()))
    return (*[t[:n_out] for t in out], origin[:n_out], counts)


@torch.no_grad()
def reset_opacity(rows14, exp_avg, exp_avg_sq, opacity: float = 0.01) -> None:
    """include/s3d.h s3d_reset_opacity, in place; the cap logit(opacity) is
    computed in double and rounded to float32 once."""
    _check_rows(rows14, "reset_opacity")
    n = rows14.shape[0]
    for t in (exp_avg, exp_avg_sq):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (n, 14):
            raise ValueError(f"reset_opacity: the moment arrays must be float32 [{n}, 14]")
        _lib.require_cuda(t)
        _lib.require_contig("reset_opacity", t)
    if not 0.0 < float(opacity) < 1.0:
        raise ValueError(f"reset_opacity: opacity must be in (0, 1), got {opacity}")
    cap = math.log(float(opacity) / (1.0 - float(opacity)))
    if n == 0:
        return
    with torch.cuda.device(rows14.device):
        _lib.call("s3d_reset_opacity", rows14.data_ptr(), exp_avg.data_ptr(),
                  exp_avg_sq.data_ptr(), n, cap, _lib.stream(rows14.device))


def compose_origin(prev: torch.Tensor, origin: torch.Tensor) -> torch.Tensor:
    """`origin` of one pass, whose inputs had the composed origin `prev`,
    composed down to the rows prev refers to: i for a row that is input row i
    itself, ~i for a row created since, out of input row i."""
    src = torch.where(origin >= 0, origin, ~origin).long()
    base = prev[src]
    return torch.where((origin < 0) & (base >= 0), ~base, base)


class DensityControl:
    """Adaptive density control of refine_splats: INRIA 3DGS's
    densify_and_prune and reset_opacity as include/s3d.h restates them.

    After step t (counted from 1) a pass runs when start <= t <= stop and
    t % interval == 0; the opacities are reset after a step with
    t % opacity_reset_interval == 0 (0: never).  Between passes every step's
    dL/dmeans2D and radii go into the statistics (s3d_accumulate); a pass
    zeroes them at the new size.

    grad_threshold, percent_dense, min_opacity and the schedule are 3DGS's
    defaults.  Nobody has tuned them for this map: 3DGS runs 30,000 steps over
    a whole scene, this map is refined for far fewer against a few keyframes.
    A growing row splits when its largest scale exceeds percent_dense x extent
    and is pruned when it exceeds max_world_scale x extent (0: never) or when
    its largest screen radius exceeded max_screen_radius pixels (0: never).
    extent None: 1.1 x the largest distance of a camera centre from the
    centres' mean, as 3DGS's cameras_extent; ValueError if that is 0 (one
    view, or coincident cameras).  capacity None: no row limit but the two
    outputs per row (SharedGaussians.refine sets max_gaussians).

    After a run: .log holds one dict per pass (t, n before, the four counts,
    n_out); .origin maps every final row to the run's first input (i: that
    row itself; ~i: created during the run, out of row i).
    on_pass(pass_index, inputs, outputs), for tests: inputs = (rows14,
    exp_avg, exp_avg_sq, grad_accum, denom, max_radii, params, cap), outputs
    = (rows14, exp_avg, exp_avg_sq, origin, counts)."""

    def __init__(self, start: int = 500, interval: int = 100, stop: int = 15000,
                 grad_threshold: float = 2e-4, percent_dense: float = 0.01, extent=None,
                 min_opacity: float = 0.005, max_world_scale: float = 0.1,
                 max_screen_radius: int = 0, opacity_reset_interval: int = 0, capacity=None,
                 seed: int = 0, on_pass=None):
        self.start, self.interval, self.stop = int(start), int(interval), int(stop)
        if self.start < 0 or self.interval < 1 or self.stop < self.start:
            raise ValueError("DensityControl: need start >= 0, interval >= 1, stop >= start")
        vals = dict(grad_threshold=grad_threshold, percent_dense=percent_dense,
                    min_opacity=min_opacity, max_world_scale=max_world_scale)
        for k, v in vals.items():
            if not (float(v) >= 0.0 and math.isfinite(float(v))):
                raise ValueError(f"DensityControl: {k} must be >= 0 and finite, got {v}")
        self.grad_threshold, self.percent_dense = float(grad_threshold), float(percent_dense)
        self.min_opacity, self.max_world_scale = float(min_opacity), float(max_world_scale)
        if extent is not None and not (float(extent) > 0.0 and math.isfinite(float(extent))):
            raise ValueError(f"DensityControl: extent must be > 0 and finite, got {extent}")
        self.extent = None if extent is None else float(extent)
        self.max_screen_radius = int(max_screen_radius)
        self.opacity_reset_interval = int(opacity_reset_interval)
        if self.max_screen_radius < 0 or self.opacity_reset_interval < 0:
            raise ValueError("DensityControl: max_screen_radius and opacity_reset_interval "
                             "must be >= 0")
        if capacity is not None and int(capacity) < 0:
            raise ValueError("DensityControl: capacity must be >= 0")
        self.capacity = None if capacity is None else int(capacity)
        self.seed = int(seed)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("DensityControl: seed must fit 64 bits, unsigned")
        self.on_pass = on_pass
        self.log: list = []
        self.origin: Optional[torch.Tensor] = None

    @staticmethod
    def cameras_extent(T_WC) -> float:
        """1.1 x the largest distance of a camera centre from the centres' mean."""
        c = T_WC.detach().to("cpu", torch.float64)[:, :3, 3]
        return 1.1 * float((c - c.mean(0, keepdim=True)).norm(dim=1).max())

    def due(self, t: int) -> bool:
        return self.start <= t <= self.stop and t % self.interval == 0

    def reset_due(self, t: int) -> bool:
        return self.opacity_reset_interval > 0 and t % self.opacity_reset_interval == 0

    def begin(self, n: int, T_WC, device) -> None:
        """Start a run over n rows seen from the poses T_WC."""
        extent = self.extent if self.extent is not None else self.cameras_extent(T_WC)
        if not extent > 0.0:
            raise ValueError("DensityControl: the camera centres coincide, so the scene extent "
                             "is 0; pass extent=")
        if self.capacity is not None and self.capacity < n:
            raise ValueError(f"DensityControl: capacity {self.capacity} < {n} rows")
        self._extent = extent
        self.log = []
        self.origin = torch.arange(n, device=device, dtype=torch.int32)

    def params(self, pass_index: int) -> S3dParams:
        return S3dParams(self.grad_threshold, self.percent_dense * self._extent, self.min_opacity,
                         self.max_world_scale * self._extent, self.max_screen_radius, self.seed,
                         int(pass_index))

    def run_pass(self, opt: "SplatAdam", stats, t: int):
        """One pass on the optimiser's tensors; returns the zeroed statistics
        of the new size."""
        k = len(self.log)
        n = opt.rows14.shape[0]
        hp = self.params(k)
        cap = 2 * n if self.capacity is None else self.capacity
        inputs = (opt.rows14, opt.exp_avg, opt.exp_avg_sq, *stats, hp, cap)
        origin, counts = opt.densify(stats, hp, cap)
        self.origin = compose_origin(self.origin, origin)
        self.log.append(dict(t=t, n=n, **counts, n_out=opt.rows14.shape[0]))
        if self.on_pass is not None:
            self.on_pass(k, inputs, (opt.rows14, opt.exp_avg, opt.exp_avg_sq, origin, counts))
        return new_stats(opt.rows14.shape[0], opt.rows14.device)


class DepthControl:
    """Depth supervision of refine_splats (splatt3r_amd.depth, include/s3z.h):
    each step's view is rendered with return_depth=True and
    weight x depth_loss(rendered depth / alpha against targets[v]) is added to
    the photometric loss before the single backward.

    targets [V, H, W]: the target depth of every view, in the units of T_WC's
    cameras (view-space z); a pixel with no target is 0 (or NaN).  weights
    [V, H, W] or None: per-pixel weights, a mask being 0 / 1.  scale: a number
    the rendered depth is multiplied by before it is compared (None: 1).
    l1_weight, l2_weight, grad_weight and alpha_min are depth_loss's.

    weight = 0.1 is MonoGS's RGB-D split (0.9 photometric, 0.1 depth); nobody
    has tuned it for this map.

    After a run: .history holds the per-step depth losses (before `weight`),
    a device tensor [iters]."""

    def __init__(self, targets, weights=None, weight: float = 0.1, l1_weight: float = 1.0,
                 l2_weight: float = 0.0, grad_weight: float = 0.0, alpha_min: float = 0.5,
                 scale=None):
        for name, t in (("targets", targets), ("weights", weights)):
            if t is None and name == "weights":
                continue
            if not torch.is_tensor(t) or t.dim() != 3 or not t.is_floating_point():
                raise ValueError(f"DepthControl: {name} must be a floating-point [V, H, W] tensor")
        if weights is not None and weights.shape != targets.shape:
            raise ValueError(f"DepthControl: weights {tuple(weights.shape)} and targets "
                             f"{tuple(targets.shape)} differ in shape")
        vals = dict(weight=weight, l1_weight=l1_weight, l2_weight=l2_weight,
                    grad_weight=grad_weight, alpha_min=alpha_min)
        for k, v in vals.items():
            if not (float(v) >= 0.0 and math.isfinite(float(v))):
                raise ValueError(f"DepthControl: {k} must be >= 0 and finite, got {v}")
        if scale is not None and not (float(scale) > 0.0 and math.isfinite(float(scale))):
            raise ValueError(f"DepthControl: scale must be > 0 and finite, got {scale}")
        self.targets, self.weights = targets, weights
        self.weight, self.l1_weight, self.l2_weight = float(weight), float(l1_weight), float(l2_weight)
        self.grad_weight, self.alpha_min = float(grad_weight), float(alpha_min)
        self.scale = 1.0 if scale is None else float(scale)
        self.history: Optional[torch.Tensor] = None

    def check(self, V: int, H: int, W: int) -> None:
        if tuple(self.targets.shape) != (V, H, W):
            raise ValueError(f"DepthControl: targets must be [{V}, {H}, {W}], got "
                             f"{tuple(self.targets.shape)}")

    def begin(self, iters: int, render_scale: float, device) -> None:
        """Start a run: targets and weights move to the device, and the
        scale-invariant factor of the cameras (the rasterizer's depth is
        render_scale x the caller's units) is folded into the kernel's scale."""
        f = lambda t: None if t is None else t.detach().to(device, torch.float32).contiguous()
        self._targets, self._weights = f(self.targets), f(self.weights)
        self._scale = torch.full((1,), self.scale / float(render_scale), dtype=torch.float32,
                                 device=device)
        self.history = torch.zeros(int(iters), device=device, dtype=torch.float32)

    def loss(self, it: int, v: int, depth, alpha):
        """The depth loss of view v's render (before `weight`); recorded."""
        from splatt3r_amd.depth import depth_loss
        out = depth_loss(depth[None], alpha[None], self._targets[v:v + 1],
                         None if self._weights is None else self._weights[v:v + 1],
                         scale=self._scale, l1_weight=self.l1_weight, l2_weight=self.l2_weight,
                         grad_weight=self.grad_weight, alpha_min=self.alpha_min)
        self.history[it] = out.detach()
        return out


def _cameras(T_WC, K, H, W, near, far, bg, dev):
    """render.camera_settings (scale-invariant) of V camera-to-world poses:
    the intrinsics-only quantities on the host (no device read for the
    tan(fov) floats), the pose part on the device.  Returns (settings, s)."""
    from splatt3r_amd.render import camera_settings, normalize_intrinsics
    V = T_WC.shape[0]
    Kc = K.detach().to("cpu", torch.float32).reshape(3, 3)
    intr = normalize_intrinsics(Kc[None].repeat(V, 1, 1), (H, W))
    bgt = torch.tensor([0.0, 0.0, 0.0] if bg is None else list(bg), dtype=torch.float32,
                       device=dev)[None].repeat(V, 1)
    settings, scale = camera_settings(
        T_WC.detach().to(dev, torch.float32), intr, torch.full((V,), float(near)),
        torch.full((V,), float(far)), (H, W), bgt, 0)
    return settings, float(scale[0])


@torch.no_grad()
def render_splats(rows14, T_WC, K, H, W, near=0.1, far=1000.0, bg=None):
    """The images [V, 3, H, W] refine_splats compares against its targets:
    rows14 rendered from the V camera-to-world poses T_WC [V, 4, 4]."""
    from diff_gaussian_rasterization import GaussianRasterizer
    _check_rows(rows14, "render_splats")
    dev = rows14.device
    with torch.cuda.device(dev):
        settings, s = _cameras(T_WC, K, H, W, near, far, bg, dev)
        means3D, shs, opac, scales, rots = activate(rows14, s)
        return torch.stack([GaussianRasterizer(st)(
            means3D=means3D, means2D=torch.zeros_like(means3D), opacities=opac, shs=shs,
            scales=scales, rotations=rots)[0] for st in settings])


def refine_splats(rows14, images, T_WC, K, iters, masks=None, l1_weight=0.8, ssim_weight=0.2,
                  mse_weight=0.0, near=0.1, far=1000.0, bg=None, sparse=True, order=None,
                  density=None, poses=None, depth=None, **lr):
    """Fit splat rows to images.  rows14 [n, 14] float32 on the GPU (a copy is
    refined; the argument is left as it is), images [V, 3, H, W] in [0, 1],
    T_WC [V, 4, 4] camera-to-world, K [3, 3] pixel intrinsics, masks
    [V, H, W] or None, bg a colour triple (default black).  One view per
    step, round-robin, or the sequence `order` gives; every step is
    activate -> render.camera_settings (scale-invariant, factor 1 / near) ->
    GaussianRasterizer(scales, rotations, shs, sh_degree 0) ->
    photometric_loss -> one backward -> one fused SplatAdam step, on that
    forward's radii when `sparse`.  **lr: SplatAdam's keyword arguments.

    density: a DensityControl, or None for a fixed set of Gaussians.  With
    one, means2D carries a gradient, every step's dL/dmeans2D and radii go to
    s3d_accumulate, and a pass (prune, clone, split) runs when due: the number
    of rows then changes, density.origin maps the returned rows to the rows
    given, and each pass reads its row count back (one host read).

    poses: a PoseControl, or None for poses taken as exact (the same launches
    and the same bits as before the argument existed).  With one, the cameras
    live on the device in float64, every step also reduces that backward's
    gradients to dL/dpose (pose_gradient, rotation form) and steps the view
    just rendered (s3x_pose_step) unless it is in poses.fixed; the refined
    poses are poses.T_WC.  Rows and poses together have a 6-dof gauge: fix a
    view, PoseControl(fixed=(0,)).

    depth: a DepthControl, or None for the photometric loss alone (the same
    launches and the same bits as before the argument existed).  With one,
    the step renders with return_depth=True and adds depth.weight x
    depth.depth_loss of the rendered depth and alpha against depth.targets[v]
    to the loss before the one backward; the cameras' scale-invariant factor
    goes into the kernel's scale argument, no tensor is rescaled.  history is
    the total loss, depth.history the depth term.  Not together with poses
    (NotImplementedError): the pose gradient is not taken through the depth.

    Returns (rows14, history): the refined rows and the per-step losses
    [iters] as a device tensor (the loss before each step).  Without density
    the loop itself reads nothing back from the device (the rasterizer's
    forward reads its instance count, as in every differentiable render)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from splatt3r_amd.photometric import photometric_loss
    if depth is not None:
        if not isinstance(depth, DepthControl):
            raise TypeError("refine_splats: depth must be a DepthControl or None")
        if poses is not None:
            raise NotImplementedError("refine_splats: depth= together with poses= is not "
                                      "implemented")
        if torch.is_tensor(images) and images.dim() == 4:
            depth.check(images.shape[0], *images.shape[-2:])
    _check_rows(rows14, "refine_splats")
    dev = rows14.device
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"refine_splats: images must be [V, 3, H, W], got {tuple(images.shape)}")
    V, _, H, W = images.shape
    if tuple(T_WC.shape) != (V, 4, 4):
        raise ValueError(f"refine_splats: T_WC must be [{V}, 4, 4], got {tuple(T_WC.shape)}")
    if masks is not None and tuple(masks.shape) != (V, H, W):
        raise ValueError(f"refine_splats: masks must be [{V}, {H}, {W}]")
    order = list(range(V)) if order is None else [int(v) for v in order]
    if int(iters) > 0 and (not order or min(order) < 0 or max(order) >= V):
        raise ValueError(f"refine_splats: order must index the {V} views")
    images = images.to(dev, torch.float32).contiguous()
    masks = None if masks is None else masks.to(dev, torch.float32).contiguous()
    rows = rows14.detach().clone()
    opt = SplatAdam(rows, **lr)
    history = torch.zeros(int(iters), device=dev, dtype=torch.float32)
    if density is not None:
        if not isinstance(density, DensityControl):
            raise TypeError("refine_splats: density must be a DensityControl or None")
        density.begin(rows.shape[0], T_WC, dev)
    if poses is not None and not isinstance(poses, PoseControl):
        raise TypeError("refine_splats: poses must be a PoseControl or None")
    if int(iters) == 0 or rows.shape[0] == 0:
        if poses is not None:
            with torch.cuda.device(dev):
                _pose_cameras(poses, T_WC, K, H, W, near, far, bg, dev)
        return rows, history
    with torch.cuda.device(dev):
        if poses is None:
            settings, s = _cameras(T_WC, K, H, W, near, far, bg, dev)
        else:
            settings, s = _pose_cameras(poses, T_WC, K, H, W, near, far, bg, dev)
        stats = None if density is None else new_stats(rows.shape[0], dev)
        if depth is not None:
            depth.begin(iters, s, dev)
        for it in range(int(iters)):
            v = order[it % len(order)]
            acts = [t.requires_grad_(True) for t in activate(opt.rows14, s)]
            means3D, shs, opac, scales, rots = acts
            means2D = torch.zeros_like(means3D)
            if density is not None:
                means2D.requires_grad_(True)
            if depth is None:
                img, radii = GaussianRasterizer(settings[v])(
                    means3D=means3D, means2D=means2D, opacities=opac, shs=shs,
                    scales=scales, rotations=rots)
            else:
                img, radii, zmap, amap = GaussianRasterizer(settings[v])(
                    means3D=means3D, means2D=means2D, opacities=opac, shs=shs,
                    scales=scales, rotations=rots, return_depth=True)
            loss = photometric_loss(img[None], images[v:v + 1],
                                    None if masks is None else masks[v:v + 1],
                                    mse_weight=mse_weight, l1_weight=l1_weight,
                                    ssim_weight=ssim_weight)
            if depth is not None:
                loss = loss + depth.weight * depth.loss(it, v, zmap, amap)
            loss.backward()
            history[it] = loss.detach()
            if poses is not None and v not in poses.fixed:
                # on the view matrix this forward and backward used
                g = pose_gradient(settings[v].viewmatrix, means3D.detach(), means3D.grad,
                                  rotations=rots.detach(), d_rotations=rots.grad, radii=radii,
                                  skipped=poses._skipped)
            opt.step([a.grad for a in acts], radii if sparse else None, s)
            if poses is not None and v not in poses.fixed:
                poses.step(v, g)
            if density is None:
                continue
            accumulate_stats(means2D.grad, radii, stats)
            if density.due(it + 1):
                stats = density.run_pass(opt, stats, it + 1)
                if opt.rows14.shape[0] == 0:      # every row pruned: nothing left to fit
                    break
            if density.reset_due(it + 1):
                opt.reset_opacity()
    return opt.rows14, history


# --------------------------------------------- pose refinement (s3x.h) ----
def _check_f32(fn, n, width, tensors, names):
    for t, name in zip(tensors, names):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != n * width:
            raise ValueError(f"{fn}: {name} must be a float32 tensor of {n} x {width} entries")


def _rows_of(t, n, width):
    t = t.detach().reshape(n, width).contiguous()
    # a view into a wider tensor may start off the 16 bytes a float4 row needs
    return t.clone() if t.data_ptr() % 16 else t


@torch.no_grad()
def pose_gradient(viewmatrix, means3D, d_means3D, *, cov3D=None, d_cov3D=None, rotations=None,
                  d_rotations=None, radii=None, skipped=None):
    """dL/dxi of one view, a float64 [6] device tensor (include/s3x.h
    s3x_pose_grad): xi = (rho, phi) is the twist of T_WC <- T_WC Exp(xi), in
    the camera's own frame and in view-space units, reduced from the
    gradients GaussianRasterizer's backward leaves on means3D and on either
    cov3D_precomp (cov3D, d_cov3D [n, 6]) or rotations (rotations,
    d_rotations [n, 4], unit quaternions as activate() writes them, with
    scale_modifier-independent scales).  viewmatrix: the [4, 4] device view
    matrix of that forward.  radii: the forward's int32 [n] (rows with
    radii <= 0 are not loaded) or None for every row.  skipped: a device
    int32 [1] counter, added to for every row left out because an input was
    not finite.

    Valid for SH degree 0 or colors_precomp only: with SH degree > 0 the
    colour depends on the view direction and this is not the whole gradient.
    Bit-reproducible: the same inputs give the same six doubles."""
    fn = "pose_gradient"
    if (cov3D is None) != (d_cov3D is None) or (rotations is None) != (d_rotations is None):
        raise ValueError(f"{fn}: cov3D goes with d_cov3D, rotations with d_rotations")
    if (cov3D is None) == (rotations is None):
        raise ValueError(f"{fn}: give either cov3D and d_cov3D or rotations and d_rotations")
    if not torch.is_tensor(means3D) or means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError(f"{fn}: means3D must be [n, 3]")
    n = means3D.shape[0]
    _check_f32(fn, n, 3, (means3D, d_means3D), ("means3D", "d_means3D"))
    if cov3D is not None:
        width, shape = 6, (cov3D, d_cov3D)
        _check_f32(fn, n, 6, shape, ("cov3D", "d_cov3D"))
    else:
        width, shape = 4, (rotations, d_rotations)
        _check_f32(fn, n, 4, shape, ("rotations", "d_rotations"))
    if not torch.is_tensor(viewmatrix) or viewmatrix.numel() != 16:
        raise ValueError(f"{fn}: viewmatrix must hold 4 x 4 entries")
    if radii is not None and (not torch.is_tensor(radii) or radii.dtype != torch.int32
                              or tuple(radii.shape) != (n,)):
        raise ValueError(f"{fn}: radii must be int32 [{n}]")
    if skipped is not None and (not torch.is_tensor(skipped) or skipped.dtype != torch.int32
                                or skipped.numel() != 1):
        raise ValueError(f"{fn}: skipped must be an int32 tensor of one entry")
    _lib.require_cuda(viewmatrix, means3D, d_means3D, *shape, radii, skipped)
    mu, dmu = _rows_of(means3D, n, 3), _rows_of(d_means3D, n, 3)
    sh, dsh = _rows_of(shape[0], n, width), _rows_of(shape[1], n, width)
    radii = None if radii is None else radii.contiguous()
    dev = mu.device
    vm = viewmatrix.detach().to(torch.float32).contiguous()
    out = torch.empty(6, device=dev, dtype=torch.float64)
    p = lambda t: t.data_ptr() if n else None
    # which pair is non-null names the form, also for n == 0 (nothing is read then)
    pair = (sh.data_ptr() or 16, dsh.data_ptr() or 16)
    with torch.cuda.device(dev):
        need = int(_lib.lib().s3x_pose_grad_workspace_bytes(n))
        ws = torch.empty(need // 8, device=dev, dtype=torch.float64)
        _lib.call("s3x_pose_grad", vm.data_ptr(), p(mu), p(dmu),
                  *(pair if cov3D is not None else (None, None)),
                  *(pair if cov3D is None else (None, None)),
                  None if radii is None else p(radii), n, out.data_ptr(),
                  None if skipped is None else skipped.data_ptr(), ws.data_ptr(), need,
                  _lib.stream(dev))
    return out


class PoseControl:
    """Camera poses as optimisation variables of refine_splats, refine_poses
    and SharedGaussians.refine_pose: Adam on the six components of the twist
    xi = (rho, phi) of T_WC <- T_WC Exp(xi) (the camera's own frame), one
    moment pair per view, fused with the retraction and the rewrite of that
    view's float32 camera (include/s3x.h s3x_pose_step).

    The learning rates are MonoGS's (rotation 3e-3, translation 1e-3).  Nobody
    has tuned them for this map.  `fixed` names the views that are never
    stepped.  Gaussians and poses refined together have a 6-dof gauge (a rigid
    motion of everything changes no image): pass fixed=(0,) there.

    After a run: .T_WC is the float64 [V, 4, 4] device tensor of the refined
    camera-to-world poses (a fixed view's is its input, bit for bit; a uniform
    scale of the 3 x 3 block is kept), .skipped the number of Gaussian rows
    the gradient left out because an input was not finite (a host read of the
    device counter).  A step whose gradient holds a NaN or an Inf leaves that
    pose and its moments as they were.  Writing the poses back into keyframes
    or the factor graph is the caller's business."""

    def __init__(self, lr_rotation: float = 3e-3, lr_translation: float = 1e-3,
                 betas=(0.9, 0.999), eps: float = 1e-15, fixed=()):
        self.lr_rotation, self.lr_translation = float(lr_rotation), float(lr_translation)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        for k, v in (("lr_rotation", self.lr_rotation), ("lr_translation", self.lr_translation)):
            if not (v >= 0.0 and math.isfinite(v)):
                raise ValueError(f"PoseControl: {k} must be >= 0 and finite, got {v}")
        if not all(0.0 <= b < 1.0 for b in self.betas):
            raise ValueError(f"PoseControl: betas must be in [0, 1), got {self.betas}")
        if not (self.eps > 0.0 and math.isfinite(self.eps)):
            raise ValueError(f"PoseControl: eps must be > 0 and finite, got {eps}")
        self.fixed = tuple(sorted({int(v) for v in fixed}))
        if any(v < 0 for v in self.fixed):
            raise ValueError(f"PoseControl: fixed must name views by index >= 0, got {fixed}")
        self.T_WC: Optional[torch.Tensor] = None
        self._skipped: Optional[torch.Tensor] = None

    @property
    def skipped(self) -> int:
        return 0 if self._skipped is None else int(self._skipped.item())

    def begin(self, T_WC, proj_t, render_scale: float, device) -> None:
        """Start a run from the poses T_WC [V, 4, 4]: the state moves to the
        device and every view's camera is written.  proj_t: the transposed
        projection matrix [4, 4]."""
        if not torch.is_tensor(T_WC) or T_WC.dim() != 3 or tuple(T_WC.shape[1:]) != (4, 4):
            raise ValueError("PoseControl: T_WC must be [V, 4, 4]")
        V = T_WC.shape[0]
        if any(v >= V for v in self.fixed):
            raise ValueError(f"PoseControl: fixed {self.fixed} must index the {V} views")
        if not (float(render_scale) > 0.0 and math.isfinite(float(render_scale))):
            raise ValueError("PoseControl: render_scale must be > 0 and finite")
        dev = torch.device(device)
        _lib.require_cuda(torch.empty(0, device=dev))
        self.T_WC = T_WC.detach().to(dev, torch.float64).contiguous().clone()
        self.exp_avg = torch.zeros(V, 6, device=dev, dtype=torch.float64)
        self.exp_avg_sq = torch.zeros(V, 6, device=dev, dtype=torch.float64)
        self.cameras = torch.empty(V, 35, device=dev, dtype=torch.float32)
        self._proj_t = proj_t.detach().to(dev, torch.float32).contiguous()
        self._scale = float(render_scale)
        self._skipped = torch.zeros(1, device=dev, dtype=torch.int32)
        self.t = [0] * V
        for v in range(V):
            self._launch(v, None)

    def camera(self, v: int):
        """(viewmatrix [4, 4], projmatrix [4, 4], campos [3]) of view v: views
        of the buffers s3x_pose_step rewrites."""
        c = self.cameras[v]
        return c[:16].view(4, 4), c[16:32].view(4, 4), c[32:35]

    def _launch(self, v, grad):
        t = max(self.t[v], 1)
        hp = S3xPoseAdam(self.lr_translation, self.lr_rotation, self.betas[0], self.betas[1],
                         self.eps, 1.0 - self.betas[0] ** t, math.sqrt(1.0 - self.betas[1] ** t),
                         self._scale)
        vm, pm, cp = self.camera(v)
        dev = self.T_WC.device
        with torch.cuda.device(dev):
            _lib.call("s3x_pose_step", self.T_WC[v].data_ptr(), self.exp_avg[v].data_ptr(),
                      self.exp_avg_sq[v].data_ptr(), None if grad is None else grad.data_ptr(),
                      ctypes.byref(hp), self._proj_t.data_ptr(), vm.data_ptr(), pm.data_ptr(),
                      cp.data_ptr(), _lib.stream(dev))

    @torch.no_grad()
    def step(self, v: int, grad: torch.Tensor) -> None:
        """One step of view v on pose_gradient's output; nothing for a fixed
        view."""
        v = int(v)
        if v in self.fixed:
            return
        if not torch.is_tensor(grad) or grad.dtype != torch.float64 or grad.numel() != 6:
            raise ValueError("PoseControl.step: grad must be a float64 tensor of six entries")
        _lib.require_cuda(grad)
        self.t[v] += 1
        self._launch(v, grad.contiguous())


def _projection(K, H, W, near, far):
    """The intrinsics-only part of render.camera_settings (scale-invariant),
    on the host with its torch ops: (tanfovx, tanfovy, transposed projection
    [4, 4], scale)."""
    from splatt3r_amd.render import get_fov, get_projection_matrix, normalize_intrinsics
    Kc = K.detach().to("cpu", torch.float32).reshape(3, 3)
    nr, fr = torch.full((1,), float(near)), torch.full((1,), float(far))
    scale = 1 / nr
    fov_x, fov_y = get_fov(normalize_intrinsics(Kc[None], (H, W))).unbind(dim=-1)
    proj_t = get_projection_matrix(nr * scale, fr * scale, fov_x, fov_y).transpose(1, 2)[0]
    return (float((0.5 * fov_x).tan()[0]), float((0.5 * fov_y).tan()[0]), proj_t.contiguous(),
            float(scale[0]))


def _pose_cameras(poses, T_WC, K, H, W, near, far, bg, dev):
    """_cameras with the pose part on the device in float64: starts the
    PoseControl's run and returns (settings over its camera buffers, s)."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    tx, ty, proj_t, s = _projection(K, H, W, near, far)
    poses.begin(T_WC, proj_t, s, dev)
    bgt = torch.tensor([0.0, 0.0, 0.0] if bg is None else list(bg), dtype=torch.float32,
                       device=dev)
    settings = []
    for v in range(T_WC.shape[0]):
        vm, pm, cp = poses.camera(v)
        settings.append(GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=tx, tanfovy=ty, bg=bgt, scale_modifier=1.0,
            viewmatrix=vm, projmatrix=pm, sh_degree=0, campos=cp, prefiltered=False, debug=False))
    return settings, s


def _pose_loop(poses, settings, images, masks, order, iters, leaves, render, grad_kw, weights):
    """The steps refine_poses and SharedGaussians.refine_pose share: render
    view v from its device camera, photometric loss, backward, pose_gradient,
    pose step.  leaves: the tensors whose .grad the backward fills (cleared
    every step); render(settings) -> (image, radii); grad_kw() -> the keyword
    arguments of pose_gradient after a backward."""
    from splatt3r_amd.photometric import photometric_loss
    history = torch.zeros(int(iters), device=images.device, dtype=torch.float32)
    for it in range(int(iters)):
        v = order[it % len(order)]
        for t in leaves:
            t.grad = None
        frozen = v in poses.fixed
        with torch.set_grad_enabled(not frozen):
            img, radii = render(settings[v])
            loss = photometric_loss(img[None], images[v:v + 1],
                                    None if masks is None else masks[v:v + 1], **weights)
        history[it] = loss.detach()
        if frozen:
            continue
        loss.backward()
        g = pose_gradient(settings[v].viewmatrix, radii=radii, skipped=poses._skipped,
                          **grad_kw())
        poses.step(v, g)
    for t in leaves:
        t.grad = None
    return history


def refine_poses(rows14, images, T_WC, K, iters, masks=None, poses=None, l1_weight=0.8,
                 ssim_weight=0.2, mse_weight=0.0, near=0.1, far=1000.0, bg=None, order=None):
    """Fit camera poses to images of a fixed map.  Arguments as refine_splats;
    rows14 is not changed.  poses: a PoseControl (default PoseControl(): every
    view moves; the map fixes the gauge).  One view per step, round-robin or
    as `order` gives: activate once, then per step render from the view's
    device camera -> photometric_loss -> backward -> pose_gradient (rotation
    form, on that forward's radii) -> s3x_pose_step.  A view in poses.fixed is
    rendered for its loss only.

    Returns (T_WC, history): the refined poses, float64 [V, 4, 4] on the
    device (also poses.T_WC), and the per-step losses [iters] as a device
    tensor.  The loop reads nothing back from the device but the rasterizer's
    instance count."""
    from diff_gaussian_rasterization import GaussianRasterizer
    _check_rows(rows14, "refine_poses")
    dev = rows14.device
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"refine_poses: images must be [V, 3, H, W], got {tuple(images.shape)}")
    V, _, H, W = images.shape
    if tuple(T_WC.shape) != (V, 4, 4):
        raise ValueError(f"refine_poses: T_WC must be [{V}, 4, 4], got {tuple(T_WC.shape)}")
    if masks is not None and tuple(masks.shape) != (V, H, W):
        raise ValueError(f"refine_poses: masks must be [{V}, {H}, {W}]")
    poses = PoseControl() if poses is None else poses
    if not isinstance(poses, PoseControl):
        raise TypeError("refine_poses: poses must be a PoseControl or None")
    order = list(range(V)) if order is None else [int(v) for v in order]
    if int(iters) > 0 and (not order or min(order) < 0 or max(order) >= V):
        raise ValueError(f"refine_poses: order must index the {V} views")
    images = images.to(dev, torch.float32).contiguous()
    masks = None if masks is None else masks.to(dev, torch.float32).contiguous()
    with torch.cuda.device(dev):
        settings, s = _pose_cameras(poses, T_WC, K, H, W, near, far, bg, dev)
        if rows14.shape[0] == 0 or int(iters) == 0:
            return poses.T_WC, torch.zeros(int(iters), device=dev, dtype=torch.float32)
        means3D, shs, opac, scales, rots = activate(rows14, s)
        leaves = [t.requires_grad_(True) for t in (means3D, scales, rots)]
        render = lambda st: GaussianRasterizer(st)(
            means3D=means3D, means2D=torch.zeros_like(means3D), opacities=opac, shs=shs,
            scales=scales, rotations=rots)
        grad_kw = lambda: dict(means3D=means3D.detach(), d_means3D=means3D.grad,
                               rotations=rots.detach(), d_rotations=rots.grad)
        history = _pose_loop(poses, settings, images, masks, order, iters, leaves, render,
                             grad_kw, dict(mse_weight=mse_weight, l1_weight=l1_weight,
                                           ssim_weight=ssim_weight))
    return poses.T_WC, history


def localise(means3D, cov3D, colors, opacities, image, T_WC, K, iters, mask=None, poses=None,
             l1_weight=0.8, ssim_weight=0.2, mse_weight=0.0, near=0.1, far=1000.0, bg=None):
    """Fit one camera pose to one image of Gaussians given as the rasterizer
    takes them from the map (SharedGaussians.refine_pose): means3D [n, 3] and
    cov3D [n, 6] already times the scale-invariant factor 1 / near and its
    square, colors [n, 3] (colors_precomp), opacities [n, 1]; the covariance
    form of pose_gradient.  image [3, H, W], T_WC [4, 4].  None of the four
    tensors is written.  Returns (T_WC float64 [4, 4] on the device,
    history [iters])."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = means3D.device
    _lib.require_cuda(means3D, cov3D, colors, opacities)
    image = image.reshape(1, 3, *image.shape[-2:]).to(dev, torch.float32).contiguous()
    H, W = image.shape[-2:]
    mask = None if mask is None else mask.reshape(1, H, W).to(dev, torch.float32).contiguous()
    poses = PoseControl() if poses is None else poses
    if not isinstance(poses, PoseControl):
        raise TypeError("localise: poses must be a PoseControl or None")
    with torch.cuda.device(dev):
        settings, _ = _pose_cameras(poses, T_WC.reshape(1, 4, 4), K, H, W, near, far, bg, dev)
        if means3D.shape[0] == 0 or int(iters) == 0:
            return poses.T_WC[0], torch.zeros(int(iters), device=dev, dtype=torch.float32)
        mu = means3D.detach().float().contiguous().clone().requires_grad_(True)
        cov = cov3D.detach().float().contiguous().clone().requires_grad_(True)
        render = lambda st: GaussianRasterizer(st)(
            means3D=mu, means2D=torch.zeros_like(mu), opacities=opacities.detach(), shs=None,
            colors_precomp=colors.detach(), cov3D_precomp=cov)
        grad_kw = lambda: dict(means3D=mu.detach(), d_means3D=mu.grad, cov3D=cov.detach(),
                               d_cov3D=cov.grad)
        history = _pose_loop(poses, settings, image, mask, [0], iters, [mu, cov], render, grad_kw,
                             dict(mse_weight=mse_weight, l1_weight=l1_weight,
                                  ssim_weight=ssim_weight))
    return poses.T_WC[0], history
