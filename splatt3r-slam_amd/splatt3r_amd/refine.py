"""Photometric refinement of Gaussian splats (include/s3o.h): fit the map's
3DGS parameter rows to the images they came from.

  activate       rows14 -> the five tensors GaussianRasterizer takes (one HIP
                 launch, csrc/splat_opt.hip k_splat_activate)
  SplatAdam      the fused chain rule + Adam step over the rows (one HIP
                 launch, k_splat_adam), sparse over the Gaussians a view did
                 not touch
  refine_splats  the loop: activate, render, photometric loss, backward, step
  render_splats  the images that loop compares against its targets

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

from splatt3r_amd import _lib

GROUPS = ("means", "f_dc", "opacity", "scale", "rotation")


class S3oAdam(ctypes.Structure):
    """s3o_adam of include/s3o.h."""
    _fields_ = [("lr", ctypes.c_float * 5), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("eps", ctypes.c_float), ("bias1", ctypes.c_float),
                ("bias2_sqrt", ctypes.c_float), ("render_scale", ctypes.c_float)]


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
                  mse_weight=0.0, near=0.1, far=1000.0, bg=None, sparse=True, order=None, **lr):
    """Fit splat rows to images.  rows14 [n, 14] float32 on the GPU (a copy is
    refined; the argument is left as it is), images [V, 3, H, W] in [0, 1],
    T_WC [V, 4, 4] camera-to-world, K [3, 3] pixel intrinsics, masks
    [V, H, W] or None, bg a colour triple (default black).  One view per
    step, round-robin, or the sequence `order` gives; every step is
    activate -> render.camera_settings (scale-invariant, factor 1 / near) ->
    GaussianRasterizer(scales, rotations, shs, sh_degree 0) ->
    photometric_loss -> one backward -> one fused SplatAdam step, on that
    forward's radii when `sparse`.  **lr: SplatAdam's keyword arguments.

    Returns (rows14, history): the refined rows and the per-step losses
    [iters] as a device tensor (the loss before each step).  The loop itself
    reads nothing back from the device (the rasterizer's forward reads its
    instance count, as in every differentiable render)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from splatt3r_amd.photometric import photometric_loss
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
    if int(iters) == 0 or rows.shape[0] == 0:
        return rows, history
    with torch.cuda.device(dev):
        settings, s = _cameras(T_WC, K, H, W, near, far, bg, dev)
        for it in range(int(iters)):
            v = order[it % len(order)]
            acts = [t.requires_grad_(True) for t in activate(rows, s)]
            means3D, shs, opac, scales, rots = acts
            img, radii = GaussianRasterizer(settings[v])(
                means3D=means3D, means2D=torch.zeros_like(means3D), opacities=opac, shs=shs,
                scales=scales, rotations=rots)
            loss = photometric_loss(img[None], images[v:v + 1],
                                    None if masks is None else masks[v:v + 1],
                                    mse_weight=mse_weight, l1_weight=l1_weight,
                                    ssim_weight=ssim_weight)
            loss.backward()
            history[it] = loss.detach()
            opt.step([a.grad for a in acts], radii if sparse else None, s)
    return rows, history
