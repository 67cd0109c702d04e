"""Depth loss and depth metrics on the device (include/s3z.h): rendered depth
against target depth, forward and backward, with no host round trip.

The reference has no counterpart: it neither supervises nor scores rendered
depth.  One HIP pass (csrc/depth_loss.hip) turns the rasterizer's
return_depth outputs -- depth D = sum z alpha T and alpha A = sum alpha T --
a target depth z, an optional per-pixel weight and an optional per-image scale
into the residual map r = s D / A - z and fourteen per-image double-precision
sums; everything below is arithmetic on those sums.  The backward is a second
HIP pass producing dL/dD and dL/dA of the three sums a loss is made of
(w |r|, w r^2 and the gradient-matching term of MiDaS).

A pixel counts when z, D, A and w are finite, z > 0, D > 0, A > 0,
A >= alpha_min and w > 0 (and the image's scale is finite and > 0); a mask is a
0 / 1 weight.  The sums of an image do not depend on the batch it is in, and
the same input gives the same bits.

Importing this module does not initialise the GPU; arguments are validated
before it is required.
"""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

from splatt3r_amd import _abi, _lib

SUM_NAMES = ("W", "ABS", "SQ", "ABSREL", "SQREL", "LOGSQ", "GRAD", "WG", "D1", "D2", "D3", "N",
             "QZ", "QQ")
(SUM_W, SUM_ABS, SUM_SQ, SUM_ABSREL, SUM_SQREL, SUM_LOGSQ, SUM_GRAD, SUM_WG, SUM_D1, SUM_D2,
 SUM_D3, SUM_N, SUM_QZ, SUM_QQ) = (_abi.constants["S3Z_SUM_" + k] for k in SUM_NAMES)
NSUMS = _abi.constants["S3Z_NSUMS"]
TILE_W, TILE_H = _abi.constants["S3Z_TILE_W"], _abi.constants["S3Z_TILE_H"]
ALIGN = (None, "scale", "global")
METRIC_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "l1", "d1", "d2", "d3", "valid", "scale")


# ------------------------------------------------------------- validation --
def _check(depth, alpha, target, weight, scale, alpha_min, fn):
    """Types, shapes and values first, then the device; returns (B, H, W)."""
    named = [("depth", depth), ("alpha", alpha), ("target", target)]
    if weight is not None:
        named.append(("weight", weight))
    if scale is not None and not isinstance(scale, (int, float)):
        named.append(("scale", scale))
    for name, t in named:
        if not torch.is_tensor(t):
            raise TypeError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{fn}: {name} must be float32, got {t.dtype}")
    if depth.dim() != 3:
        raise ValueError(f"{fn}: depth must be [B, H, W], got {tuple(depth.shape)}")
    B, H, W = depth.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{fn}: empty input {tuple(depth.shape)}")
    for name, t in named[1:]:
        want = (B,) if name == "scale" else (B, H, W)
        if tuple(t.shape) != want:
            raise ValueError(f"{fn}: {name} must be {list(want)}, got {tuple(t.shape)}")
    if isinstance(scale, (int, float)) and not (math.isfinite(scale) and scale > 0):
        raise ValueError(f"{fn}: scale must be > 0 and finite, got {scale}")
    alpha_min = float(alpha_min)
    if not (alpha_min >= 0.0 and math.isfinite(alpha_min)):
        raise ValueError(f"{fn}: alpha_min must be >= 0 and finite, got {alpha_min}")
    tensors = [t for _, t in named]
    if any(t.device != depth.device for t in tensors):
        raise RuntimeError(f"{fn}: depth, alpha, target, weight and scale must be on one device")
    _lib.require_cuda(*tensors)
    return B, H, W


def _prep(depth, alpha, target, weight, scale, alpha_min, fn):
    B, _, _ = _check(depth, alpha, target, weight, scale, alpha_min, fn)
    if isinstance(scale, (int, float)):
        scale = torch.full((B,), float(scale), dtype=torch.float32, device=depth.device)
    det = lambda t: None if t is None else t.detach().contiguous()
    return depth.contiguous(), alpha.contiguous(), det(target), det(weight), det(scale), \
        float(alpha_min)


def _run_forward(depth, alpha, target, weight, scale, alpha_min, want_map):
    """(sums [B, NSUMS] float64, residual map [B, H, W] or None)."""
    B, H, W = depth.shape
    dev = depth.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        sums = torch.empty((B, NSUMS), dtype=torch.float64, device=dev)
        rmap = torch.empty_like(depth) if want_map else None
        ws = torch.empty(L.s3z_workspace_bytes(B, H, W) // 8, dtype=torch.float64, device=dev)
        _lib.call("s3z_forward", depth.data_ptr(), alpha.data_ptr(), target.data_ptr(),
                  _lib.ptr(weight), _lib.ptr(scale), B, H, W, alpha_min, _lib.ptr(rmap),
                  sums.data_ptr(), ws.data_ptr(), _lib.stream(dev))
    return sums, rmap


def _run_backward(depth, alpha, target, weight, scale, coef, alpha_min):
    B, H, W = depth.shape
    dev = depth.device
    with torch.cuda.device(dev):
        gd, ga = torch.empty_like(depth), torch.empty_like(depth)
        _lib.call("s3z_backward", depth.data_ptr(), alpha.data_ptr(), target.data_ptr(),
                  _lib.ptr(weight), _lib.ptr(scale), coef.data_ptr(), B, H, W, alpha_min,
                  gd.data_ptr(), ga.data_ptr(), _lib.stream(dev))
    return gd, ga


class _Sums(torch.autograd.Function):
    """(depth, alpha) -> the per-image sums [B, NSUMS] (float64).  Gradient to
    depth and alpha only, and only through the sums ABS, SQ and GRAD: the
    incoming dL/dsums of those three are the backward kernel's per-image
    coefficients.  The scale is a constant (a stop-gradient)."""

    @staticmethod
    def forward(ctx, depth, alpha, target, weight, scale, alpha_min):
        sums, _ = _run_forward(depth, alpha, target, weight, scale, alpha_min, False)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(depth, alpha, target, weight, scale)
            ctx.alpha_min = alpha_min
        return sums

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        depth, alpha, target, weight, scale = ctx.saved_tensors
        coef = g[:, [SUM_ABS, SUM_SQ, SUM_GRAD]].to(torch.float32).contiguous()
        gd, ga = _run_backward(depth, alpha, target, weight, scale, coef, ctx.alpha_min)
        return gd, ga, None, None, None, None


# ------------------------------------------------------- public interface --
def depth_sums(depth, alpha, target, weight=None, scale=None, alpha_min=0.5):
    """The per-image sums [B, NSUMS] float64 of include/s3z.h (index them with
    SUM_W ... SUM_QQ), differentiable in depth and alpha through SUM_ABS,
    SUM_SQ and SUM_GRAD.  depth, alpha, target, weight: [B, H, W] float32;
    scale: a float32 [B] tensor, a number, or None for 1."""
    args = _prep(depth, alpha, target, weight, scale, alpha_min, "depth_sums")
    return _Sums.apply(*args)


@torch.no_grad()
def depth_residuals(depth, alpha, target, weight=None, scale=None, alpha_min=0.5):
    """(sums, r): the sums and the residual map r = s D / A - z [B, H, W]
    float32, 0 at pixels that do not count.  No gradient."""
    args = _prep(depth, alpha, target, weight, scale, alpha_min, "depth_residuals")
    return _run_forward(*args, True)


@torch.no_grad()
def depth_backward(depth, alpha, target, coef, weight=None, scale=None, alpha_min=0.5):
    """(dL/ddepth, dL/dalpha) [B, H, W] float32 of L = sum_b coef[b] . (ABS, SQ,
    GRAD)[b]: s3z_backward as it is, coef a float32 [B, 3] tensor."""
    fn = "depth_backward"
    B = depth.shape[0] if torch.is_tensor(depth) and depth.dim() == 3 else None
    if B is not None and (not torch.is_tensor(coef) or coef.dtype != torch.float32
                          or tuple(coef.shape) != (B, 3)):
        raise ValueError(f"{fn}: coef must be a float32 [{B}, 3] tensor")
    _lib.require_cuda(coef)
    args = _prep(depth, alpha, target, weight, scale, alpha_min, fn)
    return _run_backward(*args[:5], coef.contiguous(), args[5])


def least_squares_scale(sums, per_view=True):
    """The scale s minimising sum w (s q - z)^2, from sums taken without a
    scale: QZ / QQ per image, or with per_view=False sum QZ / sum QQ over the
    batch (repeated per image).  [B] float64; 1 where QQ = 0."""
    qz, qq = sums[:, SUM_QZ], sums[:, SUM_QQ]
    if not per_view:
        qz, qq = qz.sum().expand_as(qz), qq.sum().expand_as(qq)
    ok = qq > 0
    return torch.where(ok, qz / torch.where(ok, qq, torch.ones_like(qq)), torch.ones_like(qq))


@torch.no_grad()
def depth_metrics(depth, alpha, target, weight=None, align=None, alpha_min=0.5):
    """Per-image dict of [B] float64 device tensors: abs_rel, sq_rel, rmse,
    rmse_log, l1 (weighted means over the pixels that count), d1, d2, d3 (the
    share of those pixels with max(p / z, z / p) < 1.25^k, unweighted), valid
    (their share of the image) and scale (the scale applied to D / A).

    align None: no scale.  "scale": each image's own least-squares scale;
    "global": one least-squares scale for the batch.  With either there are
    two forward launches: the first reads QZ and QQ, the second uses the
    resulting scale (rounded to float32, the kernel's type).  Median scaling
    is not offered: it needs a selection over the pixels, which this pass of
    sums cannot give.

    An image with no pixel that counts reports NaN for the means and the
    shares d1..d3, and 0 for valid; nothing raises and nothing is read back."""
    if align not in ALIGN:
        raise ValueError(f"depth_metrics: align must be one of {ALIGN}, got {align!r}")
    args = _prep(depth, alpha, target, weight, None, alpha_min, "depth_metrics")
    sums, _ = _run_forward(*args, False)
    B, H, W = depth.shape
    if align is None:
        scale = torch.ones(B, dtype=torch.float64, device=depth.device)
    else:
        s32 = least_squares_scale(sums, per_view=align == "scale").to(torch.float32)
        sums, _ = _run_forward(*args[:4], s32.contiguous(), args[5], False)
        scale = s32.to(torch.float64)
    w, n = sums[:, SUM_W], sums[:, SUM_N]
    return dict(abs_rel=sums[:, SUM_ABSREL] / w, sq_rel=sums[:, SUM_SQREL] / w,
                rmse=(sums[:, SUM_SQ] / w).sqrt(), rmse_log=(sums[:, SUM_LOGSQ] / w).sqrt(),
                l1=sums[:, SUM_ABS] / w, d1=sums[:, SUM_D1] / n, d2=sums[:, SUM_D2] / n,
                d3=sums[:, SUM_D3] / n, valid=n / float(H * W), scale=scale)


def depth_loss(depth, alpha, target, weight=None, scale=None, l1_weight=1.0, l2_weight=0.0,
               grad_weight=0.0, alpha_min=0.5):
    """mean over the batch of
        (l1_weight ABS + l2_weight SQ) / W + grad_weight GRAD / WG,
    i.e. the weighted mean |r| and r^2 over the pixels that count plus the
    weighted mean |r_q - r_p| over the pairs of neighbouring pixels that both
    count.  A term whose denominator is 0 contributes 0.  Scalar float32;
    gradient to depth and alpha only (one backward launch), the scale a
    constant."""
    sums = depth_sums(depth, alpha, target, weight, scale, alpha_min)
    one = torch.ones_like(sums[:, SUM_W])
    w = torch.where(sums[:, SUM_W] > 0, sums[:, SUM_W], one).detach()
    wg = torch.where(sums[:, SUM_WG] > 0, sums[:, SUM_WG], one).detach()
    per_image = (l1_weight * sums[:, SUM_ABS] + l2_weight * sums[:, SUM_SQ]) / w \
        + grad_weight * sums[:, SUM_GRAD] / wg
    return per_image.mean().to(torch.float32)
