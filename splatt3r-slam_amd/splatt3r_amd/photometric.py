"""Photometric loss and render-quality metrics on the device (include/s3p.h):
masked MSE / L1, PSNR and Gaussian-window SSIM of rendered against camera
images, forward and backward, with no host round trip.

The reference decides both in splatt3r_core/main.py: calculate_loss
(:199-247) is a masked MSE (+ LPIPS, + the MASt3R term), log_metrics
(:249-258) reports psnr = -10 log10(mse) and a masked SSIM, and
utils/compute_ssim.py calls skimage's structural_similarity(win_size=11,
gaussian_weights=True, channel_axis=0, data_range=1.0) per image on the host.
Here one HIP pass (csrc/photometric.hip) produces the S map and five
per-image sums -- sum m (x-y)^2, sum m |x-y|, sum m S, sum m and sum S over
the 5-pixel crop -- and everything below is arithmetic on those sums; the
backward is a second HIP pass producing dL/dpred.

Normalisation follows the reference exactly.  With a mask the sums run over
all channels and are divided by mask.sum(), which counts pixels, not channel
values: the masked MSE, L1 and SSIM of a 3-channel image are 3 x the
per-channel mean.  Without a mask they are plain means (SSIM: skimage's
full=False mean over the crop [5, H-5) x [5, W-5)).

Importing this module does not initialise the GPU; arguments are validated
before it is required.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from splatt3r_amd import _abi, _lib

SUM_SQ, SUM_ABS, SUM_MS, SUM_M, SUM_CROP, NSUMS = (
    _abi.constants[k] for k in ("S3P_SUM_SQ", "S3P_SUM_ABS", "S3P_SUM_MS", "S3P_SUM_M",
                                "S3P_SUM_CROP", "S3P_NSUMS"))
WIN = 11
RADIUS = 5


# ------------------------------------------------------------- validation --
def _check(pred, target, mask, fn):
    for name, t in (("pred", pred), ("target", target)) + ((("mask", mask),) if mask is not None
                                                            else ()):
        if not torch.is_tensor(t):
            raise TypeError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{fn}: {name} must be float32, got {t.dtype}")
    if pred.dim() != 4:
        raise ValueError(f"{fn}: pred must be [B, C, H, W], got {tuple(pred.shape)}")
    if pred.shape != target.shape:
        raise ValueError(f"{fn}: pred {tuple(pred.shape)} and target {tuple(target.shape)} "
                         "differ in shape")
    B, C, H, W = pred.shape
    if B < 1:
        raise ValueError(f"{fn}: empty batch")
    if C not in (1, 3):
        raise ValueError(f"{fn}: C = {C}, expected 1 or 3 channels")
    if H < WIN or W < WIN:
        # skimage: "win_size exceeds image extent"
        raise ValueError(f"{fn}: win_size {WIN} exceeds image extent {H} x {W}")
    if mask is not None and tuple(mask.shape) != (B, H, W):
        raise ValueError(f"{fn}: mask must be [B, H, W] = {(B, H, W)}, got {tuple(mask.shape)}")
    _lib.require_cuda(pred, target, mask)
    if target.device != pred.device or (mask is not None and mask.device != pred.device):
        raise RuntimeError(f"{fn}: pred, target and mask must be on one device")
    return B, C, H, W


def _run_forward(pred, target, mask, sample_covariance, want_map, want_derivs):
    """(sums [B, 5] float64, S map or None, derivs [3, B, C, H, W] or None)."""
    B, C, H, W = pred.shape
    dev = pred.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        sums = torch.empty((B, NSUMS), dtype=torch.float64, device=dev)
        smap = torch.empty_like(pred) if want_map else None
        derivs = torch.empty((3, B, C, H, W), dtype=torch.float32, device=dev) if want_derivs \
            else None
        ws = torch.empty(L.s3p_workspace_bytes(B, C, H, W), dtype=torch.uint8, device=dev)
        _lib.call("s3p_forward", pred.data_ptr(), target.data_ptr(), _lib.ptr(mask), B, C, H, W,
                  int(bool(sample_covariance)), _lib.ptr(smap), _lib.ptr(derivs),
                  sums.data_ptr(), ws.data_ptr(), _lib.stream(dev))
    return sums, smap, derivs


def _run_backward(pred, target, mask, derivs, wmap, coef):
    B, C, H, W = pred.shape
    dev = pred.device
    with torch.cuda.device(dev):
        grad = torch.empty_like(pred)
        _lib.call("s3p_backward", pred.data_ptr(), target.data_ptr(), _lib.ptr(mask),
                  derivs.data_ptr(), _lib.ptr(wmap), coef.data_ptr(), B, C, H, W,
                  grad.data_ptr(), _lib.stream(dev))
    return grad


class _Sums(torch.autograd.Function):
    """pred -> the five per-image sums [B, 5] (float64).  Gradient to pred
    only: the incoming dL/dsums are the backward kernel's per-image
    coefficients."""

    @staticmethod
    def forward(ctx, pred, target, mask, sample_covariance):
        need = ctx.needs_input_grad[0]
        sums, _, derivs = _run_forward(pred, target, mask, sample_covariance, False, need)
        if need:
            ctx.save_for_backward(pred, target, mask, derivs)
        return sums

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pred, target, mask, derivs = ctx.saved_tensors
        coef = g[:, [SUM_SQ, SUM_ABS, SUM_MS, SUM_CROP]].to(torch.float32).contiguous()
        return _run_backward(pred, target, mask, derivs, None, coef), None, None, None


class _Map(torch.autograd.Function):
    """pred -> the S map [B, C, H, W], for arbitrary upstream gradients."""

    @staticmethod
    def forward(ctx, pred, target, mask, sample_covariance):
        need = ctx.needs_input_grad[0]
        _, smap, derivs = _run_forward(pred, target, mask, sample_covariance, True, need)
        if need:
            ctx.save_for_backward(pred, target, mask, derivs)
        return smap

    @staticmethod
    @once_differentiable
    def backward(ctx, w):
        pred, target, mask, derivs = ctx.saved_tensors
        coef = torch.zeros((pred.shape[0], 4), dtype=torch.float32, device=pred.device)
        return _run_backward(pred, target, mask, derivs, w.contiguous(), coef), None, None, None


def _prep(pred, target, mask, fn):
    _check(pred, target, mask, fn)
    return (pred.contiguous(), target.detach().contiguous(),
            None if mask is None else mask.detach().contiguous())


def _sums(pred, target, mask, sample_covariance, fn):
    pred, target, mask = _prep(pred, target, mask, fn)
    return _Sums.apply(pred, target, mask, bool(sample_covariance))


def _terms(sums, shape, masked):
    """Per-image (mse, l1, ssim) in float64 from the sums."""
    _, C, H, W = shape
    if masked:
        den = sums[:, SUM_M]
        ssim_ = sums[:, SUM_MS] / den
    else:
        den = float(C * H * W)
        ssim_ = sums[:, SUM_CROP] / float(C * (H - 2 * RADIUS) * (W - 2 * RADIUS))
    return sums[:, SUM_SQ] / den, sums[:, SUM_ABS] / den, ssim_


# ------------------------------------------------------- public interface --
def ssim_map(pred, target, mask=None, sample_covariance=True):
    """The S map [B, C, H, W] of pred against target (both multiplied by the
    mask first when one is given), differentiable in pred."""
    pred, target, mask = _prep(pred, target, mask, "ssim_map")
    return _Map.apply(pred, target, mask, bool(sample_covariance))


def ssim(pred, target, mask=None, full=False, sample_covariance=True):
    """full=True: the S map.  Otherwise the per-image SSIM [B]: the mean of S
    over channels and the crop [5, H-5) x [5, W-5) (skimage full=False), or
    with a mask sum(m S) / sum(m) (the reference's average_over_mask; 3 x the
    per-channel mean for C = 3, see the module docstring).

    sample_covariance: skimage's use_sample_covariance, which stays at its
    default True in the reference's call: covariances are scaled by
    121 / 120."""
    if full:
        return ssim_map(pred, target, mask, sample_covariance)
    sums = _sums(pred, target, mask, sample_covariance, "ssim")
    return _terms(sums, pred.shape, mask is not None)[2].to(torch.float32)


@torch.no_grad()
def compute_ssim(ground_truth, predicted, full=True):
    """utils/compute_ssim.py: [B, C, H, W] S maps with full=True, else the
    per-image crop means [B]; on the device, no host round trip."""
    return ssim(predicted, ground_truth, None, full=full)


@torch.no_grad()
def image_metrics(pred, target, mask=None):
    """Per-image dict of mse, psnr, ssim, l1 ([B] float32) from one forward
    pass.  psnr = -10 log10(mse) (data range 1).  With a mask the reference's
    normalisation: the sums over ALL channels divided by mask.sum(), i.e.
    3 x the per-channel mean for an RGB image (main.py:217-218, :236-238);
    without a mask plain means (ssim: over the 5-pixel crop)."""
    sums = _sums(pred, target, mask, True, "image_metrics")
    mse, l1, ssim_ = _terms(sums, pred.shape, mask is not None)
    f = lambda t: t.to(torch.float32)
    return dict(mse=f(mse), psnr=f(-10.0 * torch.log10(mse)), ssim=f(ssim_), l1=f(l1))


def photometric_loss(pred, target, mask=None, mse_weight=1.0, l1_weight=0.0, ssim_weight=0.0):
    """mean over the batch of  mse_weight mse + l1_weight l1 + ssim_weight
    (1 - ssim), each term normalised per image as in image_metrics.  Scalar
    float32; gradient to pred only (one backward launch: the three per-image
    coefficients go to the kernel, the SSIM weight map is formed there from
    the mask or the crop)."""
    sums = _sums(pred, target, mask, True, "photometric_loss")
    mse, l1, ssim_ = _terms(sums, pred.shape, mask is not None)
    per_image = mse_weight * mse + l1_weight * l1 + ssim_weight * (1.0 - ssim_)
    return per_image.mean().to(torch.float32)


def calculate_loss(target_color, predicted_color, mask, apply_mask=True, average_over_mask=True,
                   calculate_ssim=False, mse_loss_weight=1.0):
    """main.py:199-247 without the LPIPS and the MASt3R terms (neither can be
    built here).  target_color, predicted_color: [B, V, C, H, W] or
    [B, C, H, W]; mask: [B, V, H, W] or [B, H, W].  Returns (loss, mse_loss)
    or with calculate_ssim (loss, mse_loss, ssim_val), normalised over the
    whole batch as the reference does: average_over_mask divides the sums of
    all images by mask.sum().  Differentiable in predicted_color (the
    reference's SSIM is not; here it is, but it does not enter the loss)."""
    if predicted_color.dim() == 5:
        predicted_color = predicted_color.flatten(0, 1)
        target_color = target_color.flatten(0, 1)
        mask = mask.flatten(0, 1) if mask is not None and mask.dim() == 4 else mask
    if (apply_mask or average_over_mask) and mask is None:
        raise ValueError("calculate_loss: apply_mask / average_over_mask need a mask")
    if apply_mask and average_over_mask:
        sums = _sums(predicted_color, target_color, mask, True, "calculate_loss")
        den = sums[:, SUM_M].sum()
        mse = sums[:, SUM_SQ].sum() / den
        ssim_val = sums[:, SUM_MS].sum() / den
    elif average_over_mask:
        # unmasked images, masked average.  m (p - t)^2 is the masked kernel's
        # squared term for a 0 / 1 mask; S is of the unmasked images, weighted
        # outside the kernel
        sums = _sums(predicted_color, target_color, mask, True, "calculate_loss")
        den = sums[:, SUM_M].sum()
        mse = sums[:, SUM_SQ].sum() / den
        ssim_val = None
        if calculate_ssim:
            S = ssim_map(predicted_color, target_color)
            ssim_val = (S * mask[:, None]).to(torch.float64).sum() / den
    else:
        sums = _sums(predicted_color, target_color, mask if apply_mask else None, True,
                     "calculate_loss")
        B, C, H, W = predicted_color.shape
        mse = sums[:, SUM_SQ].sum() / float(B * C * H * W)
        ssim_val = sums[:, SUM_CROP].sum() / float(B * C * (H - 2 * RADIUS) * (W - 2 * RADIUS))
    mse = mse.to(torch.float32)
    loss = mse_loss_weight * mse
    if calculate_ssim:
        return loss, mse, ssim_val.to(torch.float32)
    return loss, mse
