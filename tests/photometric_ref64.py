"""Float64 PyTorch restatement of the photometric definition (include/s3p.h):
explicit reflect indexing, a separable conv2d with the 11-tap Gaussian window,
S and the five per-image sums.  Autograd differentiates it; there is no
derivative code here.  `dtype=torch.float32` runs the same graph in float32
(taps rounded to float32), which is how the tests measure the rounding floor.

`adjoint="nofold"` is the sensitivity ablation: the forward is unchanged, the
backward of the filter is the zero-extended correlation c alone, without the
two terms c(-1 - j) and c(2n - 1 - j) that fold the reflected border back
(include/s3p.h).
"""
import numpy as np
import torch
import torch.nn.functional as F

RADIUS = 5
SIGMA = 1.5
C1 = 0.01 ** 2
C2 = 0.03 ** 2


def window(dtype=torch.float64):
    k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * SIGMA * SIGMA))
    g = g / g.sum()
    return torch.from_numpy(g).to(dtype)


def reflect_index(n):
    """Source index of every position of [-5, n + 5): d c b a | a b c d | d c b a."""
    p = np.arange(-RADIUS, n + RADIUS)
    p = np.where(p < 0, -1 - p, p)
    p = np.where(p >= n, 2 * n - 1 - p, p)
    assert p.min() >= 0 and p.max() < n
    return torch.from_numpy(p)


def _conv_valid(z, g):
    n = z.shape[1]
    z = F.conv2d(z.reshape(-1, 1, *z.shape[-2:]), g.reshape(1, 1, 1, -1))
    z = F.conv2d(z, g.reshape(1, 1, -1, 1))
    return z.reshape(-1, n, *z.shape[-2:])


class _FilterWithoutFold(torch.autograd.Function):
    """Forward: the reflect-padded filter.  Backward: the zero-padded
    correlation of the incoming gradient (the border fold removed)."""

    @staticmethod
    def forward(ctx, z, g):
        ctx.save_for_backward(g)
        return gaussian_filter(z, g)

    @staticmethod
    def backward(ctx, grad):
        (g,) = ctx.saved_tensors
        return _conv_valid(F.pad(grad, (RADIUS,) * 4), g), None


def gaussian_filter(z, g=None, adjoint="Gt"):
    """G z for z [B, C, H, W]."""
    g = window(z.dtype) if g is None else g
    if adjoint == "nofold":
        return _FilterWithoutFold.apply(z, g)
    H, W = z.shape[-2:]
    z = z[..., reflect_index(H), :][..., reflect_index(W)]
    return _conv_valid(z, g)


def ssim_map(x, y, sample_covariance=True, adjoint="Gt"):
    """S [B, C, H, W] of (already masked) x, y."""
    g = window(x.dtype)
    cn = 121.0 / 120.0 if sample_covariance else 1.0
    f = lambda z: gaussian_filter(z, g, adjoint)
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx = cn * (uxx - ux * ux)
    vy = cn * (uyy - uy * uy)
    vxy = cn * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def forward(pred, target, mask=None, sample_covariance=True, dtype=torch.float64, adjoint="Gt"):
    """dict: S map and the five per-image sums (include/s3p.h), plus the
    quantities the Python interface derives from them.  pred may require
    grad (in `dtype`)."""
    x = pred.to(dtype)
    y = target.to(dtype)
    B, C, H, W = x.shape
    if mask is not None:
        m = mask.to(dtype)[:, None]
        x, y = x * m, y * m
    else:
        m = torch.ones(B, 1, H, W, dtype=dtype)
    S = ssim_map(x, y, sample_covariance, adjoint)
    d = x - y
    out = dict(S=S,
               sum_sq=(m * d * d).sum((1, 2, 3)),
               sum_abs=(m * d.abs()).sum((1, 2, 3)),
               sum_ms=(m * S).sum((1, 2, 3)),
               sum_m=m.sum((1, 2, 3)),
               sum_crop=S[..., RADIUS:H - RADIUS, RADIUS:W - RADIUS].sum((1, 2, 3)))
    if mask is not None:
        den = out["sum_m"]
        out["ssim"] = out["sum_ms"] / den
    else:
        den = float(C * H * W)
        out["ssim"] = out["sum_crop"] / float(C * (H - 2 * RADIUS) * (W - 2 * RADIUS))
    out["mse"] = out["sum_sq"] / den
    out["l1"] = out["sum_abs"] / den
    out["psnr"] = -10.0 * torch.log10(out["mse"])
    return out


def loss(pred, target, mask=None, mse_weight=1.0, l1_weight=0.0, ssim_weight=0.0, **kw):
    o = forward(pred, target, mask, **kw)
    return (mse_weight * o["mse"] + l1_weight * o["l1"] + ssim_weight * (1.0 - o["ssim"])).mean()
