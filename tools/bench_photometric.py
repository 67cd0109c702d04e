"""Photometric loss, fused HIP against a torch-op composition of the same
definition on the same device (splatt3r_amd/photometric.py, include/s3p.h).

Both compute  mse + 0.3 l1 + 0.5 (1 - ssim)  of a [1, 3, H, W] image pair:
  * fused: photometric_loss (one tile pass + the finalise of the partial sums;
    backward one launch);
  * torch: explicit reflect indexing, the five moment maps through F.conv2d
    with the separable 11-tap window (a 1 x 11 and an 11 x 1 pass), S and the
    means in elementwise ops; backward by autograd.
Forward alone (no_grad) and forward + backward, the two variants alternating
in one process; device events around every round, `--warmup` rounds, then
`--rounds` timed ones; median (min - max) in microseconds.  The launch counts
are counted, not timed: the aten operators each variant dispatches in one
round that launch a kernel (views and allocations left out), plus the
library's own launches for the fused variant.  s3p_forward_us / s3p_backward_us
are the library calls alone, back to back, without the torch arithmetic on the
five sums around them.

python -m tools.bench_photometric [--rounds 50] [--warmup 3]"""
from __future__ import annotations

import argparse
import json
import statistics

import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

from splatt3r_amd import photometric as PH

WEIGHTS = dict(mse_weight=1.0, l1_weight=0.3, ssim_weight=0.5)
SHAPES = ((1, 3, 384, 512), (1, 3, 540, 960))
# library launches per call: s3p_forward = tile pass + finalise, s3p_backward = 1
HIP_LAUNCHES = {"fwd": 2, "fwd_bwd": 3}
_NO_KERNEL = ("view", "reshape", "expand", "empty", "as_strided", "detach", "alias", "permute",
              "select", "slice", "squeeze", "unsqueeze", "transpose", "t.default", "_to_copy",
              "lift_fresh", "_local_scalar_dense", "unbind", "split")


class _OpCount(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func).replace("aten.", "")
        if not name.startswith(_NO_KERNEL):
            self.n += 1
        return func(*args, **(kwargs or {}))


class TorchComposition:
    """The definition of include/s3p.h in float32 torch ops."""

    def __init__(self, shape, device):
        _, C, H, W = shape
        win = torch.empty(11, dtype=torch.float32)
        PH._lib.lib().s3p_window(win.data_ptr())
        self.gx = win.to(device).reshape(1, 1, 1, 11)
        self.gy = win.to(device).reshape(1, 1, 11, 1)
        self.iy = self._reflect(H).to(device)
        self.ix = self._reflect(W).to(device)
        self.crop = float(C * (H - 10) * (W - 10))

    @staticmethod
    def _reflect(n):
        p = torch.arange(-5, n + 5)
        p = torch.where(p < 0, -1 - p, p)
        return torch.where(p >= n, 2 * n - 1 - p, p)

    def loss(self, x, y):
        B, C, H, W = x.shape
        z = torch.cat([x, y, x * x, y * y, x * y], 1)
        z = z[:, :, self.iy][:, :, :, self.ix].reshape(B * 5 * C, 1, H + 10, W + 10)
        z = F.conv2d(F.conv2d(z, self.gx), self.gy).reshape(B, 5, C, H, W)
        ux, uy, uxx, uyy, uxy = z.unbind(1)
        cn = 121.0 / 120.0
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        S = ((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux * ux + uy * uy + 1e-4)
                                                         * (vx + vy + 9e-4))
        d = x - y
        ssim = S[..., 5:H - 5, 5:W - 5].sum((1, 2, 3)) / self.crop
        per_image = (WEIGHTS["mse_weight"] * (d * d).mean((1, 2, 3))
                     + WEIGHTS["l1_weight"] * d.abs().mean((1, 2, 3))
                     + WEIGHTS["ssim_weight"] * (1.0 - ssim))
        return per_image.mean()


def _variants(shape, device):
    g = torch.Generator().manual_seed(0)
    pred = torch.rand(shape, generator=g).to(device)
    target = torch.rand(shape, generator=g).to(device)
    comp = TorchComposition(shape, device)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(pred, target), None
        return run

    def fwd_bwd(fn):
        def run():
            p = pred.detach().requires_grad_(True)
            loss = fn(p, target)
            loss.backward()
            return loss.detach(), p.grad
        return run

    fused = lambda p, t: PH.photometric_loss(p, t, **WEIGHTS)
    return {("fwd", "fused"): fwd(fused), ("fwd", "torch"): fwd(comp.loss),
            ("fwd_bwd", "fused"): fwd_bwd(fused), ("fwd_bwd", "torch"): fwd_bwd(comp.loss)}


def library_calls_us(shape, device, iters=20):
    """Stream time of the library calls alone (no torch arithmetic on the
    sums): s3p_forward writing the derivative maps, and s3p_backward; device
    events around `iters` back-to-back calls."""
    g = torch.Generator().manual_seed(0)
    pred = torch.rand(shape, generator=g).to(device)
    target = torch.rand(shape, generator=g).to(device)
    coef = torch.tensor([[1.0, 0.3, 0.0, -0.5]] * shape[0], device=device)
    _, _, derivs = PH._run_forward(pred, target, None, True, False, True)
    calls = {"s3p_forward": lambda: PH._run_forward(pred, target, None, True, False, True),
             "s3p_backward": lambda: PH._run_backward(pred, target, None, derivs, None, coef)}
    out = {}
    for name, call in calls.items():
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        e1.synchronize()
        out[name + "_us"] = round(e0.elapsed_time(e1) * 1e3 / iters, 1)
    return out


def bench_shape(shape, device, rounds, warmup):
    runs = _variants(shape, device)
    out = {"shape": list(shape)}
    out.update(library_calls_us(shape, device))
    # the two variants agree (float32 rounding apart)
    for what in ("fwd", "fwd_bwd"):
        (lf, gf), (lt, gt) = runs[(what, "fused")](), runs[(what, "torch")]()
        out[f"{what}_loss_rel_diff"] = float((lf - lt).abs() / lt.abs())
        if gf is not None:
            out["grad_rel_diff"] = float((gf - gt).abs().max() / gt.abs().max())
    for key, run in runs.items():
        with _OpCount() as oc:
            run()
        n = oc.n + (HIP_LAUNCHES[key[0]] if key[1] == "fused" else 0)
        out[f"{key[0]}_{key[1]}_launching_ops"] = n
    times = {k: [] for k in runs}
    for r in range(warmup + rounds):
        for key, run in runs.items():           # variants alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[key].append(e0.elapsed_time(e1) * 1e3)
    for key, v in times.items():
        out[f"{key[0]}_{key[1]}_us"] = {"median": round(statistics.median(v), 1),
                                        "min": round(min(v), 1), "max": round(max(v), 1)}
    for what in ("fwd", "fwd_bwd"):
        out[f"{what}_torch_over_fused"] = round(
            out[f"{what}_torch_us"]["median"] / out[f"{what}_fused_us"]["median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photometric needs a GPU")
    device = torch.device("cuda", 0)
    for shape in SHAPES:
        print(json.dumps(bench_shape(shape, device, a.rounds, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
