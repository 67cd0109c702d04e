"""Depth loss and depth-metric sums (include/s3z.h, csrc/depth_loss.hip)
against a torch composition of the same sums on the same device and inputs,
and what a depth term costs one refine_splats step.

  * hip fwd:       depth.depth_sums (k_depth_fwd + k_depth_sums, no residual
                   map), weights and scales given.
  * hip fwd+bwd:   depth.depth_loss(l1 1, l2 0.5, grad 0.5) and its backward
                   to depth and alpha (the two forward launches, torch's
                   arithmetic on the [B, 14] sums, k_depth_bwd).
  * torch fwd, fwd+bwd:  torch_sums below -- the same fourteen sums in float64
                   with boolean masks and shifted slices -- and autograd of the
                   same loss.  `agree`: the largest relative difference of a sum
                   from the HIP pass.
  * refine step:   one refine_splats step (activate, rasterizer forward,
                   photometric loss, [depth loss,] one backward, fused Adam
                   step) on 393,216 Gaussians, a textured plane seen at
                   384 x 512, with and without depth=DepthControl; a host clock
                   around `--steps` steps between two device synchronises, per
                   step.

Call times: `--warmup` untimed calls, then `--rounds` rounds of `--iters`
back-to-back calls between two device events; median (min - max) per call in
microseconds.  Back-to-back calls of a few microseconds are bounded by the
launches, not the kernels: the kernel times themselves come from a separate
run under `rocprofv3 --kernel-trace --stats` of `--trace-pass` (the HIP calls
only, a fixed number of times), whose kernel-stats CSV `--summarise DIR` turns
into log lines.  bytes = what the algorithm must move: 16 B read per pixel
forward, 16 B read and 8 B written backward.

One JSON line per measurement, on stdout and, with --log, appended to that
file as well (profiles/depth_loss_bench.log is such a file).

python -m tools.depth_loss_bench [--log profiles/depth_loss_bench.log]
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
    python -m tools.depth_loss_bench --trace-pass --batch 32
python -m tools.depth_loss_bench --summarise DIR --batch 32 [--log ...]"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import re
import statistics
import time

import numpy as np
import torch

from tools import bench_map_compact as base
from tools.bench_map_compact import report, timed

H, W = 384, 512
BATCHES = (1, 32)
ALPHA_MIN = 0.5
WEIGHTS = dict(l1_weight=1.0, l2_weight=0.5, grad_weight=0.5)
TRACE_CALLS = 50


def inputs(B, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed + B)
    r = lambda lo, hi: lo + (hi - lo) * torch.rand(B, H, W, generator=g, device=dev)
    z = r(0.5, 4.0)
    A = r(0.3, 1.0)                                   # ~ 29 % below alpha_min
    D = (z * (1.0 + 0.05 * torch.randn(B, H, W, generator=g, device=dev)) * A).contiguous()
    z = torch.where(r(0, 1) < 0.1, torch.zeros_like(z), z)         # 10 % without a target
    w = r(0.25, 2.0)
    s = 0.8 + 0.4 * torch.rand(B, generator=g, device=dev)
    return D, A.contiguous(), z.contiguous(), w.contiguous(), s.contiguous()


def torch_sums(D, A, z, w, s, alpha_min=ALPHA_MIN):
    """The fourteen sums [B, 14] float64 as a plain torch composition."""
    D, A, z, w = (t.double() for t in (D, A, z, w))
    s = s.double()[:, None, None]
    valid = (torch.isfinite(z) & (z > 0) & torch.isfinite(D) & torch.isfinite(A) & (D > 0) & (A > 0)
             & (A >= alpha_min) & torch.isfinite(w) & (w > 0))
    one = torch.ones_like(D)
    q = torch.where(valid, D, one) / torch.where(valid, A, one)
    zs = torch.where(valid, z, one)
    p = s * q
    r = torch.where(valid, p - zs, torch.zeros_like(D))
    wv = torch.where(valid, w, torch.zeros_like(w))
    a = r.abs()
    ratio = torch.maximum(p / zs, zs / p)
    l = p.log() - zs.log()
    vf = valid.double()
    grad = wg = 0
    for lo, hi in (((..., slice(None, -1)), (..., slice(1, None))),
                   ((..., slice(None, -1), slice(None)), (..., slice(1, None), slice(None)))):
        both = (valid[lo] & valid[hi]).double()
        wpq = 0.5 * (wv[lo] + wv[hi]) * both
        grad = grad + (wpq * (r[hi] - r[lo]).abs()).sum((1, 2))
        wg = wg + wpq.sum((1, 2))
    S = lambda t: t.sum((1, 2))
    return torch.stack([S(wv), S(wv * a), S(wv * a * a), S(wv * a / zs), S(wv * a * a / zs),
                        S(wv * l * l), grad, wg, S(vf * (ratio < 1.25)), S(vf * (ratio < 1.5625)),
                        S(vf * (ratio < 1.953125)), S(vf), S(wv * q * zs), S(wv * q * q)], 1)


def loss_of(sums):
    from splatt3r_amd import depth as Dm
    one = torch.ones_like(sums[:, 0])
    w = torch.where(sums[:, Dm.SUM_W] > 0, sums[:, Dm.SUM_W], one).detach()
    wg = torch.where(sums[:, Dm.SUM_WG] > 0, sums[:, Dm.SUM_WG], one).detach()
    return ((WEIGHTS["l1_weight"] * sums[:, Dm.SUM_ABS] + WEIGHTS["l2_weight"] * sums[:, Dm.SUM_SQ]) / w
            + WEIGHTS["grad_weight"] * sums[:, Dm.SUM_GRAD] / wg).mean()


def hip_calls(B, dev):
    from splatt3r_amd import depth as Dm
    D, A, z, w, s = inputs(B, dev)
    Dg, Ag = D.clone().requires_grad_(True), A.clone().requires_grad_(True)

    def fwd():
        return Dm.depth_sums(D, A, z, w, s, ALPHA_MIN)

    def fwd_bwd():
        Dg.grad = Ag.grad = None
        Dm.depth_loss(Dg, Ag, z, w, s, alpha_min=ALPHA_MIN, **WEIGHTS).backward()
    return (D, A, z, w, s), (Dg, Ag), fwd, fwd_bwd


def bench_kernels(a, dev):
    for B in BATCHES:
        (D, A, z, w, s), (Dg, Ag), fwd, fwd_bwd = hip_calls(B, dev)
        n = B * H * W
        common = dict(B=B, H=H, W=W, pixels=n)
        report(variant="hip", what="fwd", us=timed(fwd, a.rounds, a.iters, a.warmup),
               bytes=16 * n, **common)
        report(variant="hip", what="fwd+bwd", us=timed(fwd_bwd, a.rounds, a.iters, a.warmup),
               bytes=(16 + 16 + 8) * n, **common)
        hip_sums = fwd()
        hip_gd = Dg.grad.clone()
        Dt, At = D.clone().requires_grad_(True), A.clone().requires_grad_(True)
        t_sums = torch_sums(D, A, z, w, s)
        agree = float(((t_sums - hip_sums).abs() / hip_sums.abs().clamp_min(1e-300)).max())

        def t_fwd():
            with torch.no_grad():
                return torch_sums(D, A, z, w, s)

        def t_fwd_bwd():
            Dt.grad = At.grad = None
            loss_of(torch_sums(Dt, At, z, w, s)).backward()
        t_fwd_bwd()
        gerr = float((Dt.grad - hip_gd).abs().max() / hip_gd.abs().max())
        report(variant="torch", what="fwd", us=timed(t_fwd, a.torch_rounds, a.torch_iters, 2),
               agree=agree, **common)
        report(variant="torch", what="fwd+bwd",
               us=timed(t_fwd_bwd, a.torch_rounds, a.torch_iters, 2), grad_agree=gerr, **common)
        del D, A, z, w, s, Dg, Ag, Dt, At
        torch.cuda.empty_cache()


def plane_scene(dev, rows_v=768, rows_u=512, depth=2.0, focal=400.0):
    """393,216 Gaussians on a textured fronto-parallel plane filling a
    384 x 512 view (half a pixel apart vertically), two views."""
    from splatt3r_amd.refine import render_splats
    from splatt3r_amd.synthetic import smooth_texture
    v, u = np.meshgrid((np.arange(rows_v) + 0.5) * (H / rows_v), (np.arange(rows_u) + 0.5) * (W / rows_u),
                       indexing="ij")
    xyz = np.stack([(u - W / 2) / focal * depth, (v - H / 2) / focal * depth,
                    np.full(u.shape, depth)], -1).reshape(-1, 3)
    P = xyz.shape[0]
    rows = np.zeros((P, 14), np.float32)
    rows[:, :3] = xyz
    rows[:, 3:6] = (smooth_texture(rows_v, rows_u, 3).transpose(1, 2, 0).reshape(P, 3) - 0.5) / 0.2820948
    rows[:, 6] = 2.0
    rows[:, 7:10] = np.log(0.6 * depth / focal)
    rows[:, 10] = 1.0
    rows = torch.from_numpy(rows).to(dev)
    K = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], dtype=torch.float32)
    T = torch.eye(4).repeat(2, 1, 1)
    T[1, :3, 3] = torch.tensor([0.05, 0.0, 0.1])
    T = T.to(dev)
    images = render_splats(rows, T, K, H, W)
    targets = torch.tensor([depth, depth - 0.1], device=dev).reshape(2, 1, 1).repeat(1, H, W)
    g = torch.Generator(device=dev).manual_seed(1)
    start = rows.clone()
    start[:, :3] *= 1.0 + 0.02 * torch.randn(P, 1, generator=g, device=dev)
    return start.contiguous(), T, K, images, targets.contiguous()


def bench_refine_step(a, dev):
    from splatt3r_amd.refine import DepthControl, refine_splats
    start, T, K, images, targets = plane_scene(dev)
    out = {}
    for name in ("photometric", "photometric+depth") * a.refine_rounds:
        kw = {} if name == "photometric" else dict(depth=DepthControl(targets, grad_weight=0.5))
        refine_splats(start, images, T, K, 4, **kw)                      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, hist = refine_splats(start, images, T, K, a.steps, **kw)
        torch.cuda.synchronize()
        out.setdefault(name, []).append((time.perf_counter() - t0) * 1e6 / a.steps)
        out[name + ".loss"] = (float(hist[0]), float(hist[-1]))
    for name in ("photometric", "photometric+depth"):
        t = out[name]
        report(variant="refine_step", what=name, gaussians=start.shape[0], H=H, W=W, steps=a.steps,
               us={"median": round(statistics.median(t), 1), "min": round(min(t), 1),
                   "max": round(max(t), 1)}, first_last_loss=out[name + ".loss"])
    report(variant="refine_step", what="ratio with / without depth",
           ratio=round(statistics.median(out["photometric+depth"]) /
                       statistics.median(out["photometric"]), 3))


def trace_pass(dev, batches):
    """What the profiler run executes: each HIP call TRACE_CALLS times."""
    for B in batches:
        _, _, fwd, fwd_bwd = hip_calls(B, dev)
        for _ in range(TRACE_CALLS):
            fwd()
        for _ in range(TRACE_CALLS):
            fwd_bwd()
        torch.cuda.synchronize()


def summarise(path, batches):
    """Log lines from rocprofv3's kernel-stats CSV: every k_depth_* kernel of
    a trace pass over `batches` (one batch size per profiler run keeps a
    kernel's calls alike; k_depth_fwd and k_depth_sums run in the forward and
    in the forward of forward + backward, so twice as often as k_depth_bwd)."""
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats*.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel-stats CSV under {path}")
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name", "")
                if "k_depth_" not in name:
                    continue
                num = lambda k: float(row[k]) if row.get(k) not in (None, "") else None
                report(variant="rocprofv3_kernel_stats", kernel=re.search(r"k_depth_\w+", name).group(), calls=num("Calls"),
                       average_ns=num("AverageNs"), min_ns=num("MinNs"), max_ns=num("MaxNs"),
                       total_ns=num("TotalDurationNs"), trace_calls_per_batch=TRACE_CALLS,
                       B=list(batches), H=H, W=W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-rounds", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30, help="refine_splats steps per timing")
    ap.add_argument("--refine-rounds", type=int, default=3)
    ap.add_argument("--no-refine", action="store_true")
    ap.add_argument("--trace-pass", action="store_true", help="only run the HIP calls (profiler)")
    ap.add_argument("--summarise", default=None, help="rocprofv3 output directory to summarise")
    ap.add_argument("--batch", type=int, nargs="+", default=list(BATCHES),
                    help="batch sizes of --trace-pass / --summarise")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    base.LOG = a.log
    if a.summarise:
        summarise(a.summarise, a.batch)
        return
    if not torch.cuda.is_available():
        raise SystemExit("depth_loss_bench needs a GPU")
    dev = torch.device("cuda", 0)
    if a.trace_pass:
        trace_pass(dev, a.batch)
        return
    bench_kernels(a, dev)
    if not a.no_refine:
        bench_refine_step(a, dev)


if __name__ == "__main__":
    main()
