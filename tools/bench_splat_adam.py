"""Fused splat optimiser step (include/s3o.h, csrc/splat_opt.hip) against the
torch composition it replaces, same device, same inputs:

  * hip:   s3o_activate + s3o_adam_step, two launches (the step recomputes
           the activations it needs; culled rows load their radius only);
  * torch: the five activations as torch ops under autograd, their backward
           from the same five gradients, and torch.optim.Adam over five
           parameter groups, with its fused implementation (`fused=True`, the
           fastest torch has; `--torch-adam foreach` for the default one).
           It has no sparse form: it steps every row whatever the radii say,
           so its one figure per n is set against the dense hip figure
           (torch_over_hip_dense) and, separately named, against the sparse
           one (dense_torch_over_sparse_hip: what skipping the culled rows
           buys on top).

n = 393,216 and 8,388,608 rows, dense (radii NULL) and sparse with ~10 % of
the rows visible (seeded Bernoulli radii).  Each variant: `--warmup` untimed
calls, then `--rounds` rounds of `--iters` back-to-back calls between two
device events; the median (min - max) per call in microseconds.

Bytes per step, the model of the kernels (what a row moves, not a counter):
activate reads 56 B and writes 56 B per row; the fused step moves 396 B per
visible row (read: 56 B row, 112 B moments, 56 B gradients, 4 B radius;
write: 56 B row, 112 B moments; the dense step has no radius: 392 B) and 4 B
per culled one.  tb_per_s is bytes / time, hbm_fraction_* that over the
8 TB/s peak and over the 6.3 TB/s a streaming kernel achieves on this chip.
At n = 393,216 the 66 MB working set fits the 256 MiB Infinity Cache, so that
size is not an HBM measurement.  One JSON line per (n, case, variant), on
stdout and, with --log, appended to that file as well
(profiles/splat_adam_bench.log is such a file).

python -m tools.bench_splat_adam [--sizes 393216 8388608] [--rounds 10]
                                 [--log profiles/splat_adam_bench.log]"""
from __future__ import annotations

import argparse
import json
import statistics

import torch

from splatt3r_amd.refine import SplatAdam, activate

HBM_PEAK = 8.0e12
HBM_ACHIEVABLE = 6.3e12
LR = dict(means=1.6e-4, f_dc=2.5e-3, opacity=0.05, scale=5e-3, rotation=1e-3)
LOG = None
COLS = dict(means=slice(0, 3), f_dc=slice(3, 6), opacity=slice(6, 7), scale=slice(7, 10),
            rotation=slice(10, 14))


def inputs(n, device, seed=0, visible=0.1):
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device=device)
    rows = torch.empty(n, 14, device=device)
    rows[:, 0:3] = torch.randn(n, 3, generator=g, device=device) * 3
    rows[:, 3:6] = torch.randn(n, 3, generator=g, device=device)
    rows[:, 6] = r(n) * 8 - 4
    rows[:, 7:10] = r(n, 3) * 5 - 7
    rows[:, 10:14] = torch.randn(n, 4, generator=g, device=device)
    grads = [torch.randn(*s, generator=g, device=device) * 1e-3
             for s in ((n, 3), (n, 1, 3), (n, 1), (n, 3), (n, 4))]
    radii = (r(n) < visible).to(torch.int32) * 7
    return rows, grads, radii


def torch_activate(parts, s):
    xyz, fdc, logit, lsc, q = parts
    return (s * xyz, fdc.reshape(-1, 1, 3), torch.sigmoid(logit), s * torch.exp(lsc),
            q / q.norm(dim=1, keepdim=True))


def timed(fn, rounds, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3 / iters)
    return {"median": round(statistics.median(t), 1), "min": round(min(t), 1),
            "max": round(max(t), 1)}


def report(n, case, variant, us, nbytes=None, **extra):
    out = {"n": n, "case": case, "variant": variant, "us": us}
    if nbytes is not None:
        sec = us["median"] * 1e-6
        out.update(bytes=nbytes, tb_per_s=round(nbytes / sec / 1e12, 3),
                   hbm_fraction_of_peak=round(nbytes / sec / HBM_PEAK, 3),
                   hbm_fraction_of_achievable=round(nbytes / sec / HBM_ACHIEVABLE, 3))
    out.update(extra)
    line = json.dumps(out)
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[393216, 8388608])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-rounds", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--render-scale", type=float, default=10.0)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-adam", choices=("fused", "foreach"), default="fused")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    global LOG
    LOG = a.log
    if not torch.cuda.is_available():
        raise SystemExit("bench_splat_adam needs a GPU")
    dev = torch.device("cuda", 0)
    s = a.render_scale
    for n in a.sizes:
        rows, grads, radii = inputs(n, dev)
        vis = int((radii > 0).sum())
        opt = SplatAdam(rows.clone())
        act_us = timed(lambda: activate(opt.rows14, s), a.rounds, a.iters, a.warmup)
        report(n, "activate", "hip", act_us, nbytes=n * 112, launches=1)
        hip = {}
        for case, rd, nbytes in (("dense", None, n * 392),
                                 ("sparse", radii, vis * 396 + (n - vis) * 4)):
            hip[case] = timed(lambda: opt.step(grads, rd, s), a.rounds, a.iters, a.warmup)
            extra = dict(visible_rows=vis) if rd is not None else {}
            report(n, case, "hip_step", hip[case], nbytes=nbytes, launches=1, **extra)
            both = timed(lambda: (activate(opt.rows14, s), opt.step(grads, rd, s)), a.rounds,
                         a.iters, a.warmup)
            hip[case + "_both"] = both
            report(n, case, "hip_activate_plus_step", both, nbytes=nbytes + n * 112, launches=2,
                   **extra)
        if a.no_torch:
            continue
        parts = [rows[:, COLS[g]].clone().requires_grad_(True) for g in LR]
        topt = torch.optim.Adam([dict(params=[p], lr=LR[g]) for p, g in zip(parts, LR)],
                                betas=(0.9, 0.999), eps=1e-15, fused=a.torch_adam == "fused",
                                foreach=a.torch_adam == "foreach")

        def torch_step():
            topt.zero_grad(set_to_none=True)
            torch.autograd.backward(torch_activate(parts, s), grads)
            topt.step()
        us = timed(torch_step, a.torch_rounds, a.torch_iters, 2)
        report(n, "dense", "torch_" + a.torch_adam, us,
               torch_over_hip_dense=round(us["median"] / hip["dense_both"]["median"], 1),
               dense_torch_over_sparse_hip=round(us["median"] / hip["sparse_both"]["median"], 1))
        del parts, topt, opt, rows, grads, radii
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
