"""Pose-gradient reduction (include/s3x.h, csrc/pose_grad.hip) against a torch
composition of the same formula, same device, same inputs:

  * hip:   s3x_pose_grad, two launches (the per-row terms with the workgroup
           partials, then one workgroup over the partials), double
           throughout, culled rows load their radius only;
  * torch: the formula as float64 torch ops over the whole arrays (it has no
           sparse form short of a gather, which is what the sparse variant
           does: index the visible rows, then the dense formula on them).

n = 393,216 and 8,388,608 rows, dense (radii None) and sparse with ~10 % of
the rows visible (seeded Bernoulli radii), covariance and rotation form.  Each
variant: `--warmup` untimed calls, then `--rounds` rounds of `--iters`
back-to-back calls between two device events; the median (min - max) per call
in microseconds.

Bytes per call, the model of the kernel (what a row moves, not a counter): a
visible row loads 24 B of mean and mean gradient and 48 B (covariance form)
or 32 B (rotation form) of shape and shape gradient, plus its 4 B radius when
radii are given: 76 B / 60 B sparse, 72 B / 56 B dense; a culled row 4 B.  The
partials are 48 B per 2,048 rows, written and read once.  tb_per_s is bytes /
time, hbm_fraction_* that over the 8 TB/s peak and over the 6.3 TB/s a
streaming kernel achieves on this chip.  At n = 393,216 the working set fits
the 256 MiB Infinity Cache, so that size is not an HBM measurement.  One JSON
line per (n, form, case, variant), on stdout and, with --log, appended to that
file as well (profiles/pose_grad_bench.log is such a file).

python -m tools.bench_pose_grad [--sizes 393216 8388608] [--rounds 10]
                                [--log profiles/pose_grad_bench.log]"""
from __future__ import annotations

import argparse
import json
import statistics

import torch

from splatt3r_amd.refine import pose_gradient

HBM_PEAK = 8.0e12
HBM_ACHIEVABLE = 6.3e12
LOG = None
ROWS_PER_BLOCK = 2048


def inputs(n, form, device, seed=0, visible=0.1):
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    c, s = 0.9553364891256060, 0.2955202066613396          # a rotation by 0.3 rad about y
    vm = torch.tensor([[c, 0, -s, 0], [0, 1, 0, 0], [s, 0, c, 0], [0.1, -0.2, 0.3, 1]],
                      device=device) * torch.tensor([0.8, 0.8, 0.8, 1.0], device=device)
    mu, dmu = rn(n, 3) * 3, rn(n, 3) * 1e-3
    if form == "cov":
        L = rn(n, 3, 3) * 0.1
        S = L @ L.transpose(1, 2)
        iu = torch.triu_indices(3, 3, device=device)
        shape, dshape = S[:, iu[0], iu[1]].contiguous(), rn(n, 6) * 1e-3
    else:
        q = rn(n, 4)
        shape, dshape = q / q.norm(dim=1, keepdim=True), rn(n, 4) * 1e-3
    radii = (torch.rand(n, generator=g, device=device) < visible).to(torch.int32) * 7
    return vm, mu, dmu, shape, dshape, radii


def torch_pose_grad(vm, mu, dmu, shape, dshape, form):
    """The formula of include/s3x.h in float64 torch ops."""
    vm = vm.double()
    A, b = vm[:3, :3].T, vm[3, :3]
    Ait = torch.linalg.inv(A).T
    t = mu.double() @ A.T + b
    g = dmu.double() @ Ait.T
    phi = torch.linalg.cross(t, g)
    if form == "cov":
        ix = torch.tensor([[0, 1, 2], [1, 3, 4], [2, 4, 5]], device=mu.device)
        half = torch.tensor([[1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 1.0]], device=mu.device,
                            dtype=torch.float64)
        Sv = A @ shape.double()[:, ix] @ A.T
        Gv = Ait @ (dshape.double()[:, ix] * half) @ Ait.T
        X = Gv @ Sv
        X = X - X.transpose(1, 2)
        phi = phi + 2.0 * torch.stack([X[:, 2, 1], X[:, 0, 2], X[:, 1, 0]], -1)
    else:
        q, dq = shape.double(), dshape.double()
        r, qv, dr, dv = q[:, :1], q[:, 1:], dq[:, :1], dq[:, 1:]
        w = 0.5 * (r * dv - dr * qv + torch.linalg.cross(qv, dv))
        Rc = A / torch.linalg.det(A).abs().pow(1.0 / 3.0)
        phi = phi + w @ Rc.T
    return -torch.cat([g.sum(0), phi.sum(0)])


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


def report(n, form, case, variant, us, nbytes=None, **extra):
    out = {"n": n, "form": form, "case": case, "variant": variant, "us": us}
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
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    global LOG
    LOG = a.log
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_grad needs a GPU")
    dev = torch.device("cuda", 0)
    for n in a.sizes:
        for form, width in (("cov", 48), ("rot", 32)):
            vm, mu, dmu, shape, dshape, radii = inputs(n, form, dev)
            kw = dict(cov3D=shape, d_cov3D=dshape) if form == "cov" else \
                dict(rotations=shape, d_rotations=dshape)
            vis = int((radii > 0).sum())
            partials = 2 * 48 * -(-n // ROWS_PER_BLOCK)
            keep = torch.nonzero(radii > 0).flatten()
            for case, rd, nbytes in (("dense", None, n * (24 + width) + partials),
                                     ("sparse", radii, vis * (28 + width) + (n - vis) * 4 + partials)):
                us = timed(lambda: pose_gradient(vm, mu, dmu, radii=rd, **kw), a.rounds, a.iters,
                           a.warmup)
                extra = dict(visible_rows=vis) if rd is not None else {}
                report(n, form, case, "hip", us, nbytes=nbytes, launches=2, **extra)
                if a.no_torch:
                    continue
                if rd is None:
                    fn = lambda: torch_pose_grad(vm, mu, dmu, shape, dshape, form)
                else:
                    fn = lambda: torch_pose_grad(vm, mu[keep], dmu[keep], shape[keep], dshape[keep],
                                                 form)
                got, ref = pose_gradient(vm, mu, dmu, radii=rd, **kw), fn()
                tus = timed(fn, a.torch_rounds, a.torch_iters, 2)
                report(n, form, case, "torch_float64", tus,
                       torch_over_hip=round(tus["median"] / us["median"], 1),
                       max_rel_diff=float((got - ref).abs().max() / ref.abs().max()))
            del vm, mu, dmu, shape, dshape, radii, kw, keep
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
