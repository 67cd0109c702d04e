"""Splat export (include/s3w.h s3w_map_to_splats, csrc/splat_io.hip) against
the torch route it replaces, same device, same inputs:

  * hip:   one launch, one Gaussian per thread (fixed-sweep Jacobi), rows
           staged through LDS;
  * torch: torch.linalg.eigh on the [n, 3, 3] batch, then the elementwise
           maps in torch ops (descending order, determinant fix, the
           four-branch rotation -> quaternion as torch.where, log / logit)
           and the concatenation into [n, 17].

n = 4,194,304 and 8,388,608 random covariances (scales exp(U(ln 1e-3,
ln 0.5)), random rotations; 453 MB and 906 MB of traffic, both past the
256 MiB Infinity Cache).  Each variant: `--warmup` untimed calls, then
`--rounds` rounds of `--iters` back-to-back calls between two device events;
the median (min - max) per call in microseconds.  The torch route gets
`--torch-rounds` rounds of one call (it is orders of magnitude longer), after
a probe call on n / 16 Gaussians: if 16 x the probe says the full size would
exceed `--torch-budget-s`, the probe's time is reported and the size skipped.
Bytes moved by the export: 40 B read + 68 B written per Gaussian; hbm_fraction
is bytes / time over the 8 TB/s peak and over the 6.3 TB/s a streaming kernel
achieves on this chip.  One JSON line per (n, variant), printed as soon as it
is measured; the hip lines come first.  log_scale_err_vs_float64 is each
route's largest |scale_i - log sqrt(max(lambda_i, scale_min^2))| per column
against numpy float64 eigvalsh on the host, over the first 65,536 Gaussians
(the quaternions are not compared: eigenvectors of close eigenvalues, and
their signs, differ legitimately).

python -m tools.bench_splat_export [--sizes 4194304 8388608] [--rounds 10]"""
from __future__ import annotations

import argparse
import json
import statistics

import torch

from splatt3r_amd import _lib

C0 = 0.28209479177387814
HBM_PEAK = 8.0e12
HBM_ACHIEVABLE = 6.3e12
BYTES_PER_GAUSSIAN = 40 + 68


def inputs(n, device, seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device=device)
    s = torch.exp(r(n, 3) * (torch.log(torch.tensor(0.5)) - torch.log(torch.tensor(1e-3))).item()
                  + torch.log(torch.tensor(1e-3)).item())
    q = torch.randn(n, 4, generator=g, device=device)
    R = quat_to_R(q / q.norm(dim=1, keepdim=True))
    S = (R * (s * s)[:, None, :]) @ R.transpose(1, 2)
    cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
    return (torch.randn(n, 3, generator=g, device=device).contiguous(), cov.contiguous(),
            r(n, 3).contiguous(), (0.05 + 0.95 * r(n)).contiguous())


def quat_to_R(q):
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
                       1).reshape(-1, 3, 3)


def hip_export(means, cov, colors, op, rows, scale_min=1e-7):
    _lib.call("s3w_map_to_splats", means.data_ptr(), cov.data_ptr(), colors.data_ptr(),
              op.data_ptr(), None, means.shape[0], scale_min, rows.data_ptr(),
              _lib.stream(means.device))
    return rows


@torch.no_grad()
def torch_export(means, cov, colors, op, scale_min=1e-7):
    n = means.shape[0]
    S = cov[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(n, 3, 3)
    lam, V = torch.linalg.eigh(S)
    lam, V = lam.flip(1), V.flip(2)
    V = torch.cat([V[:, :, :2], V[:, :, 2:] * torch.linalg.det(V).sign()[:, None, None]], 2)
    scale = torch.log(lam.clamp_min(0).sqrt().clamp_min(scale_min))
    m = lambda i, j: V[:, i, j]
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    four = torch.stack([tr, m(0, 0), m(1, 1), m(2, 2)], 1)
    k = four.argmax(1)
    # 1 + tr for the trace branch, 1 + Rkk - (the other two) = 1 + 2 Rkk - tr else
    largest = four.gather(1, k[:, None])[:, 0]
    s = 2 * torch.sqrt(torch.where(k == 0, 1 + tr, 1 + 2 * largest - tr).clamp_min(0))
    a, b, c = (m(2, 1) - m(1, 2)) / s, (m(0, 2) - m(2, 0)) / s, (m(1, 0) - m(0, 1)) / s
    d, e, f = (m(0, 1) + m(1, 0)) / s, (m(0, 2) + m(2, 0)) / s, (m(1, 2) + m(2, 1)) / s
    quarter = s / 4
    q = torch.stack([
        torch.where(k == 0, quarter, torch.where(k == 1, a, torch.where(k == 2, b, c))),
        torch.where(k == 0, a, torch.where(k == 1, quarter, torch.where(k == 2, d, e))),
        torch.where(k == 0, b, torch.where(k == 1, d, torch.where(k == 2, quarter, f))),
        torch.where(k == 0, c, torch.where(k == 1, e, torch.where(k == 2, f, quarter)))], 1)
    q = q / q.norm(dim=1, keepdim=True)
    q = torch.where(q[:, :1] < 0, -q, q)
    o = op.clamp(1e-6, 1 - 1e-6)
    return torch.cat([means, torch.zeros_like(means), (colors - 0.5) / C0,
                      torch.log(o / (1 - o))[:, None], scale, q], 1)


def log_scale_err(cov, rows, scale_min=1e-7, k=65536):
    """Largest |scale - float64 reference| per scale column over the first k."""
    import numpy as np
    c = cov[:k].double().cpu().numpy()
    S = c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    lam = np.linalg.eigvalsh(S)[:, ::-1]
    ref = 0.5 * np.log(np.maximum(lam, scale_min ** 2))
    got = rows[:k, 10:13].double().cpu().numpy()
    return [float(f"{v:.3g}") for v in np.abs(got - ref).max(0)]


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


def report(n, variant, us, **extra):
    nbytes = n * BYTES_PER_GAUSSIAN
    sec = us["median"] * 1e-6
    out = {"n": n, "variant": variant, "us": us, "bytes": nbytes,
           "tb_per_s": round(nbytes / sec / 1e12, 3),
           "hbm_fraction_of_peak": round(nbytes / sec / HBM_PEAK, 3),
           "hbm_fraction_of_achievable": round(nbytes / sec / HBM_ACHIEVABLE, 3),
           "gaussians_per_s": round(n / sec / 1e9, 2)}
    out.update(extra)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4194304, 8388608])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--torch-budget-s", type=float, default=120.0)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_splat_export needs a GPU")
    dev = torch.device("cuda", 0)
    data, hip_us = {}, {}
    for n in a.sizes:                       # every hip line before any torch line
        data[n] = inputs(n, dev)
        rows = torch.empty(n, 17, device=dev)
        hip_us[n] = timed(lambda: hip_export(*data[n], rows), a.rounds, a.iters, a.warmup)
        report(n, "hip", hip_us[n], launches=1,
               log_scale_err_vs_float64=log_scale_err(data[n][1], rows))
        del rows
    if a.no_torch:
        return
    for n in a.sizes:
        # one call on the first n / 16 Gaussians first: if 16 x its time says
        # the full size would not fit the budget, report the probe instead
        probe = tuple(t[:n // 16] for t in data[n])
        try:
            p_us = timed(lambda: torch_export(*probe), 1, 1, 1)["median"]
            if p_us * 16 * (a.torch_rounds + 1) * 1e-6 > a.torch_budget_s:
                print(json.dumps({"n": n, "variant": "torch", "skipped": "over the time budget",
                                  "probe_n": n // 16, "probe_us": p_us}), flush=True)
                continue
            us = timed(lambda: torch_export(*data[n]), a.torch_rounds, 1, 1)
        except RuntimeError as e:           # e.g. out of memory in the batched solver
            print(json.dumps({"n": n, "variant": "torch", "error": str(e).split("\n")[0]}),
                  flush=True)
            continue
        t = torch_export(*data[n])
        report(n, "torch", us, log_scale_err_vs_float64=log_scale_err(data[n][1], t),
               torch_over_hip=round(us["median"] / hip_us[n]["median"], 1))
        del t


if __name__ == "__main__":
    main()
