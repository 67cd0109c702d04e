"""Density control (include/s3d.h, csrc/splat_density.hip) against a torch
composition of the same pass, same device, same tensors:

  * hip:   s3d_densify, three launches (classify + block counts, scan of the
           block counts, emit) into preallocated outputs, no host read;
           s3d_accumulate with ~10 % of the rows visible; s3d_reset_opacity;
  * torch: the decision as masks (sigmoid, exp, max, compares), then boolean
           indexing and `cat` on the rows and both moment arrays, `randn` for
           the split children's offsets through the rotation of the normalised
           quaternion.  It appends the new rows at the end, as INRIA 3DGS
           does, so it does not keep the input order the kernels keep; every
           boolean index reads its count back, which the kernels never do.

n = 8,388,608 and 393,216 rows; 5 % pruned, 5 % cloned, 5 % split.  Each
variant: `--warmup` untimed calls, then `--rounds` rounds of `--iters`
back-to-back calls between two device events; the median (min - max) per call
in microseconds.

Bytes, the model of the kernels (what a row moves, not a counter): the pass
reads 168 B of rows and moments and 12 B of statistics per input row and
writes 172 B (three rows and an origin entry) per output row; the code byte
written and read back and the rows the emit reads again are not counted.
s3d_accumulate moves 4 B per culled row and 36 B per visible one (radius,
dx, dy, three statistics in and out); s3d_reset_opacity reads 4 B and writes
up to 12 B per row, in 56-byte strides.  tb_per_s is bytes / time,
hbm_fraction_* that over the 8 TB/s peak and the 6.3 TB/s a streaming kernel
achieves on this chip.  At n = 393,216 the working set fits the 256 MiB
Infinity Cache, so that size is not an HBM measurement.  One JSON line per
(n, case, variant), on stdout and, with --log, appended to that file
(profiles/splat_density_bench.log is such a file).

python -m tools.bench_splat_density [--sizes 8388608 393216] [--rounds 10]
                                    [--log profiles/splat_density_bench.log]"""
from __future__ import annotations

import argparse
import ctypes
import math

import torch

from splatt3r_amd import _lib
from splatt3r_amd.refine import S3dParams, accumulate_stats, new_stats, reset_opacity
from tools import bench_splat_adam as base
from tools.bench_splat_adam import report, timed

PARAMS = dict(grad_threshold=2e-4, split_scale=0.01, min_opacity=0.005, max_scale=0.0,
              max_screen_radius=0, seed=1, pass_=0)


def inputs(n, device, seed=0):
    """Rows, moments and statistics with 5 % of the rows pruned (opacity),
    5 % cloned and 5 % split."""
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device=device)
    rows = torch.empty(n, 14, device=device)
    rows[:, 0:3] = torch.randn(n, 3, generator=g, device=device) * 3
    rows[:, 3:6] = torch.randn(n, 3, generator=g, device=device)
    rows[:, 6] = r(n) * 8 - 4
    rows[:, 7:10] = r(n, 3) * 5 - 7
    rows[:, 10:14] = torch.randn(n, 4, generator=g, device=device)
    u = r(n)
    rows[u < 0.05, 6] = -10.0
    clone, split = (u >= 0.05) & (u < 0.10), (u >= 0.10) & (u < 0.15)
    rows[clone, 7:10] = -7.5
    rows[split, 7] = -1.0
    ga, dn, mr = new_stats(n, device)
    ga[clone | split] = 1.0
    dn[clone | split] = 1
    m = torch.randn(n, 14, generator=g, device=device) * 1e-3
    v = r(n, 14) * 1e-6
    return rows, m, v, (ga, dn, mr)


def torch_pass(rows, m, v, stats, p):
    ga, dn, mr = stats
    o = torch.sigmoid(rows[:, 6])
    s = torch.exp(rows[:, 7:10])
    smax = s.max(1).values
    prune = ~torch.isfinite(rows).all(1) | (o < p["min_opacity"])
    avg = torch.where(dn > 0, ga / dn.clamp(min=1), torch.zeros_like(ga))
    grow = ~prune & (avg >= p["grad_threshold"])
    split = grow & (smax > p["split_scale"])
    clone = grow & ~split
    keep = ~prune & ~split
    par = rows[split]
    q = par[:, 10:14] / par[:, 10:14].norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
                    1).reshape(-1, 3, 3)
    kids = []
    for _ in range(2):
        c = par.clone()
        eps = torch.randn(par.shape[0], 3, device=rows.device)
        c[:, 0:3] += torch.bmm(R, (s[split] * eps)[:, :, None])[:, :, 0]
        c[:, 7:10] -= math.log(1.6)
        kids.append(c)
    new = torch.cat([rows[clone]] + kids)
    zeros = torch.zeros_like(new)
    return (torch.cat([rows[keep], new]), torch.cat([m[keep], zeros]),
            torch.cat([v[keep], zeros]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8388608, 393216])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-rounds", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    base.LOG = a.log
    if not torch.cuda.is_available():
        raise SystemExit("bench_splat_density needs a GPU")
    dev = torch.device("cuda", 0)
    hp = S3dParams(*[PARAMS[k] for k in ("grad_threshold", "split_scale", "min_opacity",
                                         "max_scale", "max_screen_radius", "seed", "pass_")])
    for n in a.sizes:
        rows, m, v, stats = inputs(n, dev)
        cap = 2 * n
        out = [torch.empty(cap, 14, device=dev) for _ in range(3)]
        origin = torch.empty(cap, device=dev, dtype=torch.int32)
        tally = torch.zeros(3, device=dev, dtype=torch.int64)
        need = int(_lib.lib().s3d_workspace_bytes(n))
        ws = torch.empty(need, device=dev, dtype=torch.uint8)

        def hip_pass():
            _lib.call("s3d_densify", rows.data_ptr(), m.data_ptr(), v.data_ptr(), n,
                      *[t.data_ptr() for t in stats], ctypes.byref(hp), cap,
                      *[t.data_ptr() for t in out], origin.data_ptr(), tally.data_ptr(),
                      tally.data_ptr() + 8, ws.data_ptr(), need, _lib.stream(dev))
        us = timed(hip_pass, a.rounds, a.iters, a.warmup)
        host = tally.cpu()
        n_out = int(host[0])
        counts = host[1:].view(torch.int32).tolist()
        hip = report(n, "densify", "hip", us, nbytes=n * 180 + n_out * 172, launches=3,
                     n_out=n_out, pruned=counts[0], cloned=counts[1], split=counts[2])

        d2 = torch.randn(n, 3, device=dev) * 1e-4
        radii = (torch.rand(n, device=dev) < 0.1).to(torch.int32) * 7
        vis = int((radii > 0).sum())
        acc = new_stats(n, dev)
        us = timed(lambda: accumulate_stats(d2, radii, acc), a.rounds, a.iters, a.warmup)
        report(n, "accumulate", "hip", us, nbytes=vis * 36 + (n - vis) * 4, launches=1,
               visible_rows=vis)
        r2, m2, v2 = rows.clone(), m.clone(), v.clone()
        us = timed(lambda: reset_opacity(r2, m2, v2, 0.01), a.rounds, a.iters, a.warmup)
        report(n, "reset_opacity", "hip", us, nbytes=n * 16, launches=1)
        del r2, m2, v2, d2, radii, acc, out, origin
        torch.cuda.empty_cache()
        if a.no_torch:
            continue
        p = dict(PARAMS)
        tout = torch_pass(rows, m, v, stats, p)
        assert tout[0].shape[0] == n_out, (tout[0].shape, n_out)
        del tout
        us = timed(lambda: torch_pass(rows, m, v, stats, p), a.torch_rounds, a.torch_iters, 2)
        report(n, "densify", "torch", us,
               torch_over_hip=round(us["median"] / hip["us"]["median"], 1))
        del rows, m, v, stats
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
