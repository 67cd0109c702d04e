"""Map compaction (include/s3v.h, csrc/map_compact.hip) against a torch
composition of the same definition, same device, same inputs:

  * hip:   merge_gaussians: voxel keys packed to the occupied cell range, a
           stable radix sort in as many 8-bit passes as those need, two scans,
           the chunked double sums; no host read;
  * torch: the definition as torch ops: float64 keys, torch.unique(...,
           return_inverse=True) for the groups, float64 index_add_ for every
           sum, scatter_reduce(amin) for `first`, argsort for the output order.

The input is a synthetic map of overlapping keyframes: 512 x 384 pixel-aligned
Gaussians per keyframe (196,608) on an undulating surface about 2 m in front
of cameras that step 5 cm sideways, fx = fy = 400 px, so one pixel's footprint
on the surface is about 5 mm and neighbouring keyframes see mostly the same
surface.  n = 393,216 (two keyframes) and 8,388,608 (42.7).  Two voxel sizes,
both untuned: 5 mm (about one pixel footprint) and 20 mm (about four).

Each variant: `--warmup` untimed calls, then `--rounds` rounds of `--iters`
back-to-back calls between two device events; the median (min - max) per call
in microseconds.

Bytes per call, the model of the pass (what a row moves, not a counter), for n
rows in m groups sorted in P passes: keys 52 B read + 8 B written; packing 8 B
read + 12 B written; a sort pass 8 B (histogram) + 12 B read + 12 B written;
heads 12 B read + 8 B written; scans 16 B read + 8 B written; sums 16 B of
indices, 52 B of fields gathered, 8 B of `group` written: 200 + 32 P bytes per
row, and 68 B per group (the merged row, `first`, the kf_id gather).  P is
reported as sort_passes (ceil(bits / 8), bits the sum over the axes of the
bits of the occupied cell range).  tb_per_s is bytes
/ time, hbm_fraction_* that over the 8 TB/s peak and the 6.3 TB/s a streaming
kernel achieves on this chip.  At n = 393,216 the working set fits the 256 MiB
Infinity Cache, so that size is not an HBM measurement.

With --render (default on) the compacted map is also rendered (render_map,
512 x 384, from the middle keyframe's camera) and compared with the render of
the uncompacted map: image_metrics' PSNR and SSIM, reported, not asserted.

One JSON line per measurement, on stdout and, with --log, appended to that
file as well (profiles/map_compact_bench.log is such a file).

python -m tools.bench_map_compact [--sizes 393216 8388608] [--rounds 10]
                                  [--log profiles/map_compact_bench.log]"""
from __future__ import annotations

import argparse
import json
import math
import statistics

import numpy as np
import torch

from splatt3r_amd.compact import merge_gaussians

HBM_PEAK = 8.0e12
HBM_ACHIEVABLE = 6.3e12
LOG = None
KF_W, KF_H, FOCAL, DEPTH, STEP = 512, 384, 400.0, 2.0, 0.05
FOOTPRINT = DEPTH / FOCAL                    # 5 mm
VOXELS = (("1_footprint", FOOTPRINT), ("4_footprints", 4 * FOOTPRINT))
BIAS, TOP = float(1 << 20), float((1 << 21) - 1)


def synthetic_map(n, device, seed=0):
    """n Gaussians, keyframe after keyframe (row r: keyframe r // 196,608,
    pixel r % 196,608), kf_id non-decreasing."""
    g = torch.Generator(device=device).manual_seed(seed)
    r = torch.arange(n, device=device)
    per = KF_W * KF_H
    kf, pix = r // per, r % per
    u = (pix % KF_W).float() + 0.5 + (torch.rand(n, generator=g, device=device) - 0.5) * 0.4
    v = (pix // KF_W).float() + 0.5 + (torch.rand(n, generator=g, device=device) - 0.5) * 0.4
    cx = kf.float() * STEP
    # depth of the surface along the pixel's ray, one fixed-point step
    x0 = cx + (u - KF_W / 2) / FOCAL * DEPTH
    y0 = (v - KF_H / 2) / FOCAL * DEPTH
    z = DEPTH + 0.15 * torch.sin(1.7 * x0) * torch.cos(2.3 * y0)
    z = z + torch.randn(n, generator=g, device=device) * 0.2 * FOOTPRINT
    means = torch.stack([cx + (u - KF_W / 2) / FOCAL * z, (v - KF_H / 2) / FOCAL * z, z], 1)
    s2, t2 = (0.6 * FOOTPRINT) ** 2, (0.2 * FOOTPRINT) ** 2
    cov = torch.zeros(n, 6, device=device)
    cov[:, 0], cov[:, 3], cov[:, 5] = s2, s2, t2
    x, y = means[:, 0], means[:, 1]
    colors = torch.stack([0.5 + 0.5 * torch.sin(9.0 * x), 0.5 + 0.5 * torch.sin(7.0 * y + 1.0),
                          0.5 + 0.5 * torch.sin(5.0 * (x + y))], 1)
    opac = 0.6 + 0.35 * torch.rand(n, generator=g, device=device)
    return (means.contiguous(), cov, colors.contiguous(), opac, kf.to(torch.int32))


def torch_merge(means, cov, colors, opac, kf_id, voxel, origin=(0.0, 0.0, 0.0)):
    """The definition of include/s3v.h in torch ops, float64 sums."""
    dev = means.device
    ok = (torch.isfinite(means).all(1) & torch.isfinite(cov).all(1)
          & torch.isfinite(colors).all(1) & torch.isfinite(opac))
    kept = torch.nonzero(ok).flatten()
    x, S, c, o = (t[kept].double() for t in (means, cov, colors, opac))
    cell = torch.floor((x - torch.tensor(origin, device=dev, dtype=torch.float64)) / voxel) + BIAS
    cell = cell.clamp(0.0, TOP).long()
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    uniq, inv = torch.unique(key, return_inverse=True)
    G = uniq.numel()
    add = lambda v: torch.zeros((G, *v.shape[1:]), device=dev, dtype=torch.float64) \
        .index_add_(0, inv, v)
    w = torch.where(add(o)[inv] == 0.0, torch.ones_like(o), o)
    W = add(w)
    mean = add(w[:, None] * x) / W[:, None]
    d = x - mean[inv]
    dd = torch.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2],
                      d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
    sigma = add(w[:, None] * (S + dd)) / W[:, None]
    colour = add(w[:, None] * c) / W[:, None]
    opacity = add(w * o) / W
    first = torch.full((G,), means.shape[0], device=dev, dtype=torch.int64) \
        .scatter_reduce_(0, inv, kept, "amin")
    first, order = torch.sort(first)
    row_of = torch.empty(G, device=dev, dtype=torch.int64)
    row_of[order] = torch.arange(G, device=dev)
    group = torch.full((means.shape[0],), -1, device=dev, dtype=torch.int64)
    group[kept] = row_of[inv]
    return (mean[order].float(), sigma[order].float(), colour[order].float(),
            opacity[order].float(), kf_id[first], first, group)


def sort_passes(means, voxel):
    """The 8-bit passes the packed keys of `means` take (origin 0, no dropped row)."""
    cell = torch.floor(means.double() / voxel).long()
    span = (cell.amax(0) - cell.amin(0)).tolist()
    return -(-sum(int(v).bit_length() for v in span) // 8)


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


def report(**out):
    us, nbytes = out.get("us"), out.get("bytes")
    if nbytes is not None:
        sec = us["median"] * 1e-6
        out.update(tb_per_s=round(nbytes / sec / 1e12, 3),
                   hbm_fraction_of_peak=round(nbytes / sec / HBM_PEAK, 3),
                   hbm_fraction_of_achievable=round(nbytes / sec / HBM_ACHIEVABLE, 3))
    line = json.dumps(out)
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")
    return out


def render_of(fields, m, n_kf):
    """render_map of the first m rows of `fields` from the middle keyframe."""
    from splatt3r_amd.gaussian_map import SharedGaussians, render_map
    gm = SharedGaussians(max_gaussians=m, device=fields[0].device)
    for dst, src in zip((gm.means, gm.cov_triu, gm.colors, gm.opacities, gm.kf_id), fields):
        dst.copy_(src[:m])
    gm._n.fill_(m)
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = (n_kf // 2) * STEP
    vfov = math.degrees(2.0 * math.atan(KF_H / 2 / FOCAL))
    return render_map(gm, T, KF_W, KF_H, vfov, bg=(0.0, 0.0, 0.0), n=m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[393216, 8388608])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-iters", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    global LOG
    LOG = a.log
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_compact needs a GPU")
    from splatt3r_amd.photometric import image_metrics
    dev = torch.device("cuda", 0)
    for n in a.sizes:
        fields = synthetic_map(n, dev)
        n_kf = -(-n // (KF_W * KF_H))
        full = None if a.no_render else render_of(fields, n, n_kf)
        for name, voxel in VOXELS:
            out = merge_gaussians(*fields, voxel)
            m = int(out[7])
            us = timed(lambda: merge_gaussians(*fields, voxel), a.rounds, a.iters, a.warmup)
            P = sort_passes(fields[0], voxel)
            report(n=n, voxel=name, voxel_m=voxel, variant="hip", us=us, m=m,
                   count_ratio=round(m / n, 4), sort_passes=P,
                   bytes=(200 + 32 * P) * n + 68 * m)
            if not a.no_torch:
                ref = torch_merge(*fields, voxel)
                same = ref[0].shape[0] == m and bool(torch.equal(ref[5], out[5][:m])) \
                    and bool(torch.equal(ref[6], out[6]))
                diff = max(float((r - o[:m]).abs().max()) for r, o in zip(ref[:4], out[:4])) \
                    if same else float("nan")
                tus = timed(lambda: torch_merge(*fields, voxel), a.rounds, a.torch_iters, 1)
                report(n=n, voxel=name, voxel_m=voxel, variant="torch_float64", us=tus,
                       torch_over_hip=round(tus["median"] / us["median"], 2),
                       same_groups=same, max_abs_diff=diff)
                del ref
            if full is not None:
                img = render_of(out[:5], m, n_kf)
                q = image_metrics(img[None].contiguous(), full[None].contiguous())
                report(n=n, voxel=name, voxel_m=voxel, variant="render_vs_uncompacted", m=m,
                       count_ratio=round(m / n, 4), psnr=round(float(q["psnr"][0]), 2),
                       ssim=round(float(q["ssim"][0]), 4))
                del img
            del out
            torch.cuda.empty_cache()
        del fields, full
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
