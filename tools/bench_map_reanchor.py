"""Map re-anchor (include/s3a.h, csrc/map_reanchor.hip) against a torch
composition of the same definition, same device, same inputs:

  * hip:        s3a_map_reanchor, direct per-lane accesses (the shipped path):
                the per-keyframe deltas, then one thread per Gaussian that
                reads kf_id and its keyframe's flag and stops there unless
                the row moves;
  * hip_staged: the same with s3a_set_path(1): a workgroup with something to
                move stages its 256 rows through LDS as float4 runs;
  * torch:      float64 deltas per keyframe, gathered by kf_id, two bmm for
                the covariance and one for the mean, written back with a
                masked store (torch.where over every row).

The map: n rows labelled in 240 equal runs (row r: keyframe r * 240 // n), as
a map appended keyframe after keyframe is.  Poses: random rotations, |t| <= 1,
s = 1 (the values stay bounded however often the same delta is applied; the
time does not depend on them).  Cases: every keyframe moved; 24 of 240 (10 %)
moved, as three contiguous runs of 8 keyframes; none moved.

Each variant: `--warmup` untimed calls, then `--rounds` rounds of `--iters`
back-to-back calls between two device events; the median (min - max) per call
in microseconds.  Every call works from the same anchor table: a round's
`--iters` calls each take their own copy of it, and the copies are restored
before the round, outside the timed region.

Bytes per call, the model (what a row moves, not a counter): 76 B per moved
row (4 B label + 36 B read, 36 B written), 4 B per unmoved row.  tb_per_s is
bytes / time, hbm_fraction_* that over the 8 TB/s peak and the 6.3 TB/s a
streaming kernel achieves on this chip.  At n = 393,216 the working set fits
the 256 MiB Infinity Cache, so that size is not an HBM measurement.

One JSON line per measurement, on stdout and, with --log, appended to that
file as well (profiles/map_reanchor_bench.log is such a file).

python -m tools.bench_map_reanchor [--sizes 393216 8388608] [--rounds 10]
                                   [--cases all 10_percent none]
                                   [--log profiles/map_reanchor_bench.log]"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics

import torch

from splatt3r_amd import _lib
from splatt3r_amd.gaussian_map import SharedGaussians

HBM_PEAK = 8.0e12
HBM_ACHIEVABLE = 6.3e12
LOG = None
N_KF = 240
MOVED_RUNS = ((20, 28), (100, 108), (200, 208))     # 24 keyframes, 10 %


def random_poses(n, g, device):
    q = torch.randn(n, 4, generator=g, device=device)
    q = q / q.norm(dim=1, keepdim=True)
    t = torch.rand(n, 3, generator=g, device=device) * 2 - 1
    t = t / t.norm(dim=1, keepdim=True).clamp_min(1.0)
    return torch.cat([t, q, torch.ones(n, 1, device=device)], 1).contiguous()


def synthetic_map(n, device, seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    gm = SharedGaussians(max_gaussians=n, device=device, max_keyframes=N_KF)
    gm.means.copy_(torch.randn(n, 3, generator=g, device=device) * 3)
    a = torch.randn(n, 3, 3, generator=g, device=device) * 0.05
    S = a @ a.transpose(1, 2)
    gm.cov_triu.copy_(torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2],
                                   S[:, 2, 2]], 1))
    del a, S
    gm.colors.uniform_(generator=g)
    gm.opacities.uniform_(generator=g)
    gm.kf_id.copy_((torch.arange(n, device=device) * N_KF // n).to(torch.int32))
    gm._n.fill_(n)
    return gm


def cases(anchor, g):
    moved = random_poses(N_KF, g, anchor.device)
    some = anchor.clone()
    for a, b in MOVED_RUNS:
        some[a:b] = moved[a:b]
    return (("all", moved), ("10_percent", some), ("none", anchor.clone()))


def quat_R(q):
    q = q / q.norm(dim=1, keepdim=True)
    x, y, z, w = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
                       1).reshape(-1, 3, 3)


def torch_reanchor(gm, n, anchor, poses):
    """The definition in torch ops (valid, set poses only): float64 deltas
    gathered by kf_id, bmm, a masked store.  Returns the new fields; the map
    is not written."""
    a, p = anchor.double(), poses.double()
    M = (p[:, 7] / a[:, 7])[:, None, None] * (quat_R(p[:, 3:7]) @ quat_R(a[:, 3:7]).transpose(1, 2))
    flag = (anchor.view(torch.int32) != poses.view(torch.int32)).any(1)
    kf = gm.kf_id[:n].long()
    ok = (kf >= 0) & (kf < N_KF)
    k = kf.clamp(0, N_KF - 1)
    mv = ok & flag[k]
    Mi = M[k]
    mu = p[k, :3] + torch.bmm(Mi, (gm.means[:n].double() - a[k, :3])[:, :, None])[:, :, 0]
    c = gm.cov_triu[:n].double()
    Sig = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4],
                       c[:, 5]], 1).reshape(-1, 3, 3)
    out = torch.bmm(torch.bmm(Mi, Sig), Mi.transpose(1, 2)).reshape(-1, 9)
    cov = out[:, [0, 1, 2, 4, 5, 8]]
    return (torch.where(mv[:, None], mu.float(), gm.means[:n]),
            torch.where(mv[:, None], cov.float(), gm.cov_triu[:n]), mv)


def timed(fn, rounds, iters, warmup, before_round=None):
    if before_round:
        before_round()
    for j in range(warmup):
        fn(j)
    torch.cuda.synchronize()
    t = []
    for _ in range(rounds):
        if before_round:
            before_round()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for j in range(iters):
            fn(j)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[393216, 8388608])
    ap.add_argument("--cases", nargs="+", default=["all", "10_percent", "none"])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    global LOG
    LOG = a.log
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_reanchor needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    slots = max(a.iters, a.warmup)
    for n in a.sizes:
        gm = synthetic_map(n, dev)
        g = torch.Generator(device=dev).manual_seed(1)
        anchor = random_poses(N_KF, g, dev)
        ws = torch.empty(int(lib.s3a_reanchor_workspace_bytes(N_KF)) // 8, dtype=torch.float64,
                         device=dev)
        tables = torch.empty(slots, N_KF, 8, device=dev)
        for name, poses in cases(anchor, g):
            if name not in a.cases:
                continue
            gm.anchors[:N_KF] = anchor
            moved, held = gm.reanchor(poses, count=True)
            assert held == 0
            nbytes = 76 * moved + 4 * (n - moved)

            def call(j):
                _lib.call("s3a_map_reanchor", ctypes.byref(gm._c), tables[j].data_ptr(),
                          poses.data_ptr(), N_KF, None, None, ws.data_ptr(), ws.numel() * 8,
                          _lib.stream(dev))

            restore = lambda: tables.copy_(anchor[None].expand_as(tables))
            us = {}
            for variant, path in (("hip", 0), ("hip_staged", 1)):
                lib.s3a_set_path(path)
                try:
                    us[variant] = timed(call, a.rounds, a.iters, a.warmup, restore)
                finally:
                    lib.s3a_set_path(0)
                report(n=n, case=name, variant=variant, us=us[variant], moved=moved,
                       bytes=nbytes)
            if not a.no_torch:
                gm.anchors[:N_KF] = anchor
                before = (gm.means.clone(), gm.cov_triu.clone())
                tm, tc, mv = torch_reanchor(gm, n, anchor, poses)
                gm.reanchor(poses)
                diff = max(float((tm - gm.means).abs().max()), float((tc - gm.cov_triu).abs().max()))
                same = int(mv.sum()) == moved
                gm.means.copy_(before[0])
                gm.cov_triu.copy_(before[1])
                del tm, tc, mv, before
                tus = timed(lambda j: torch_reanchor(gm, n, anchor, poses), a.rounds,
                            a.torch_iters, 1)
                report(n=n, case=name, variant="torch_float64", us=tus,
                       torch_over_hip=round(tus["median"] / us["hip"]["median"], 2),
                       same_rows=same, max_abs_diff=diff)
            torch.cuda.empty_cache()
        del gm, tables, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
