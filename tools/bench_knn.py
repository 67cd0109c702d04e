"""Exact k nearest neighbours on the grid (include/s3k.h s3k_knn,
csrc/nn_search.hip k_nn_knn) and the map's floater removal, against a torch
composition on the same device and inputs:

  * hip_knn:  PointGrid.knn of n uniform points of the unit cube on
              themselves (exclude_self) at k = 3, 8, 16, the grid built once
              outside the timed region at the default cell
              2 (volume / n)^(1/3) and at twice it (neither tuned).  Two forms:
              `table` writes idx and dist [n, k], `mean` only the fused row
              mean [n] (what outlier_mask and knn_scale ask for).
  * torch_cdist_topk:  torch.cdist of a chunk of queries against every row,
              then topk(k + 1, largest=False) (the + 1 is the point itself),
              chunk by chunk, each chunk's matrix at most 1 GiB.  Above
              `--torch-full-below` rows it runs on the first `scaled_from`
              queries and the time is multiplied up: such a line is an
              extrapolation and carries `scaled_from`.  cdist is float32:
              `same_rows` is the share of queries whose k indices are the
              exact search's.
  * hip_outlier_mask, hip_remove_outliers:  an 8,388,608-row map
              (bench_map_compact's synthetic surface, the last 1 % of the rows
              lifted off it along z by 5 to 30 cm, either way), k = 16,
              std_ratio = 2.  outlier_mask is the grid build, the search and
              the threshold; remove_outliers adds the two host reads and the
              move of the five fields, the map restored before every call
              outside the timed region.
  * hip_query (`--k1`):  PointGrid.query, the k = 1 path this work leaves
              alone.  Run once per library: the parent commit's library built
              as libsplatt3r_hip_parent.so beside the shipped one and chosen
              with S3_LIB_VARIANT=_parent, the two alternated process by
              process (`lib` names which one a line is).

hip_knn and torch lines: `--warmup` untimed calls, then `--rounds` rounds of
`--iters` back-to-back calls between two device events.  The map lines: a host
clock around one call between two device synchronises (the call reads back),
`--rounds` of them.  Median (min - max) per call in microseconds.

One JSON line per measurement, on stdout and, with --log, appended to that
file as well (profiles/knn_bench.log is such a file).

python -m tools.bench_knn [--sizes 200000 2000000] [--map-rows 8388608]
                          [--k1] [--log profiles/knn_bench.log]"""
from __future__ import annotations

import argparse
import os
import statistics
import time

import torch

from splatt3r_amd import nn
from tools import bench_map_compact as base
from tools.bench_map_compact import FOOTPRINT, report, synthetic_map, timed

KS = (3, 8, 16)
CELLS = (("default", 1.0), ("twice", 2.0))
CHUNK_BYTES = 1 << 30
LIB = os.environ.get("S3_LIB_VARIANT") or "this_tree"


def torch_knn(q, ref, k):
    """Chunked cdist + topk: idx [m, k] int64 of the k + 1 nearest without the
    first column (the point itself: q is the head of ref)."""
    step = max(1, CHUNK_BYTES // (4 * max(ref.shape[0], 1)))
    out = []
    for a in range(0, q.shape[0], step):
        out.append(torch.cdist(q[a:a + step], ref).topk(k + 1, dim=1, largest=False).indices[:, 1:])
    return torch.cat(out)


def host_timed(fn, before, rounds):
    t = []
    for _ in range(rounds + 1):              # the first call is the warm-up
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    t = t[1:]
    return {"median": round(statistics.median(t), 1), "min": round(min(t), 1),
            "max": round(max(t), 1)}


def bench_self_queries(a, dev):
    for n in a.sizes:
        g = torch.Generator(device=dev).manual_seed(n)
        pts = torch.rand(n, 3, generator=g, device=dev).contiguous()
        _, cell0, _ = nn.default_grid(pts)
        exact = {}
        for name, factor in CELLS:
            origin, cell, dims = nn.default_grid(pts, cell=cell0 * factor)
            grid = nn.PointGrid(pts, origin=origin, cell=cell, dims=dims)
            for k in KS:
                full = grid.knn(pts, k, exclude_self=True, want=nn.KNN_OUTPUTS)
                if k not in exact:
                    exact[k] = full
                same = all(torch.equal(full[o].view(torch.int32), exact[k][o].view(torch.int32))
                           for o in nn.KNN_OUTPUTS)
                common = dict(n=n, k=k, cell=name, cell_m=cell, dims=list(dims), lib=LIB)
                us = timed(lambda: grid.knn(pts, k, exclude_self=True), a.rounds, a.iters, a.warmup)
                report(variant="hip_knn", form="table", us=us,
                       rows_per_s=round(n / (us["median"] * 1e-6)), same_as_default_cell=same,
                       **common)
                us = timed(lambda: grid.knn(pts, k, exclude_self=True, want=("mean",)), a.rounds,
                           a.iters, a.warmup)
                report(variant="hip_knn", form="mean", us=us,
                       rows_per_s=round(n / (us["median"] * 1e-6)), **common)
            del grid
        if not a.no_torch:
            m = n if n < a.torch_full_below else max(1, a.torch_pairs // n)
            for k in KS:
                t_idx = torch_knn(pts[:m], pts, k)
                agree = float((t_idx == exact[k]["idx"][:m].long()).all(1).float().mean())
                tus = timed(lambda: torch_knn(pts[:m], pts, k), a.torch_rounds, 1, 1)
                if m < n:
                    tus = {key: round(v * n / m, 1) for key, v in tus.items()}
                report(n=n, k=k, variant="torch_cdist_topk", us=tus, same_rows=round(agree, 6),
                       scaled_from=m if m < n else None)
        del pts, exact
        torch.cuda.empty_cache()


def bench_map(a, dev):
    from splatt3r_amd.gaussian_map import SharedGaussians
    n, k = a.map_rows, 16
    fields = synthetic_map(n, dev)
    means = fields[0].clone()
    f = n // 100
    g = torch.Generator(device=dev).manual_seed(7)
    off = 0.05 + 0.25 * torch.rand(f, generator=g, device=dev)
    means[n - f:, 2] += torch.where(torch.rand(f, generator=g, device=dev) < 0.5, -off, off)
    gm = SharedGaussians(max_gaussians=n, device=dev)
    saved = (means,) + tuple(fields[1:5])

    def restore():
        for dst, src in zip((gm.means, gm.cov_triu, gm.colors, gm.opacities, gm.kf_id), saved):
            dst.copy_(src)
        gm._n.fill_(n)
    restore()
    removed = gm.remove_outliers(k=k)
    spread = int((~nn.outlier_mask(means, k=k))[n - f:].sum())
    common = dict(n=n, k=k, std_ratio=2.0, lib=LIB)
    us = host_timed(lambda: nn.outlier_mask(means, k=k), lambda: None, a.rounds)
    report(variant="hip_outlier_mask", us=us, **common)
    us = host_timed(lambda: gm.remove_outliers(k=k), restore, a.rounds)
    report(variant="hip_remove_outliers", us=us, removed=removed, lifted_rows=f,
           lifted_rows_removed=spread, **common)
    if not a.no_torch:
        m = max(1, a.torch_pairs // n)
        tus = timed(lambda: torch_knn(means[:m], means, k), a.torch_rounds, 1, 1)
        tus = {key: round(v * n / m, 1) for key, v in tus.items()}
        report(n=n, k=k, variant="torch_cdist_topk", us=tus, scaled_from=m,
               note="the search alone, without the threshold and the move")


def bind_what_the_library_has():
    """An older library lacks the entry points added since: load the variant
    S3_LIB_VARIANT names and bind the declarations it exports."""
    import ctypes
    from splatt3r_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    _lib._bind(lib, {name: sig for name, sig in _lib.SIGNATURES.items() if hasattr(lib, name)})
    _lib._lib = lib


def bench_k1(a, dev):
    if os.environ.get("S3_LIB_VARIANT"):
        bind_what_the_library_has()
    for n in a.sizes:
        ref = synthetic_map(n, dev)[0]
        g = torch.Generator(device=dev).manual_seed(1)
        q = (ref + torch.randn(n, 3, generator=g, device=dev) * FOOTPRINT).contiguous()
        grid = nn.PointGrid(ref)
        idx, dist = grid.query(q)
        us = timed(lambda: grid.query(q), a.rounds, a.iters, a.warmup)
        report(variant="hip_query", n=n, lib=LIB, us=us, idx_sum=int(idx.long().sum()),
               dist_sum=float(dist.double().sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200000, 2000000])
    ap.add_argument("--map-rows", type=int, default=8388608)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--torch-full-below", type=int, default=500000,
                    help="from this many rows on the torch composition runs on a slice")
    ap.add_argument("--torch-pairs", type=int, default=40_000_000_000,
                    help="query-row pairs of a sliced torch run")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-map", action="store_true")
    ap.add_argument("--k1", action="store_true", help="only PointGrid.query (see the head)")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    base.LOG = a.log
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn needs a GPU")
    dev = torch.device("cuda", 0)
    if a.k1:
        bench_k1(a, dev)
        return
    bench_self_queries(a, dev)
    if not a.no_map:
        bench_map(a, dev)


if __name__ == "__main__":
    main()
