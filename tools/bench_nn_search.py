"""Grid nearest neighbour and mesh sampling (include/s3k.h, csrc/nn_search.hip)
against a torch composition on the same device, same inputs:

  * hip:   PointGrid (build) and PointGrid.query, timed separately, at the
           default cell 2 (volume / n)^(1/3), half of it and twice it (none of
           them tuned); the grid's origin and dims are computed once outside
           the timed region, so a timed build reads nothing back;
  * torch: torch.cdist of a chunk of queries against every reference row, then
           min over the row, chunk by chunk (each chunk's matrix at most
           1 GiB).  At 2,000,000 rows it runs on the first tenth of the queries
           and the time is multiplied by ten (`scaled_from` says so).  cdist is
           float32: `same_index` is the share of queries for which it names
           the same row as the exact search.

The input is bench_map_compact's synthetic surface (pixel-aligned points, one
pixel's footprint, 5 mm, apart) as the reference and a copy displaced by a
normal step of one footprint per axis as the queries; n = m = 200,000 and
2,000,000.  Sampling: a 1,501 x 1,501 vertex grid over the same kind of surface,
4,500,000 triangles, 200,000 samples (the call includes its one host read of
the two counters).

Each variant: `--warmup` untimed calls, then `--rounds` rounds of `--iters`
back-to-back calls between two device events; the median (min - max) per call
in microseconds.

Bytes per query, the model of the pass (what a query moves, not a counter):
keys 12 B read + 8 B written; a sort pass 4 B (histogram) + 8 B read + 8 B
written, P passes for the bits of the cell count; the search 4 B of order,
12 B of the query gathered, 8 B written back, 8 B of `start` per run of cells
and 16 B per record looked at.  For a query that ends after ring 1 that is
9 runs and the R records of its 27 cells: 28 + 20 P + 72 + 16 R bytes, R
measured here as the mean over the queries of the rows in those 27 cells
(`rows_27`).  Neighbouring lanes hold queries of the same cell and read the
same records, so the model overstates what reaches HBM.  Build, per row: 12 B
read + 4 B cell id + an atomic, then 4 + 12 B read, an atomic and 16 B
written; per cell 4 B cleared, read twice, written twice.

One JSON line per measurement, on stdout and, with --log, appended to that
file as well (profiles/nn_search_bench.log is such a file).

`hip_query_ab` lines: the same query call with nn.set_query_mode "unsorted"
(no sort, the queries' own order) and "wave" (sorted, one wave per query, the
lanes sharing each run of records), on the queries as given and on a random
permutation of them; `same_bits` says the result did not change.

python -m tools.bench_nn_search [--sizes 200000 2000000] [--rounds 10]
                                [--log profiles/nn_search_bench.log]"""
from __future__ import annotations

import argparse

import torch

from splatt3r_amd.nn import PointGrid, default_grid, sample_mesh, set_query_mode
from tools import bench_map_compact as base
from tools.bench_map_compact import FOOTPRINT, report, synthetic_map, timed

CELLS = (("default", 1.0), ("half", 0.5), ("twice", 2.0))
CHUNK_BYTES = 1 << 30


def torch_nearest(q, ref):
    """Chunked cdist + min: (idx int64, dist float32)."""
    step = max(1, CHUNK_BYTES // (4 * max(ref.shape[0], 1)))
    idx, dist = [], []
    for a in range(0, q.shape[0], step):
        d, i = torch.cdist(q[a:a + step], ref).min(1)
        idx.append(i)
        dist.append(d)
    return torch.cat(idx), torch.cat(dist)


def rows_27(ref, q, origin, cell, dims):
    """Mean over the queries of the reference rows in the 27 cells around
    the query's (torch, float64 cell arithmetic as s3k.h states it)."""
    dev = ref.device
    org = torch.tensor(origin, device=dev, dtype=torch.float64)
    top = torch.tensor(dims, device=dev, dtype=torch.float64) - 1.0
    cell_of = lambda p: torch.minimum(torch.floor((p.double() - org) / cell).clamp_min(0.0),
                                      top).long()
    flat = lambda c: (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    counts = torch.bincount(flat(cell_of(ref)), minlength=dims[0] * dims[1] * dims[2])
    vol = counts.reshape(1, 1, dims[2], dims[1], dims[0]).float()
    box = torch.nn.functional.avg_pool3d(vol, 3, 1, 1, count_include_pad=True) * 27.0
    return float(box.reshape(-1)[flat(cell_of(q))].mean())


def surface_mesh(k, device):
    """A k x k vertex grid over the undulating surface: 2 (k - 1)^2 triangles."""
    g = torch.linspace(-1.5, 1.5, k, device=device)
    y, x = torch.meshgrid(g, g, indexing="ij")
    z = 2.0 + 0.15 * torch.sin(1.7 * x) * torch.cos(2.3 * y)
    verts = torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()
    i = (torch.arange(k - 1, device=device)[:, None] * k
         + torch.arange(k - 1, device=device)[None, :]).reshape(-1)
    faces = torch.cat([torch.stack([i, i + 1, i + k], 1), torch.stack([i + 1, i + k + 1, i + k], 1)])
    return verts, faces.to(torch.int32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200000, 2000000])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--torch-subset-above", type=int, default=500000,
                    help="above this many rows the torch composition runs on a tenth of the queries")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--mesh-side", type=int, default=1501)
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    base.LOG = a.log
    if not torch.cuda.is_available():
        raise SystemExit("bench_nn_search needs a GPU")
    dev = torch.device("cuda", 0)
    for n in a.sizes:
        ref = synthetic_map(n, dev)[0]
        g = torch.Generator(device=dev).manual_seed(1)
        q = (ref + torch.randn(n, 3, generator=g, device=dev) * FOOTPRINT).contiguous()
        _, cell0, _ = default_grid(ref)
        exact = None
        for name, factor in CELLS:
            origin, cell, dims = default_grid(ref, cell=cell0 * factor)
            kw = dict(origin=origin, cell=cell, dims=dims)
            cells = dims[0] * dims[1] * dims[2]
            P = -(-cells.bit_length() // 8)
            grid = PointGrid(ref, **kw)
            idx, dist = grid.query(q)
            if exact is None:
                exact = (idx, dist)
            same = bool(torch.equal(idx, exact[0])) and bool(torch.equal(dist, exact[1]))
            common = dict(n=n, cell=name, cell_m=cell, dims=list(dims))
            us = timed(lambda: PointGrid(ref, **kw), a.rounds, a.iters, a.warmup)
            report(variant="hip_build", us=us, bytes=48 * n + 20 * cells, **common)
            R = rows_27(ref, q, origin, cell, dims)
            us = timed(lambda: grid.query(q), a.rounds, a.iters, a.warmup)
            report(variant="hip_query", us=us, sort_passes=P, rows_27=round(R, 1),
                   bytes=int((100 + 20 * P + 16 * R) * n), same_as_default_cell=same,
                   mean_dist_m=round(float(dist.mean()), 6), **common)
            if name != "twice":
                # the walks not chosen (nn.set_query_mode), on the queries as they
                # come (pixel order: neighbours in memory are neighbours in space)
                # and on a random permutation of them
                perm = torch.randperm(n, device=dev, generator=g)
                q_shuf = q[perm].contiguous()
                for order, qq in (("as_given", q), ("shuffled", q_shuf)):
                    for mode in ("sorted", "unsorted", "wave"):
                        if (order, mode) == ("as_given", "sorted"):
                            continue
                        set_query_mode(mode)
                        try:
                            i2, d2 = grid.query(qq)
                            want = (exact[0][perm], exact[1][perm]) if order == "shuffled" else exact
                            ok = bool(torch.equal(i2, want[0])) and bool(torch.equal(d2, want[1]))
                            us2 = timed(lambda: grid.query(qq), a.rounds, a.iters, a.warmup)
                        finally:
                            set_query_mode("sorted")
                        report(variant="hip_query_ab", mode=mode, query_order=order, us=us2,
                               over_sorted_as_given=round(us2["median"] / us["median"], 2),
                               same_bits=ok, **common)
                del perm, q_shuf
            del grid
        if not a.no_torch:
            part = n > a.torch_subset_above
            qs = q[:n // 10] if part else q
            t_idx, _ = torch_nearest(qs, ref)
            agree = float((t_idx == exact[0][:qs.shape[0]].long()).float().mean())
            tus = timed(lambda: torch_nearest(qs, ref), a.torch_rounds, 1, 1)
            if part:
                tus = {k: round(v * 10.0, 1) for k, v in tus.items()}
            report(n=n, variant="torch_cdist_min", us=tus, same_index=round(agree, 6),
                   scaled_from=qs.shape[0] if part else None)
        del ref, q, exact
        torch.cuda.empty_cache()
    verts, faces = surface_mesh(a.mesh_side, dev)
    us = timed(lambda: sample_mesh(verts, faces, a.samples), a.rounds, a.iters, a.warmup)
    F = faces.shape[0]
    report(variant="hip_sample_mesh", faces=F, samples=a.samples, us=us,
           bytes=F * (12 + 36 + 8 + 2 * 8 + 8) + a.samples * (16 + 23 * 8 + 48))


if __name__ == "__main__":
    main()
