"""numpy float64 restatement of map compaction (include/s3v.h): voxel keys,
groups in (key, index) order, the moment-matched merge.  The checker of
tests/test_map_compact.py; it shares no code with the kernel and takes the
definition literally (the mean first, then the covariance about that mean,
raw coordinates in double)."""
import numpy as np

BIAS = 1 << 20
TOP = (1 << 21) - 1


def voxel_cells(means, voxel, origin=(0.0, 0.0, 0.0)):
    """[n, 3] int64 cells: floor(((double)x - origin) / voxel) + 2^20, clamped
    to [0, 2^21 - 1].  `means` must be finite."""
    x = np.asarray(means, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        t = np.floor((x - np.asarray(origin, np.float64)) / np.float64(voxel)) + BIAS
    return np.clip(t, 0, TOP).astype(np.int64)


def voxel_keys(means, voxel, origin=(0.0, 0.0, 0.0)):
    """[n] int64 keys ix << 42 | iy << 21 | iz."""
    c = voxel_cells(means, voxel, origin)
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def _segsum(x, starts):
    """Per-group sums of the rows of x (sorted order), groups starting at `starts`."""
    return np.add.reduceat(x, starts, axis=0)


def merge_ref(means, cov_triu, colors, opacities, kf_id, voxel, origin=(0.0, 0.0, 0.0), n=None):
    """Returns a dict: means [m, 3], cov_triu [m, 6], colors [m, 3],
    opacities [m] (float64, not rounded), kf_id [m] int32, first [m] int64,
    group [n] int64 (-1: dropped), size [m] int64 (members per group), m,
    dropped."""
    n = len(means) if n is None else min(int(n), len(means))
    mu = np.asarray(means, np.float32)[:n].astype(np.float64).reshape(n, 3)
    cov = np.asarray(cov_triu, np.float32)[:n].astype(np.float64).reshape(n, 6)
    col = np.asarray(colors, np.float32)[:n].astype(np.float64).reshape(n, 3)
    op = np.asarray(opacities, np.float32)[:n].astype(np.float64).reshape(n)
    kf = np.asarray(kf_id, np.int32)[:n]
    ok = (np.isfinite(mu).all(1) & np.isfinite(cov).all(1) & np.isfinite(col).all(1)
          & np.isfinite(op))
    group = np.full(n, -1, np.int64)
    kept = np.flatnonzero(ok)
    dropped = int(n - len(kept))
    if len(kept) == 0:
        z = np.zeros
        return dict(means=z((0, 3)), cov_triu=z((0, 6)), colors=z((0, 3)), opacities=z(0),
                    kf_id=z(0, np.int32), first=z(0, np.int64), size=z(0, np.int64), group=group,
                    m=0, dropped=dropped)
    keys = voxel_keys(mu[kept], voxel, origin)
    order = kept[np.lexsort((kept, keys))]        # by key, then index
    skeys = voxel_keys(mu[order], voxel, origin)
    starts = np.flatnonzero(np.r_[True, skeys[1:] != skeys[:-1]])
    size = np.diff(np.r_[starts, len(order)])
    gid = np.repeat(np.arange(len(starts)), size)  # group of each sorted row
    o, x, c, S = op[order], mu[order], col[order], cov[order]
    w = np.where((_segsum(o, starts) == 0.0)[gid], 1.0, o)   # all-zero weights: every w = 1
    W = _segsum(w, starts)
    mean = _segsum(w[:, None] * x, starts) / W[:, None]
    d = x - mean[gid]
    dd = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2],
                   d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
    sigma = _segsum(w[:, None] * (S + dd), starts) / W[:, None]
    colour = _segsum(w[:, None] * c, starts) / W[:, None]
    opac = _segsum(w * o, starts) / W
    first = order[starts]                         # sorted by index within a key: the lowest
    by_first = np.argsort(first, kind="stable")   # output order
    row_of = np.empty(len(starts), np.int64)
    row_of[by_first] = np.arange(len(starts))
    group[order] = row_of[gid]
    return dict(means=mean[by_first], cov_triu=sigma[by_first], colors=colour[by_first],
                opacities=opac[by_first], kf_id=kf[first[by_first]], first=first[by_first],
                size=size[by_first], group=group, m=len(starts), dropped=dropped)
