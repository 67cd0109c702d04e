"""numpy float64 restatement of s3k_knn (include/s3k.h): the k nearest rows by
brute force, every candidate sorted.  It takes nothing from the code under
test and knows no grid.  Also the statistical outlier rule of
splatt3r_amd.nn.outlier_mask, with exactly rounded sums."""
import math

import numpy as np

f32 = np.float32
K_MAX = 32


def neighbours(q, ref, max_dist=np.inf, exclude_self=False, k_max=K_MAX, chunk=256):
    """(idx [m, k_max] int64, d2 [m, k_max] float64): per query the first
    k_max candidates in ascending (d2, index) order, -1 / +inf past the last.
    Candidates: the finite rows i of ref, without i = j for query j when
    exclude_self, with d2 = (dx dx + dy dy) + dz dz in float64 on the float32
    inputs, d2 <= max_dist max_dist.  A non-finite query has none."""
    q = np.ascontiguousarray(q, f32).reshape(-1, 3)
    ref = np.ascontiguousarray(ref, f32).reshape(-1, 3)
    m = len(q)
    idx = np.full((m, k_max), -1, np.int64)
    d2o = np.full((m, k_max), np.inf, np.float64)
    kept = np.nonzero(np.isfinite(ref).all(1))[0]
    if len(kept) == 0 or m == 0:
        return idx, d2o
    r = ref[kept].astype(np.float64)
    limit = np.float64(max_dist) * np.float64(max_dist)
    ok_q = np.isfinite(q).all(1)
    for a in range(0, m, chunk):
        rows = np.nonzero(ok_q[a:a + chunk])[0] + a
        if len(rows) == 0:
            continue
        p = q[rows].astype(np.float64)
        dx = p[:, None, 0] - r[None, :, 0]
        dy = p[:, None, 1] - r[None, :, 1]
        dz = p[:, None, 2] - r[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        index = np.broadcast_to(kept[None, :], d2.shape)
        counts = d2 <= limit
        if exclude_self:
            counts &= index != rows[:, None]
        order = np.lexsort((index, d2), axis=-1)
        for t, row in enumerate(rows):
            o = order[t][counts[t][order[t]]][:k_max]
            idx[row, :len(o)] = kept[o]
            d2o[row, :len(o)] = d2[t, o]
    return idx, d2o


def rows(idx, d2, k):
    """dict(idx [m, k] int32, dist [m, k] float32, mean [m], mean_sq [m]
    float32) of the first k slots of neighbours(): dist = (float)sqrt(d2);
    the means over the filled slots, float64 sums in slot order
    (np.add.accumulate is sequential), +inf when no slot is filled."""
    idx, d2 = idx[:, :k], d2[:, :k]
    has = idx >= 0
    c = has.sum(1)
    root = np.sqrt(np.where(has, d2, 0.0))
    acc_d = np.add.accumulate(root, axis=1)
    acc_d2 = np.add.accumulate(np.where(has, d2, 0.0), axis=1)
    last = np.maximum(c, 1) - 1
    take = np.arange(len(idx))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(c > 0, acc_d[take, last] / c, np.inf).astype(f32)
        mean_sq = np.where(c > 0, acc_d2[take, last] / c, np.inf).astype(f32)
    dist = np.where(has, root, np.inf).astype(f32)
    return dict(idx=idx.astype(np.int32), dist=dist, mean=mean, mean_sq=mean_sq)


def knn(q, ref, k, max_dist=np.inf, exclude_self=False):
    return rows(*neighbours(q, ref, max_dist, exclude_self, k_max=k), k)


def outliers(points, k, std_ratio):
    """dict(keep [n] bool, thr, gap): the rule of nn.outlier_mask on the
    reference's means, the sums exactly rounded (math.fsum).  gap is the
    smallest |mean - thr| / thr over the finite means."""
    points = np.ascontiguousarray(points, f32).reshape(-1, 3)
    mean = knn(points, points, k, exclude_self=True)["mean"].astype(np.float64)
    ok = np.isfinite(mean)
    c = int(ok.sum())
    if c < 2:
        return dict(keep=np.isfinite(points).all(1), thr=math.inf, gap=math.inf)
    s1, s2 = math.fsum(mean[ok]), math.fsum(mean[ok] * mean[ok])
    mu = s1 / c
    var = max(0.0, s2 - s1 * mu) / (c - 1)
    thr = mu + std_ratio * math.sqrt(var)
    gap = float(np.abs(mean[ok] - thr).min() / thr) if thr > 0.0 else 0.0
    return dict(keep=ok & (mean <= thr), thr=thr, gap=gap)
