"""numpy float64 restatement of include/s3k.h: brute-force nearest neighbour
with the tie and drop rules, the distance statistics, the stratified mesh
sampler (Philox4x32-10 from splat_density_ref64) and Umeyama's alignment.  It
takes nothing from the code under test and knows no grid."""
import math

import numpy as np

from splat_density_ref64 import philox4x32_10

f32 = np.float32
M32 = np.uint64(0xFFFFFFFF)
TWO32 = 4294967296.0


# ------------------------------------------------------ nearest neighbour --
def nearest(q, ref, max_dist=np.inf, chunk=512):
    """(idx [m] int32, dist [m] float32): over the finite rows i of ref,
    d2_i = (dx dx + dy dy) + dz dz in float64 on the float32 inputs, the
    smallest d2 wins, ties to the smallest i; it counts only if
    d2 <= max_dist max_dist.  -1 / +inf when none does or the query row is
    not finite."""
    q = np.ascontiguousarray(q, f32).reshape(-1, 3)
    ref = np.ascontiguousarray(ref, f32).reshape(-1, 3)
    m = len(q)
    idx = np.full(m, -1, np.int32)
    dist = np.full(m, np.inf, f32)
    kept = np.nonzero(np.isfinite(ref).all(1))[0]
    if len(kept) == 0 or m == 0:
        return idx, dist
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
        j = d2.argmin(1)                       # the first minimum: the lowest kept index
        best = d2[np.arange(len(rows)), j]
        hit = best <= limit
        idx[rows[hit]] = kept[j[hit]].astype(np.int32)
        dist[rows[hit]] = np.sqrt(best[hit]).astype(f32)
    return idx, dist


def nearest_prefiltered(q, ref, chunk=1024):
    """nearest(q, ref) for finite rows, a few times faster at 20,000 rows: a
    float64 matrix product gives |q|^2 + |r|^2 - 2 q.r, wrong by a few 2^-52
    of scale = max |q|^2 + max |r|^2; every pair within 1e-9 scale of a row's
    minimum of that (five orders above its error) is then evaluated by the
    definition, and the smallest d2, lowest index first, wins."""
    q = np.ascontiguousarray(q, f32).reshape(-1, 3)
    ref = np.ascontiguousarray(ref, f32).reshape(-1, 3)
    assert np.isfinite(q).all() and np.isfinite(ref).all() and len(ref)
    p, r = q.astype(np.float64), ref.astype(np.float64)
    rn = (r * r).sum(1)
    scale = (p * p).sum(1).max() + rn.max()
    idx = np.empty(len(q), np.int32)
    dist = np.empty(len(q), f32)
    for a in range(0, len(q), chunk):
        pc = p[a:a + chunk]
        approx = (pc * pc).sum(1)[:, None] + rn[None, :] - 2.0 * (pc @ r.T)
        rows, cols = np.nonzero(approx <= approx.min(1)[:, None] + 1e-9 * scale)
        dx, dy, dz = (pc[rows, k] - r[cols, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        order = np.lexsort((cols, d2, rows))
        rows, cols, d2 = rows[order], cols[order], d2[order]
        first = np.unique(rows, return_index=True)[1]
        idx[a:a + chunk] = cols[first]
        dist[a:a + chunk] = np.sqrt(d2[first]).astype(f32)
    return idx, dist


def dropped(ref):
    return int((~np.isfinite(np.asarray(ref, f32).reshape(-1, 3)).all(1)).sum())


# -------------------------------------------------------------- statistics --
def stats(dist, threshold):
    """(count, sum d, sum d^2, count of d <= threshold, max) over the finite
    entries, the sums exactly rounded (math.fsum); max -inf when none."""
    d = np.asarray(dist, f32).astype(np.float64)
    d = d[np.isfinite(d)]
    return (float(len(d)), math.fsum(d), math.fsum(d * d), float((d <= threshold).sum()),
            float(d.max()) if len(d) else -math.inf)


def stats_in_order(dist, threshold):
    """The same five values with the two sums (and the counts) added in the
    order include/s3k.h fixes: segments of 2,048 entries, 256 threads of 8
    consecutive entries each, a pairwise tree over the threads (t += t + o for
    o = 128, 64, .. 1); then thread t adds the segments' partials t, t + 256,
    .. in order, and the same tree.  A skipped entry is a term of 0."""
    d = np.asarray(dist, f32).astype(np.float64).reshape(-1)
    nblk = -(-len(d) // 2048)
    d = np.concatenate([d, np.full(nblk * 2048 - len(d), np.nan)])
    ok = np.isfinite(d)
    z = np.where(ok, d, 0.0)
    terms = np.stack([ok.astype(np.float64), z, z * z, (ok & (d <= threshold)).astype(np.float64)])

    def tree(v):                                   # [4, k, 256] -> [4, k]
        v = v.copy()
        o = 128
        while o:
            v[..., :o] = v[..., :o] + v[..., o:2 * o]
            o //= 2
        return v[..., 0]
    t = terms.reshape(4, nblk, 256, 8)
    v = np.zeros((4, nblk, 256))
    for k in range(8):
        v = v + t[..., k]
    part = tree(v)                                 # [4, nblk]
    pad = -(-max(nblk, 1) // 256) * 256
    part = np.concatenate([part, np.zeros((4, pad - nblk))], 1).reshape(4, -1, 256)
    v = np.zeros((4, 256))
    for k in range(part.shape[1]):
        v = v + part[:, k]
    out = tree(v[:, None, :])[:, 0]
    return (float(out[0]), float(out[1]), float(out[2]), float(out[3]),
            float(d[ok].max()) if ok.any() else -math.inf)


# ----------------------------------------------------------------- sampler --
def face_areas(verts, faces):
    """(area [F] float64, bad [F] bool): 0.5 |(b - a) x (c - a)| in float64; a
    face with an index outside [0, V) or a non-finite area has area 0."""
    verts = np.asarray(verts, f32).reshape(-1, 3).astype(np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(verts)
    inside = ((faces >= 0) & (faces < V)).all(1)
    fc = np.where(inside[:, None], faces, 0)
    if V == 0:
        return np.zeros(len(faces)), np.ones(len(faces), bool)
    a, b, c = verts[fc[:, 0]], verts[fc[:, 1]], verts[fc[:, 2]]
    e1, e2 = b - a, c - a
    with np.errstate(all="ignore"):
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    bad = ~inside | ~np.isfinite(area)
    return np.where(bad, 0.0, area), bad


def weights(verts, faces):
    """(w [F] uint64, C [F] uint64 inclusive sums, bad count)."""
    area, bad = face_areas(verts, faces)
    a_max = area.max() if len(area) else 0.0
    if a_max > 0.0:
        w = np.floor(area / a_max * TWO32).astype(np.uint64)
    else:
        w = np.zeros(len(area), np.uint64)
    return w, np.cumsum(w, dtype=np.uint64), int(bad.sum())


def sample_mesh(verts, faces, S, seed):
    """dict(points [S, 3] float32, face [S] int32, bad, total, w, u): the
    stratified sampler of include/s3k.h; points and face are None when the
    total weight is 0."""
    verts32 = np.asarray(verts, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    w, C, n_bad = weights(verts32, faces)
    Q = int(C[-1]) if len(C) else 0
    out = dict(points=None, face=None, bad=n_bad, total=Q, w=w, u=None)
    if Q == 0:
        return out
    k = np.arange(S, dtype=np.uint64)
    ctr = np.stack([k & M32, k >> np.uint64(32), np.zeros(S, np.uint64), np.zeros(S, np.uint64)], -1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64), (S, 2))
    u = (philox4x32_10(ctr, key).astype(np.float64) + 0.5) / TWO32
    t = np.floor((k.astype(np.float64) + u[:, 0]) / np.float64(S) * np.float64(np.uint64(Q)))
    t = np.minimum(t.astype(np.uint64), np.uint64(Q - 1))
    f = np.searchsorted(C, t, side="right")            # the smallest f with C_f > t
    v = verts32.astype(np.float64)
    a, b, c = v[faces[f, 0]], v[faces[f, 1]], v[faces[f, 2]]
    s = np.sqrt(u[:, 1])
    wa, wb, wc = (1.0 - s)[:, None], (s * (1.0 - u[:, 2]))[:, None], (s * u[:, 2])[:, None]
    out.update(points=((wa * a + wb * b) + wc * c).astype(f32), face=f.astype(np.int32), u=u)
    return out


def barycentric(points, verts, faces, face):
    """Barycentric coordinates [S, 3] of each point in its face's plane,
    float64 (least squares on the two edge vectors)."""
    v = np.asarray(verts, f32).astype(np.float64)
    tri = np.asarray(faces, np.int64)[np.asarray(face, np.int64)]
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    e1, e2, d = b - a, c - a, np.asarray(points, np.float64) - a
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
    det = g11 * g22 - g12 * g12
    lb, lc = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
    return np.stack([1.0 - lb - lc, lb, lc], 1)


# ---------------------------------------------------------------- alignment --
def umeyama(src, dst, with_scale=True):
    """(s, R, t) of Umeyama 1991, eqs. 40-43, in float64."""
    x, y = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = len(x)
    mx, my = x.sum(0) / n, y.sum(0) / n
    sx2 = ((x - mx) ** 2).sum() / n
    cov = sum(np.outer(b - my, a - mx) for a, b in zip(x, y)) / n
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(cov) < 0.0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    s = np.trace(np.diag(D) @ S) / sx2 if with_scale else 1.0
    return float(s), R, my - s * R @ mx


def ate(est, gt, transform):
    """Per-pose translation errors |gt - (s R est + t)|."""
    s, R, t = transform
    return np.sqrt(((np.asarray(gt, np.float64) - (s * (np.asarray(est, np.float64) @ R.T) + t))
                    ** 2).sum(1))
