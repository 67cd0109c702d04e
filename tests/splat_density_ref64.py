"""Reference of adaptive density control (include/s3d.h): numpy, float64 (the
reference) or float32 (the rounding floor), Philox4x32-10 in integer
arithmetic.  Shares no code with csrc/splat_density_math.hpp or
splatt3r_amd/refine.py.

A row is x y z | f_dc | logit | log scale | rot w x y z (raw); statistics are
grad_accum float32 [n], denom int32 [n], max_radii int32 [n].
"""
import numpy as np

from splat_opt_ref64 import ZERO_QUAT_ROW, make_inputs as make_rows
from splat_ref64 import tolerance  # noqa: F401  (4 x floor, one significant digit up)

PRUNE, KEEP, CLONE, SPLIT = 0, 1, 2, 3
f32 = np.float32
LOG_SPLIT = float(f32(np.log(1.6)))
M32 = np.uint64(0xFFFFFFFF)

# thresholds of the test inputs (float32 values, as the ABI carries them)
PARAMS = dict(grad_threshold=float(f32(2e-4)), split_scale=float(f32(np.exp(-1.2))),
              min_opacity=float(f32(1.0 / (1.0 + np.exp(9.0)))), max_scale=float(f32(np.exp(0.8))),
              max_screen_radius=100, seed=0x0123456789ABCDEF, **{"pass": 3})
ON_THRESHOLD_ROWS = (20, 21, 22)     # avg == grad_threshold exactly, denom 1
NAN_ROW, INF_ROW = 30, 31


# ------------------------------------------------------------------ Philox --
def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (integers < 2^32) -> [..., 4] uint64 words."""
    c = [np.asarray(ctr)[..., j].astype(np.uint64) for j in range(4)]
    k0, k1 = (np.asarray(key)[..., j].astype(np.uint64) for j in range(2))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]          # < 2^64: no wrap
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, -1)


def normals(rows, pass_, k, seed, drop_k=False):
    """eps [m, 3] float64 holding float32 values: counter (row lo32, row hi32,
    pass, k), key (seed lo32, seed hi32)."""
    rows = np.asarray(rows, np.uint64)
    m = len(rows)
    ctr = np.stack([rows & M32, rows >> np.uint64(32), np.full(m, pass_, np.uint64),
                    np.full(m, 0 if drop_k else k, np.uint64)], -1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64), (m, 2))
    x = philox4x32_10(ctr, key).astype(np.float64)
    u = (x + 0.5) / 4294967296.0
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    z = np.stack([r0 * np.cos(2.0 * np.pi * u[:, 1]), r0 * np.sin(2.0 * np.pi * u[:, 1]),
                  r1 * np.cos(2.0 * np.pi * u[:, 3])], 1)
    return z.astype(f32).astype(np.float64)


# ---------------------------------------------------------------- decision --
def activations(rows):
    """(o, smax, avg-free): sigmoid and exp formed in double, rounded to
    float32 once."""
    r = np.asarray(rows, np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(r[:, 6]))
        o = (np.where(r[:, 6] >= 0, 1.0, e) / (1.0 + e)).astype(f32)
        s = np.exp(r[:, 7:10]).astype(f32)
    return o, s.max(1)


def decide(rows, stats, p):
    """codes [n], and near [n]: rows whose avg, o or smax lies within relative
    1e-5 of its threshold (a row put exactly on avg == grad_threshold with
    denom 1 is not near: it pins the >=)."""
    rows = np.asarray(rows)
    ga, dn, mr = (np.asarray(t) for t in stats)
    finite = np.isfinite(rows).all(1)
    o, smax = activations(np.where(np.isfinite(rows), rows, 0.0))
    with np.errstate(all="ignore"):
        avg = np.where(dn > 0, ga.astype(np.float64) / np.where(dn > 0, dn, 1), 0.0)
    prune = ~finite | (o < f32(p["min_opacity"]))
    if p["max_scale"] > 0:
        prune |= smax > f32(p["max_scale"])
    if p["max_screen_radius"] > 0:
        prune |= mr > p["max_screen_radius"]
    grow = ~prune & (avg >= p["grad_threshold"])
    split = grow & (smax > f32(p["split_scale"]))
    codes = np.where(prune, PRUNE, np.where(split, SPLIT, np.where(grow, CLONE, KEEP)))
    close = lambda x, t: np.abs(np.asarray(x, np.float64) - t) <= 1e-5 * abs(t)
    near = close(avg, p["grad_threshold"]) & ~((dn == 1) & (avg == p["grad_threshold"]))
    near |= close(o, p["min_opacity"]) | close(smax, p["split_scale"])
    if p["max_scale"] > 0:
        near |= close(smax, p["max_scale"])
    return codes.astype(np.int64), near & finite


def prune_causes(rows, stats, p):
    """[n, 4] bool: non-finite, opacity, world scale, screen radius."""
    rows = np.asarray(rows)
    finite = np.isfinite(rows).all(1)
    o, smax = activations(np.where(np.isfinite(rows), rows, 0.0))
    return np.stack([~finite, finite & (o < f32(p["min_opacity"])),
                     finite & (smax > f32(p["max_scale"])),
                     finite & (np.asarray(stats[2]) > p["max_screen_radius"])], 1)


# ---------------------------------------------------------------- children --
def children(rows, idx, k, p, dtype=np.float64, ablate=()):
    """Child k of the rows `idx` (their indices feed the counter): [m, 14] of
    `dtype`.  float64: the reference; float32: the same composition with
    every operation rounded to float32 (the floor)."""
    r = np.asarray(rows)[idx].astype(dtype)
    eps = normals(idx, p["pass"], k, p["seed"], drop_k="k" in ablate).astype(dtype)
    s = np.exp(r[:, 7:10])
    q = r[:, 10:14]
    nn = np.sqrt((q * q).sum(1, keepdims=True))
    live = nn > 0
    ident = np.zeros_like(q)
    ident[:, 0] = 1
    q = np.where(live, q / np.where(live, nn, 1), ident)
    w, x, y, z = q.T
    one, two = dtype(1), dtype(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)],
                 1).reshape(-1, 3, 3)
    d = eps if "s" in ablate else s * eps
    off = d if "R" in ablate else np.einsum("nij,nj->ni", R, d)
    c = r.copy()
    c[:, 0:3] = r[:, 0:3] + off.astype(dtype)
    if "log" not in ablate:
        c[:, 7:10] = r[:, 7:10] - dtype(LOG_SPLIT)
    return c


def densify(rows, m, v, stats, p, cap, dtype=np.float64, ablate=()):
    """The whole pass.  Returns a dict: rows, m, v [n_out, 14] (`dtype`),
    origin [n_out], n_out, counts (pruned, cloned, split, denied), codes [n],
    near [n], granted [n], child [n_out] (True for a split child)."""
    rows, m, v = (np.asarray(t) for t in (rows, m, v))
    n = len(rows)
    assert cap >= n
    codes, near = decide(rows, stats, p)
    alive = codes != PRUNE
    grows = codes >= CLONE
    B = int(alive.sum())
    grow_before = np.cumsum(grows) - grows
    granted = grows & (grow_before < cap - B)
    n_rows = alive.astype(np.int64) + granted
    off = np.cumsum(n_rows) - n_rows
    n_out = int(n_rows.sum())
    out = [np.zeros((n_out, 14), dtype) for _ in range(3)]
    origin = np.zeros(n_out, np.int64)
    child = np.zeros(n_out, bool)
    idx = np.arange(n)
    sp = granted & (codes == SPLIT)
    whole = alive & ~sp                      # kept, denied, and a clone's original
    for o_, src in zip(out, (rows, m, v)):
        o_[off[whole]] = src[whole].astype(dtype)
    origin[off[whole]] = idx[whole]
    cl = granted & (codes == CLONE)
    out[0][off[cl] + 1] = rows[cl].astype(dtype)
    origin[off[cl] + 1] = ~idx[cl]
    for k in (0, 1):
        out[0][off[sp] + k] = children(rows, idx[sp], k, p, dtype, ablate)
        origin[off[sp] + k] = ~idx[sp]
        child[off[sp] + k] = True
    G = int(grows.sum())
    counts = (n - B, int(cl.sum()), int(sp.sum()), G - int(granted.sum()))
    return dict(rows=out[0], m=out[1], v=out[2], origin=origin, n_out=n_out, counts=counts,
                codes=codes, near=near, granted=granted, child=child)


# -------------------------------------------------- statistics and the reset --
def accumulate(d2, radii, stats, dtype=np.float64):
    """One step; grad_accum is carried in `dtype`.  Returns new statistics."""
    ga, dn, mr = (np.array(t) for t in stats)
    d2 = np.asarray(d2)
    ok = (np.asarray(radii) > 0) & np.isfinite(d2[:, 0]) & np.isfinite(d2[:, 1])
    d = np.where(ok[:, None], d2[:, :2], 0).astype(dtype)
    g = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    ga = ga.astype(dtype)
    ga[ok] = ga[ok] + g[ok]
    dn[ok] += 1
    mr[ok] = np.maximum(mr[ok], np.asarray(radii)[ok])
    return ga, dn, mr


def reset_opacity(rows, m, v, logit_cap):
    rows, m, v = (np.array(t) for t in (rows, m, v))
    rows[:, 6] = np.minimum(rows[:, 6], f32(logit_cap))
    m[:, 6] = 0
    v[:, 6] = 0
    return rows, m, v


# ------------------------------------------------------------------ errors --
def _row_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not len(a):
        return 0.0
    return float((np.abs(a - b).max(1) / np.abs(b).max(1)).max())


def child_errors(got_rows, ref):
    """Errors of the split children's means and log scales, per row relative
    to the row's largest reference entry of the group."""
    c = ref["child"]
    return {"child.means": _row_err(np.asarray(got_rows)[c, 0:3], ref["rows"][c, 0:3]),
            "child.log_scale": _row_err(np.asarray(got_rows)[c, 7:10], ref["rows"][c, 7:10])}


def accum_error(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nz = ref != 0
    assert not got[~nz].any()
    return float((np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])).max()) if nz.any() else 0.0


# ------------------------------------------------------------------ inputs --
def make_inputs(n=1000, seed=77):
    """(rows, m, v, (grad_accum, denom, max_radii)) for PARAMS: rows in the
    ranges of splat_opt_ref64.make_inputs; about a fifth each pruned, cloned
    and split."""
    rng = np.random.default_rng(seed)
    rows = make_rows(n)[0].copy()
    m = (rng.normal(size=(n, 14)) * 1e-3).astype(f32)
    v = (rng.random((n, 14)) * 1e-5 + 1e-12).astype(f32)
    dn = rng.integers(0, 6, n).astype(np.int32)
    dn[rng.random(n) < 0.05] = 0
    avg = np.exp(rng.uniform(np.log(1e-5), np.log(1e-2), n))
    ga = (avg * np.maximum(dn, 1)).astype(f32)            # non-zero where denom == 0 too
    mr = rng.integers(0, 105, n).astype(np.int32)
    if n > max(ON_THRESHOLD_ROWS + (NAN_ROW, INF_ROW, ZERO_QUAT_ROW)):
        z = ZERO_QUAT_ROW                                  # a zero quaternion that splits
        rows[z, 6], rows[z, 7:10] = 1.0, (0.0, -1.0, -2.0)
        ga[z], dn[z], mr[z] = 1.0, 2, 5
        for j, i in enumerate(ON_THRESHOLD_ROWS):          # avg == grad_threshold exactly
            rows[i, 6] = 0.5
            rows[i, 7:10] = (-3.0, -4.0, -5.0) if j else (0.0, -1.0, -1.0)
            ga[i], dn[i], mr[i] = PARAMS["grad_threshold"], 1, 3
        rows[NAN_ROW, 4] = np.nan
        rows[INF_ROW, 8] = np.inf
    return rows, m, v, (ga, dn, mr)


def tile_inputs(n, base=None):
    """The 1,000-row inputs repeated to n rows."""
    rows, m, v, st = base if base is not None else make_inputs()
    idx = np.arange(n) % len(rows)
    return rows[idx], m[idx], v[idx], tuple(t[idx] for t in st)
