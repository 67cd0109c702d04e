"""numpy float64 restatement of the depth loss and depth-metric sums
(include/s3z.h): per-pixel terms, per-image sums, the residual map and both
gradients, and cases(), the named synthetic inputs of tests/test_depth_loss.py.

Every operation is one IEEE double operation in the order
csrc/depth_loss_math.hpp fixes, so the per-pixel quantities (rmap, the
gradients, the counts) are comparable bit for bit; the sums are added exactly
(math.fsum), so a sum of the code under test differs from them only by its own
order of addition.  Takes nothing from the code under test but the tile size
the shapes are placed around (S3Z_TILE_W, S3Z_TILE_H of the header).
"""
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64
NAMES = ("W", "ABS", "SQ", "ABSREL", "SQREL", "LOGSQ", "GRAD", "WG", "D1", "D2", "D3", "N",
         "QZ", "QQ")
IDX = {k: i for i, k in enumerate(NAMES)}
COUNTS = ("D1", "D2", "D3", "N")


def _inputs(D, A, z, w, s):
    D, A, z = (np.asarray(t, f32).astype(f64) for t in (D, A, z))
    B = D.shape[0]
    w = np.ones_like(D) if w is None else np.asarray(w, f32).astype(f64)
    s = np.ones(B, f64) if s is None else np.asarray(s, f32).astype(f64)
    return D, A, z, w, s[:, None, None] * np.ones_like(D)


def pixels(D, A, z, w=None, s=None, alpha_min=0.5):
    """(valid, w, q, p, r) [B, H, W]: bool and float64; 0 where not valid."""
    D, A, z, w, s = _inputs(D, A, z, w, s)
    valid = (np.isfinite(z) & (z > 0) & np.isfinite(D) & np.isfinite(A) & (D > 0) & (A > 0)
             & (A >= alpha_min) & np.isfinite(w) & (w > 0) & np.isfinite(s) & (s > 0))
    one = np.ones_like(D)
    q = np.where(valid, np.where(valid, D, one) / np.where(valid, A, one), 0.0)
    p = np.where(valid, np.where(valid, s, one) * q, 0.0)
    r = np.where(valid, p - np.where(valid, z, one), 0.0)
    return valid, np.where(valid, w, 0.0), q, p, r


def _pairs(valid, w, r, axis):
    """(both valid, w_pq, r_q - r_p) of every pixel with its next neighbour along axis."""
    a = [slice(None)] * 3
    b = [slice(None)] * 3
    a[axis], b[axis] = slice(None, -1), slice(1, None)
    a, b = tuple(a), tuple(b)
    return valid[a] & valid[b], 0.5 * (w[a] + w[b]), r[b] - r[a]


def forward(D, A, z, w=None, s=None, alpha_min=0.5):
    """(sums [B, 14] float64, rmap [B, H, W] float32)."""
    valid, w, q, p, r = pixels(D, A, z, w, s, alpha_min)
    zz = np.where(valid, np.asarray(z, f32).astype(f64), 1.0)
    pp = np.where(valid, p, 1.0)
    a = np.abs(r)
    wa = w * a
    waa = wa * a
    l = np.log(pp) - np.log(zz)
    up, down = pp / zz, zz / pp
    ratio = np.where(up > down, up, down)
    wq = w * q
    t = {"W": w, "ABS": wa, "SQ": waa, "ABSREL": wa / zz, "SQREL": waa / zz, "LOGSQ": w * (l * l),
         "D1": ratio < 1.25, "D2": ratio < 1.5625, "D3": ratio < 1.953125,
         "N": np.ones_like(w), "QZ": wq * zz, "QQ": wq * q}
    B = w.shape[0]
    sums = np.zeros((B, len(NAMES)), f64)
    for b in range(B):
        for k, v in t.items():
            sums[b, IDX[k]] = math.fsum(np.where(valid[b], v[b], 0.0).ravel().tolist())
        g, wg = [], []
        for axis in (2, 1):
            both, wpq, d = _pairs(valid, w, r, axis)
            g += np.where(both[b], wpq[b] * np.abs(d[b]), 0.0).ravel().tolist()
            wg += np.where(both[b], wpq[b], 0.0).ravel().tolist()
        sums[b, IDX["GRAD"]], sums[b, IDX["WG"]] = math.fsum(g), math.fsum(wg)
    return sums, r.astype(f32)


def dl_dr(D, A, z, coef, w=None, s=None, alpha_min=0.5):
    """dL/dr [B, H, W] float64 of L = sum_b coef[b] . (ABS, SQ, GRAD)[b]; 0
    where not valid.  Neighbours in the order left, right, up, down."""
    valid, w, _, _, r = pixels(D, A, z, w, s, alpha_min)
    c = np.asarray(coef, f32).astype(f64)
    c_abs, c_sq, c_grad = (c[:, k][:, None, None] for k in range(3))

    def shifted(t, dy, dx):
        """t of the neighbour at (y + dy, x + dx); 0 outside the image."""
        out = np.zeros_like(t)
        H, W = t.shape[1:]
        ys, yd = (slice(1, H), slice(0, H - 1)) if dy > 0 else (slice(0, H - 1), slice(1, H)) \
            if dy < 0 else (slice(None), slice(None))
        xs, xd = (slice(1, W), slice(0, W - 1)) if dx > 0 else (slice(0, W - 1), slice(1, W)) \
            if dx < 0 else (slice(None), slice(None))
        out[:, yd, xd] = t[:, ys, xs]
        return out
    g = None
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        wn, rn = shifted(w, dy, dx), shifted(r, dy, dx)
        t = np.where(wn > 0, (0.5 * (w + wn)) * np.sign(r - rn), 0.0)
        g = t if g is None else g + t
    total = w * (c_abs * np.sign(r) + (2.0 * c_sq) * r) + c_grad * g
    return np.where(valid, total, 0.0)


def backward64(D, A, z, coef, w=None, s=None, alpha_min=0.5):
    """(dL/dD, dL/dA) in float64, before the one rounding to float32."""
    valid = pixels(D, A, z, w, s, alpha_min)[0]
    d = dl_dr(D, A, z, coef, w, s, alpha_min)
    Dd, Ad, _, _, sd = _inputs(D, A, z, w, s)
    As = np.where(valid, Ad, 1.0)
    gd = np.where(valid, d * (sd / As), 0.0)
    ga = np.where(valid, -(d * ((sd * Dd) / (As * As))), 0.0)
    return gd, ga


def backward(D, A, z, coef, w=None, s=None, alpha_min=0.5):
    with np.errstate(over="ignore"):
        return tuple(g.astype(f32) for g in backward64(D, A, z, coef, w, s, alpha_min))


# ------------------------------------------------------------------ cases --
def tile():
    from splatt3r_amd import _abi
    return _abi.constants["S3Z_TILE_W"], _abi.constants["S3Z_TILE_H"]


def shapes():
    """(H, W) around the workgroup tile."""
    tw, th = tile()
    return ((1, 1), (1, tw + 1), (th + 1, 1), (th - 1, tw - 1), (th, tw), (th + 1, tw + 1),
            (2 * th + 3, tw + 5))


def edge_pixels(H, W):
    """The (y, x) on both sides of every tile edge and at every tile corner."""
    tw, th = tile()
    ys = sorted({y for k in range(0, H + th, th) for y in (k - 1, k) if 0 <= y < H})
    xs = sorted({x for k in range(0, W + tw, tw) for x in (k - 1, k) if 0 <= x < W})
    return ys, xs


def _base(rng, B, H, W, weights):
    z = rng.uniform(0.5, 4.0, (B, H, W))
    A = rng.uniform(0.6, 1.0, (B, H, W)).astype(f32)
    q = z * (1.0 + rng.normal(0, 0.08, (B, H, W)))
    D = (q * A).astype(f32)
    w = rng.uniform(0.25, 2.0, (B, H, W)).astype(f32) if weights else None
    return D, A, z.astype(f32), w


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(D, A, z, w, s, alpha_min, coef); w and s may be None."""
    rng = np.random.default_rng(23)
    tw, th = tile()
    out = {}

    def add(name, D, A, z, w, s, alpha_min=0.5, coef=None):
        B = D.shape[0]
        coef = rng.uniform(-1.0, 1.0, (B, 3)).astype(f32) if coef is None else coef
        c = lambda t: None if t is None else np.ascontiguousarray(t, f32)
        out[name] = dict(D=c(D), A=c(A), z=c(z), w=c(w), s=c(s), alpha_min=float(alpha_min),
                         coef=c(coef))

    # every shape: plain, and dirty (every kind of invalid pixel, on the tile edges too)
    for H, W in shapes():
        D, A, z, w = _base(rng, 1, H, W, False)
        add(f"plain_{H}x{W}", D, A, z, None, None)
        D, A, z, w = _base(rng, 2, H, W, True)
        n = 2 * H * W
        flat = lambda t: t.reshape(-1)
        kinds = rng.permutation(n)
        # one of each kind first (as far as the pixels go), then 30 % of the rest at random
        kind = np.full(n, -1)
        kind[kinds[:min(n, 11)]] = np.arange(min(n, 11))
        rest = kinds[11:]
        kind[rest] = np.where(rng.uniform(size=len(rest)) < 0.3, rng.integers(0, 11, len(rest)), -1)
        ys, xs = edge_pixels(H, W)
        for y in ys:                       # invalid pixels on the tile edges and corners
            for x in xs:
                if (y + x) % 2 == 0:
                    kind.reshape(2, H, W)[:, y, x] = (3 * y + x) % 11
        for t, k, v in ((z, 0, np.nan), (z, 1, np.inf), (z, 2, 0.0), (z, 3, -1.5), (A, 4, 0.25),
                        (A, 6, 0.0), (w, 7, 0.0), (D, 8, np.nan), (A, 9, np.inf), (w, 10, -1.0)):
            flat(t)[kind == k] = v
        flat(A)[kind == 5] = 0.5           # exactly at alpha_min: valid
        flat(D)[kind == 6] = 0.0           # A = 0 with D = 0
        add(f"dirty_{H}x{W}", D, A, z, w, np.array([1.7, 0.6], f32))
    # B = 3, the middle image wholly invalid (no target)
    H, W = th + 1, tw + 1
    D, A, z, w = _base(rng, 3, H, W, True)
    z[1] = 0.0
    add("batch_one_invalid", D, A, z, w, np.array([1.0, 2.0, 0.5], f32))
    add("batch_one_invalid_noscale", D, A, z, None, None)
    # r = 0 exactly and r_p = r_q exactly: A = 1, z on a grid of 1/4, D = z (+ 1/4)
    H, W = th + 3, tw + 5
    z = (rng.integers(4, 16, (1, H, W)) / 4.0).astype(f32)
    A = np.ones((1, H, W), f32)
    D = z.copy()
    D[:, : H // 2] += 0.25                 # top half: r = 1/4 everywhere; bottom half: r = 0
    D[:, :, W - 3:] = (z[:, :, W - 3:] * 1.1).astype(f32)
    add("sign_zero", D, A, z, None, None, coef=np.array([[0.7, 0.3, 0.9]], f32))
    add("sign_zero_scaled", D * 2, A, z, rng.uniform(0.5, 1.5, (1, H, W)), np.array([0.5], f32),
        coef=np.array([[0.7, 0.3, 0.9]], f32))
    # no |r| and no |r_p - r_q| below 1e-3: the kink-free case of the autograd comparison
    H, W = 2 * th + 3, tw + 5
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r = 0.01 * (1 + (3 * x + 7 * y) % 11) - 0.055
    z = rng.uniform(1.0, 3.0, (2, H, W))
    A = rng.uniform(0.6, 1.0, (2, H, W)).astype(f32)
    w = rng.uniform(0.25, 2.0, (2, H, W)).astype(f32)
    z[1, 3:6, 10:20] = 0.0                 # a hole: pairs with one end missing
    s = np.array([1.25, 0.8], f32)
    D = ((z + r) / s.astype(f64)[:, None, None] * A).astype(f32)
    add("kink_free", D, A, z, w, s)
    return out


def case_args(c):
    return c["D"], c["A"], c["z"], c["w"], c["s"], c["alpha_min"]
