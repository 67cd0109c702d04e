"""ORACLE — test infrastructure only.  The cases of tests/golden/ref_kernels.npz:
inputs for the reference's per-thread kernels (refine_matches, iter_proj,
Sim3 / pose_retr), chosen at the edges where a restatement goes wrong, and
the recipe that turns inputs into outputs with the reference library
(oracle.ref_lib()).

  make_inputs()      -> dict of numeric arrays (deterministic)
  reference_outputs(fx) -> dict of the library's outputs for those inputs
  refine_cases(fx) / iter_cases(fx) -> iterate a fixture's cases

gen_golden.py's `ref_kernels` section writes inputs + outputs; the freshness
test recomputes reference_outputs() from the stored inputs.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
EPS32 = F32(1e-6)          # the float nearest the reference's EPS (a double 1e-6); it lies below it

# --------------------------------------------------------- refine_matches --
# name: (b, h, w, f, n, radius, dilation_max, kind)
REFINE_CASES = {
    "ties_b2":   (2, 24, 32, 24, 1030, 3, 5, "ties"),    # b n >= 2048: the binned orders run
    "ties_r2d3": (1, 13, 19, 24, 247, 2, 3, "ties"),
    "ties_f32":  (1, 13, 19, 32, 247, 1, 2, "ties"),
    "ties_r4d2": (1, 13, 19, 24, 101, 4, 2, "ties"),
    "ties_f16":  (1, 13, 19, 16, 247, 3, 1, "ties"),
    "ties_f8":   (1, 13, 19, 8, 247, 3, 5, "ties"),
    "low":       (1, 13, 19, 24, 247, 3, 5, "low"),
    "neg":       (1, 13, 19, 24, 247, 3, 5, "neg"),
    "big":       (1, 13, 19, 16, 247, 3, 5, "big"),
    "edges":     (1, 24, 32, 24, 37, 3, 5, "edges"),
    "float":     (1, 13, 19, 8, 101, 3, 5, "float"),     # fp32 descriptors: reference library only
}


def _unit(rng, shape):
    d = rng.normal(size=shape)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _starts(rng, b, n, h, w, m=3):
    return np.stack([rng.integers(-m, w + m, size=(b, n)),
                     rng.integers(-m, h + m, size=(b, n))], -1).astype(np.int64)


def _refine_inputs(name, seed):
    b, h, w, f, n, radius, dil, kind = REFINE_CASES[name]
    rng = np.random.default_rng(seed)
    p1 = _starts(rng, b, n, h, w)
    dt = np.float16
    if kind == "ties":
        # multiples of 1/4: every product and partial sum is exact in fp16, equal scores abound
        lo = -1 if b > 1 else -2          # three levels in the large case (fixture size)
        D11 = rng.integers(lo, -lo + 1, size=(b, h, w, f)) * 0.25
        D21 = rng.integers(lo, -lo + 1, size=(b, n, f)) * 0.25
    elif kind == "low":
        # score ~ 3e-4 (alpha + noise): straddles 0 and the fp16 smallest normal 6.1e-5; the
        # products (~1e-5) and partial sums are fp16 subnormals.  alpha < 0: every candidate
        # scores below 0 and the query stays; alpha > 0: it moves
        e = np.ones(f) / np.sqrt(f)
        s = np.sqrt(3e-4)
        alpha = rng.uniform(-1.0, 1.0, size=(b, n, 1))
        D11 = (e + 0.1 * _unit(rng, (b, h, w, f))) * s
        D21 = (alpha * e + 0.1 * np.abs(alpha) * _unit(rng, (b, n, f))) * s
    elif kind == "neg":
        D11 = np.round(np.abs(_unit(rng, (b, h, w, f))) * 32 + 1) / 32
        D21 = -np.round(np.abs(_unit(rng, (b, n, f))) * 32 + 1) / 32
    elif kind == "big":
        # products up to 1600, partial sums in the thousands (fp16 spacing 1-4), |sum| <= 25600
        D11 = rng.integers(-40, 41, size=(b, h, w, f))
        D21 = rng.integers(-40, 41, size=(b, n, f))
    elif kind == "edges":
        D11 = np.round(_unit(rng, (b, h, w, f)) * 8) / 8
        D21 = np.round(_unit(rng, (b, n, f)) * 8) / 8
        fixed = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1),             # corners
                 (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2),  # edges
                 (-3, -3), (w + 2, h + 2), (-3, h // 2), (w // 2, h + 2)]     # off the image
        p1[0, :len(fixed)] = fixed
    elif kind == "float":
        dt = np.float32
        D11 = np.round(_unit(rng, (b, h, w, f)) * 256) / 256
        D21 = np.round(_unit(rng, (b, n, f)) * 256) / 256
    return dict(D11=D11.astype(dt), D21=D21.astype(dt), p1=p1,
                rd=np.int64([radius, dil]))


def refine_cases(fx):
    """(name, D11, D21, p1, radius, dilation_max, expected or None)"""
    for name in REFINE_CASES:
        pre = f"rf_{name}_"
        r, d = (int(v) for v in fx[pre + "rd"])
        yield (name, fx[pre + "D11"], fx[pre + "D21"], fx[pre + "p1"], r, d,
               fx[pre + "out"] if pre + "out" in fx else None)


# -------------------------------------------------------------- iter_proj --
LAMBDA_INIT, COST_THRESH = 1e-8, 1e-6           # config/base.yaml:8-14
# name: (image, max_iters); image "a" = 12 x 16, b = 2 (patched); "b" = 24 x 32, b = 1
ITER_CASES = {
    "a_outside": ("a", (10,)),
    "a_integer": ("a", (0, 1, 10)),
    "a_patches": ("a", (1, 10)),
    "b_smooth":  ("b", (10,)),
}
ZERO_RAY = (0, slice(4, 8), slice(5, 9))        # image a: batch 0, rows, cols: all 9 channels 0
ZERO_GRAD = (1, slice(3, 8), slice(2, 7))       # batch 1: gx = gy = 0 exactly
TINY_GRAD = (1, slice(3, 8), slice(9, 14))      # batch 1: gradients x 1e-5 (huge, clamped steps)


def _pointmap(b, h, w, rng, z=2.0):
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    f = max(h, w)
    x, y = (u - w / 2) / f, (v - h / 2) / f
    out = []
    for _ in range(b):
        a = rng.normal(size=3) * 0.2
        depth = z + a[0] * np.sin(3 * x) + a[1] * np.cos(2 * y) + a[2] * x * y
        out.append(np.stack([x * depth, y * depth, depth], -1))
    return np.stack(out).astype(F32)


def _iter_inputs():
    import oracle
    out = {}
    rng = np.random.default_rng(500)
    # image a
    b, h, w = 2, 12, 16
    X11 = _pointmap(b, h, w, rng)
    X21 = np.roll(X11, (1, -2), axis=(1, 2)) + rng.normal(size=X11.shape).astype(F32) * 1e-3
    rays, pts_grid, _ = oracle.prep_iter_proj(X11, X21)
    rays[ZERO_RAY] = 0.0
    rays[ZERO_GRAD][..., 3:] = 0.0
    rays[TINY_GRAD][..., 3:] *= F32(1e-5)
    out["ip_rays_a"] = rays

    def pts_for(n):
        idx = rng.integers(0, h * w, size=(b, n))
        return np.take_along_axis(pts_grid, idx[..., None], 1)

    n = 150
    p = np.stack([rng.uniform(-5, w + 5, (b, n)), rng.uniform(-5, h + 5, (b, n))], -1)
    p[:, 0] = (-3.5, 5.2)          # left
    p[:, 1] = (w + 2.5, 5.2)       # right
    p[:, 2] = (6.3, -4.0)          # above
    p[:, 3] = (6.3, h + 7.0)       # below
    p[:, 4] = (-1e6, 1e6)
    out["ip_a_outside_pinit"], out["ip_a_outside_pts"] = p.astype(F32), pts_for(n)

    n = 77
    p = np.stack([rng.integers(0, w, (b, n)), rng.integers(0, h, (b, n))], -1).astype(F32)
    p[:, 0] = (1, 1)
    p[:, 1] = (w - 2, h - 2)
    p[:, 2] = (1, h - 2)
    p[:, 3] = (w - 2, 1)
    p[:, 4] = (0, 0)
    p[:, 5] = (w - 1, h - 1)
    p[:, 6] = (np.nextafter(F32(5), F32(0)), np.nextafter(F32(6), F32(0)))   # a float below an integer
    p[:, 7] = (np.nextafter(F32(w - 2), F32(0)), np.nextafter(F32(1), F32(2)))
    p[:, 8] = (np.nextafter(F32(w - 2), F32(w)), np.nextafter(F32(1), F32(0)))
    out["ip_a_integer_pinit"], out["ip_a_integer_pts"] = p, pts_for(n)

    n = 60
    p = np.zeros((b, n, 2))
    # batch 0: in and around the zero-ray patch; batch 1: the zero / tiny gradient patches
    p[0] = np.stack([rng.uniform(3.5, 10.5, n), rng.uniform(2.5, 9.5, n)], -1)
    p[1, :30] = np.stack([rng.uniform(1.5, 7.5, 30), rng.uniform(2.5, 8.5, 30)], -1)
    p[1, 30:] = np.stack([rng.uniform(8.5, 14.0, 30), rng.uniform(2.5, 8.5, 30)], -1)
    out["ip_a_patches_pinit"], out["ip_a_patches_pts"] = p.astype(F32), pts_for(n)

    # image b: a smooth surface, a planted shift, points on the pixel grid
    b, h, w = 1, 24, 32
    X11 = _pointmap(b, h, w, rng)
    X21 = np.roll(X11, (2, -3), axis=(1, 2)) + rng.normal(size=X11.shape).astype(F32) * 2e-3
    rays, pts, p_init = oracle.prep_iter_proj(X11, X21)
    out["ip_rays_b"] = rays
    keep = np.sort(rng.permutation(h * w)[:509])         # 509 of the 768 pixels (fixture size)
    out["ip_b_smooth_pinit"], out["ip_b_smooth_pts"] = p_init[:, keep], pts[:, keep]
    for name, (_, iters) in ITER_CASES.items():
        out[f"ip_{name}_iters"] = np.int64(iters)
    return out


def iter_cases(fx):
    """(name, rays, pts, p_init, max_iters, expected p [k,b,n,2] or None,
    expected converged [k,b,n] or None)"""
    for name, (img, _) in ITER_CASES.items():
        pre = f"ip_{name}_"
        yield (name, fx["ip_rays_" + img], fx[pre + "pts"], fx[pre + "pinit"],
               [int(i) for i in fx[pre + "iters"]],
               fx[pre + "p"] if pre + "p" in fx else None,
               fx[pre + "conv"] if pre + "conv" in fx else None)


# ------------------------------------------------------------------- Sim3 --
REGIMES = ("zero", "theta_tiny", "sigma_tiny", "generic", "theta_1e-6_1e-3", "theta_1e-3_0.1",
           "sigma_1e-6_1e-2", "thr_theta_sq", "thr_theta", "thr_sigma")
ROWS = 144                  # per regime (the threshold regimes hold what the search finds)
POOL = 64                   # poses: row i of the tangent table acts on pose i % POOL


def rand_sim3(n, rng, tscale=1.0):
    t = rng.normal(size=(n, 3)) * tscale
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    s = np.exp(rng.normal(size=(n, 1)) * 0.3)
    return np.concatenate([t, q, s], 1).astype(F32)


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _theta_sq32(phi):
    phi = phi.astype(F32)
    return phi[:, 0] * phi[:, 0] + phi[:, 1] * phi[:, 1] + phi[:, 2] * phi[:, 2]


def _steps(x, k):
    """the 2k+1 floats around x"""
    lo = hi = F32(x)
    out = [F32(x)]
    for _ in range(k):
        lo = np.nextafter(lo, F32(-np.inf))
        hi = np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return np.sort(np.array(out, F32))


def _sim3_inputs():
    rng = np.random.default_rng(900)
    rows, regime = [], []

    def add(rid, tau_phi_sigma):
        rows.append(tau_phi_sigma)
        regime.append(np.full(len(tau_phi_sigma), rid, np.int8))

    def table(theta, sigma):
        n = len(theta)
        tau = np.round(rng.normal(size=(n, 3)) * 64) / 64      # exact in fp32
        phi = _unit(rng, (n, 3)) * np.asarray(theta)[:, None]
        return np.concatenate([tau, phi, np.asarray(sigma)[:, None]], 1).astype(F32)

    sgn = lambda n: rng.choice([-1.0, 1.0], n)
    gen_theta = lambda n: rng.uniform(0.1, 3.0, n)
    gen_sigma = lambda n: rng.uniform(0.05, 1.0, n) * sgn(n)
    R = ROWS
    add(0, table(np.zeros(R), np.zeros(R)))
    add(1, table(_logu(rng, 1e-12, 9e-7, R), gen_sigma(R)))
    add(2, table(gen_theta(R), _logu(rng, 1e-12, 9e-7, R) * sgn(R)))
    add(3, table(gen_theta(R), gen_sigma(R)))
    add(4, table(_logu(rng, 1.1e-6, 9e-4, R), gen_sigma(R)))
    add(5, table(_logu(rng, 1e-3, 0.1, R), gen_sigma(R)))
    add(6, table(gen_theta(R), _logu(rng, 1.1e-6, 1e-2, R) * sgn(R)))

    # theta_sq (fp32, summed as expSO3 does) on the floats around EPS32, the last float below the
    # reference's double EPS: search directions scaled to norm ~1e-3
    want = {float(v): [] for v in _steps(EPS32, 2)}
    cand = _unit(rng, (200000, 3)) * rng.uniform(0.9999995e-3, 1.0000005e-3, (200000, 1))
    cand = cand.astype(F32)
    for row, tsq in zip(cand, _theta_sq32(cand)):
        got = want.get(float(tsq))
        if got is not None and len(got) < 6:
            got.append(row)
    assert all(len(v) >= 2 for v in want.values()), {k: len(v) for k, v in want.items()}
    phi = np.concatenate([np.stack(v) for v in want.values()])
    t = table(np.ones(len(phi)), np.where(np.arange(len(phi)) % 2 == 0, gen_sigma(len(phi)), 3e-7))
    t[:, 3:6] = phi
    add(7, t)

    # theta = sqrtf(theta_sq) on the floats around EPS32: phi along one axis
    vals = _steps(EPS32, 3)
    phi = []
    for k, v in enumerate(vals):
        for s in (1.0, -1.0):
            p = np.zeros(3, F32)
            p[k % 3] = F32(s) * v
            phi.append(p)
    phi = np.stack(phi)
    t = table(np.ones(len(phi)), np.where(np.arange(len(phi)) % 4 < 2, gen_sigma(len(phi)), -2e-7))
    t[:, 3:6] = phi
    add(8, t)

    # |sigma| on the floats around EPS32, generic and tiny theta
    vals = np.concatenate([_steps(EPS32, 3), -_steps(EPS32, 3)])
    sig = np.repeat(vals, 2)
    th = np.where(np.arange(len(sig)) % 2 == 0, gen_theta(len(sig)), 4e-7)
    t = table(th, np.zeros(len(sig)))
    t[:, 6] = sig
    add(9, t)

    pool = rand_sim3(POOL, rng)
    pool[POOL - 2, 7], pool[POOL - 1, 7] = 0.05, 20.0
    out = dict(s3_xi=np.concatenate(rows), s3_regime=np.concatenate(regime), s3_pool=pool)

    # group operations that do not depend on a tangent
    n = 64
    T, U = rand_sim3(n, rng), rand_sim3(n, rng)
    T[:4, 7], U[:4, 7] = (0.05, 20.0, 0.05, 20.0), (20.0, 0.05, 0.05, 20.0)
    out.update(g_T=T, g_U=U, g_X=(rng.normal(size=(n, 3)) * 3).astype(F32),
               g_X7=rng.normal(size=(n, 7)).astype(F32),
               g_r=np.concatenate([rng.normal(size=n - 6) * 2, _steps(F32(1.345), 1),
                                   -_steps(F32(1.345), 1)]).astype(F32))
    # pose_retr: in place, the first num_fix poses pinned
    out.update(pr_poses=rand_sim3(37, rng), pr_fix=np.int64([1, 3]),
               pr_dx=np.concatenate([rng.normal(size=(30, 7)) * 0.1, out["s3_xi"][::97][:6]]
                                    ).astype(F32))
    return out


def sim3_T(fx):
    """the pose each tangent row of s3_xi is retracted onto"""
    return fx["s3_pool"][np.arange(len(fx["s3_xi"])) % len(fx["s3_pool"])]


IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1, 1], F32)


# ---------------------------------------------------------------- fixture --
def make_inputs():
    out = {}
    for k, name in enumerate(REFINE_CASES):
        for key, v in _refine_inputs(name, 100 + k).items():
            out[f"rf_{name}_{key}"] = v
    out.update(_iter_inputs())
    out.update(_sim3_inputs())
    return out


def reference_outputs(fx):
    """Every output of the fixture, recomputed with the reference library."""
    import oracle
    out = {}
    for name, D11, D21, p1, r, d, _ in refine_cases(fx):
        out[f"rf_{name}_out"] = oracle.ref_refine_matches(D11, D21, p1, r, d)
    for name, rays, pts, p_init, iters, _, _ in iter_cases(fx):
        res = [oracle.ref_iter_proj(rays, pts, p_init, it, LAMBDA_INIT, COST_THRESH)
               for it in iters]
        out[f"ip_{name}_p"] = np.stack([p for p, _ in res])
        out[f"ip_{name}_conv"] = np.stack([c for _, c in res])
    out["s3_exp"] = oracle.ref_sim3_exp(fx["s3_xi"])
    out["s3_retr"] = oracle.ref_sim3_retr(sim3_T(fx), fx["s3_xi"])
    T, U = fx["g_T"], fx["g_U"]
    out["g_act"] = oracle.ref_sim3_act(T, fx["g_X"])
    out["g_act1"] = oracle.ref_sim3_act(T[5:6], fx["g_X"])          # one pose, broadcast
    out["g_mul_raw"] = oracle.ref_sim3_mul(T, U)
    out["g_rel"] = oracle.ref_sim3_rel(T, U)
    out["g_inv"] = oracle.ref_sim3_rel(T, np.tile(IDENTITY, (len(T), 1)))
    out["g_adj"] = oracle.ref_sim3_adj_inv(T, fx["g_X7"])
    out["g_huber"] = oracle.ref_huber(fx["g_r"])
    for nf in fx["pr_fix"]:
        nf = int(nf)
        dx = fx["pr_dx"][:len(fx["pr_poses"]) - nf]
        out[f"pr_out_fix{nf}"] = oracle.ref_pose_retr(fx["pr_poses"], dx, nf)
    return out
