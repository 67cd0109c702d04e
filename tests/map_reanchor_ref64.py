"""numpy float64 restatement of the map re-anchor (include/s3a.h).

A pose row is lietorch's [t(3), q(x y z w), s] in float32: T(x) = s R(q/|q|) x + t.
`reanchor` returns float64 results that are NOT rounded to float32 (moved
rows), so a float32 implementation is compared against the exact value;
unmoved rows come back as the float32 inputs, cast.

`variant` drops one term for the sensitivity test:
  "no_s2"    the covariance is rotated but not scaled (M / s on Sigma)
  "no_RoT"   M = s R_n (the old rotation is not undone)
  "no_norm"  the quaternions are used as given, not normalised
`dtype=np.float32` evaluates the same composition in float32 (the tolerance's
yardstick).
"""
import numpy as np

KEEP, MOVE = 0, 1


def pose_valid(p):
    p = np.asarray(p, np.float32)
    q = p[3:7].astype(np.float64)
    return bool(np.all(np.isfinite(p)) and p[7] > 0 and np.sqrt(np.sum(q * q)) > 0)


def rotation(p, dtype=np.float64, normalise=True):
    q = np.asarray(p, np.float32)[3:7].astype(dtype)
    if normalise:
        q = q / np.sqrt(np.sum(q * q, dtype=dtype)).astype(dtype)
    x, y, z, w = q
    one, two = dtype(1), dtype(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]],
                    dtype)


def deltas(anchor, poses, variant=None, dtype=np.float64):
    """Per keyframe: flag (KEEP/MOVE), held, M [3,3], t_o, t_n, S (the matrix
    applied to Sigma), and the new anchor table."""
    anchor = np.asarray(anchor, np.float32)
    poses = np.asarray(poses, np.float32)
    n_kf = len(poses)
    flag = np.zeros(n_kf, np.int32)
    held = np.zeros(n_kf, bool)
    M = np.zeros((n_kf, 3, 3), dtype)
    S = np.zeros((n_kf, 3, 3), dtype)
    t_o = np.zeros((n_kf, 3), dtype)
    t_n = np.zeros((n_kf, 3), dtype)
    new_anchor = anchor.copy()
    for k in range(n_kf):
        a, p = anchor[k], poses[k]
        if not pose_valid(p):
            held[k] = True
            continue
        new_anchor[k] = p
        if a[7] == 0 or not pose_valid(a):
            continue
        if a.view(np.uint32).tolist() == p.view(np.uint32).tolist():
            continue
        norm = variant != "no_norm"
        Rn = rotation(p, dtype, norm)
        Ro = rotation(a, dtype, norm)
        s = dtype(p[7]) / dtype(a[7])
        R = Rn if variant == "no_RoT" else Rn @ Ro.T
        M[k] = s * R
        S[k] = R if variant == "no_s2" else M[k]
        t_o[k] = a[:3].astype(dtype)
        t_n[k] = p[:3].astype(dtype)
        flag[k] = MOVE
    return flag, held, M, t_o, t_n, S, new_anchor


def triu_to_full(c6):
    xx, xy, xz, yy, yz, zz = np.moveaxis(c6, -1, 0)
    return np.stack([np.stack([xx, xy, xz], -1), np.stack([xy, yy, yz], -1),
                     np.stack([xz, yz, zz], -1)], -2)


def full_to_triu(S):
    return np.stack([S[..., 0, 0], S[..., 0, 1], S[..., 0, 2], S[..., 1, 1], S[..., 1, 2],
                     S[..., 2, 2]], -1)


def reanchor(means, cov_triu, kf_id, n, anchor, poses, variant=None, dtype=np.float64):
    """-> dict(means [cap,3], cov [cap,6] (dtype), mask [cap] (moved rows),
    anchor [n_kf,8] float32, moved, held)."""
    means = np.asarray(means, np.float32)
    cov_triu = np.asarray(cov_triu, np.float32)
    kf_id = np.asarray(kf_id, np.int64)
    n_kf = len(poses)
    flag, held, M, t_o, t_n, S, new_anchor = deltas(anchor, poses, variant, dtype)
    live = np.arange(len(kf_id)) < n
    inr = live & (kf_id >= 0) & (kf_id < n_kf)
    mask = np.zeros(len(kf_id), bool)
    mask[inr] = flag[kf_id[inr]] == MOVE
    out_m = means.astype(dtype)
    out_c = cov_triu.astype(dtype)
    k = kf_id[mask]
    e = means[mask].astype(dtype) - t_o[k]
    out_m[mask] = t_n[k] + np.einsum("nij,nj->ni", M[k], e)
    Sig = triu_to_full(cov_triu[mask].astype(dtype))
    out_c[mask] = full_to_triu(np.einsum("nik,nkl,njl->nij", S[k], Sig, S[k]))
    return dict(means=out_m, cov=out_c, mask=mask, anchor=new_anchor, moved=int(mask.sum()),
                held=int(held.sum()), kf=kf_id, M=M, t_o=t_o, t_n=t_n, flag=flag)


def errors(got_means, got_cov, ref, want_means=None, want_cov=None):
    """The two metrics of the tolerance, over the moved rows of `ref`
    (float64 reanchor result): a mean's error relative to
    |M| |mu - t_o| + |t_n| (|M| the scale ratio), a covariance row's error
    relative to its largest output entry.  A zero denominator admits only a
    zero error (reported as 0, else inf).  want_*: measure the distance to
    these instead of to `ref` (the scales stay those of `ref`)."""
    mask = ref["mask"]
    if not mask.any():
        return 0.0, 0.0
    gm = np.asarray(got_means, np.float64)[mask]
    gc = np.asarray(got_cov, np.float64)[mask]
    rm, rc = ref["means"][mask], ref["cov"][mask]
    wm = rm if want_means is None else np.asarray(want_means, np.float64)[mask]
    wc = rc if want_cov is None else np.asarray(want_cov, np.float64)[mask]
    k = ref["kf"][mask]
    # M is a scaled rotation: |M| |mu - t_o| = |M (mu - t_o)| = |mu' - t_n|
    den_m = np.linalg.norm(rm - ref["t_n"][k], axis=1) + np.linalg.norm(ref["t_n"][k], axis=1)
    em = np.linalg.norm(gm - wm, axis=1)
    den_c = np.abs(rc).max(1)
    ec = np.abs(gc - wc).max(1)

    def ratio(e, d):
        r = np.where(d > 0, e / np.where(d > 0, d, 1.0), np.where(e == 0, 0.0, np.inf))
        return float(r.max())
    return ratio(em, den_m), ratio(ec, den_c)
