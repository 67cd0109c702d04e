"""Inputs, the float64 reference and the float32 host restatement for the
splat export / import tests (tests/test_splat_io.py).

  * inputs: numpy PCG64 seeds; random covariances R diag(s^2) R^T with
    s = exp(U(ln 1e-3, ln 0.5)) and uniformly random rotations, and the
    hand-built set of the degenerate and extreme cases;
  * float64 reference: numpy.linalg.eigvalsh of the float32 covariance and
    quaternion -> rotation in float64.  Eigenvectors are never compared (they
    are ill-conditioned near repeated eigenvalues): a row is judged by the
    covariance it reconstructs and by its eigenvalues;
  * float32 host restatement: torch.linalg.eigh on CPU float32 for the
    decomposition, numpy float32 for logit / sigmoid / log / exp.  Its error
    against the float64 reference is the floor the tolerances are taken from
    (tolerance = 4 x floor, rounded up to one significant digit).
"""
import numpy as np
import torch

C0 = 0.28209479177387814
SCALE_MIN = 1e-7
COLS = dict(xyz=slice(0, 3), normal=slice(3, 6), f_dc=slice(6, 9), opacity=9,
            scale=slice(10, 13), rot=slice(13, 17))
ROWS14 = [0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]   # import columns of a 17-row


def roundup_1sig(x):
    if x <= 0.0:
        return 0.0
    e = np.floor(np.log10(x))
    return float(np.ceil(x / 10 ** e - 1e-9) * 10 ** e)


def tolerance(floor):
    """The project's rule (test_raster_grad.py, test_loss_mask.py)."""
    return roundup_1sig(4.0 * floor)


def triu(S):
    S = np.asarray(S)
    return np.stack([S[..., 0, 0], S[..., 0, 1], S[..., 0, 2], S[..., 1, 1], S[..., 1, 2],
                     S[..., 2, 2]], -1)


def full(c6):
    c6 = np.asarray(c6)
    S = np.empty(c6.shape[:-1] + (3, 3), c6.dtype)
    S[..., 0, 0], S[..., 0, 1], S[..., 0, 2] = c6[..., 0], c6[..., 1], c6[..., 2]
    S[..., 1, 0], S[..., 1, 1], S[..., 1, 2] = c6[..., 1], c6[..., 3], c6[..., 4]
    S[..., 2, 0], S[..., 2, 1], S[..., 2, 2] = c6[..., 2], c6[..., 4], c6[..., 5]
    return S


def quat_to_R(q):
    """(w, x, y, z) -> rotation, in the dtype of q (the rasterizer's formula,
    raster_math.hpp); q is normalised first."""
    q = np.asarray(q)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3), q.dtype)
    R[..., 0, 0] = 1 - 2 * (y * y + z * z)
    R[..., 0, 1] = 2 * (x * y - w * z)
    R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z)
    R[..., 1, 1] = 1 - 2 * (x * x + z * z)
    R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y)
    R[..., 2, 1] = 2 * (y * z + w * x)
    R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    return quat_to_R(q)


def random_gaussians(n, seed):
    """means [n,3], cov_triu [n,6], colors [n,3], opacities [n], float32."""
    rng = np.random.default_rng(seed)
    s = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), size=(n, 3)))
    R = random_rotations(rng, n)
    S = np.einsum("nij,nj,nkj->nik", R, s * s, R)
    means = rng.normal(size=(n, 3)) * 2.0
    colors = rng.uniform(0.0, 1.0, size=(n, 3))
    op = rng.uniform(0.06, 1.0, size=n)
    # the clamp's two ends and a value far inside it
    op[::97] = 1.0
    op[5::97] = 0.0
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f(means), f(triu(S)), f(colors), f(op)


def hand_built():
    """name -> [3,3] float64 covariance, the degenerate and extreme cases."""
    rng = np.random.default_rng(20240)
    R = random_rotations(rng, 8)
    rot = lambda k, lam: R[k] @ np.diag(lam) @ R[k].T
    P = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])   # det -1
    u = R[3][:, 0]
    return {
        "isotropic": 0.04 * np.eye(3),
        "two_equal": rot(0, [0.09, 0.01, 0.01]),
        "two_equal_large": rot(1, [0.09, 0.09, 0.0004]),
        "diagonal_unsorted": np.diag([0.01, 0.25, 0.04]),
        "diagonal_tiny_offdiag": np.diag([0.01, 0.25, 0.04]) + 1e-30 * (1 - np.eye(3)),
        "zero": np.zeros((3, 3)),
        "rank1": 0.04 * np.outer(u, u),
        "rank2": rot(2, [0.09, 0.01, 0.0]),
        "anisotropy_1e8": rot(4, [1.0, 1e-3, 1e-8]),
        "entries_1e-12": 1e-12 * np.array([[2.0, 1.0, 0.9], [1.0, 2.1, 1.1], [0.9, 1.1, 1.9]]),
        "entries_1e+6": 1e6 * np.array([[2.0, 1.0, 0.9], [1.0, 2.1, 1.1], [0.9, 1.1, 1.9]]),
        "slightly_indefinite": rot(5, [0.25, 0.01, -1e-9 * 0.25]),
        "improper_permutation": P @ np.diag([0.01, 0.25, 0.04]) @ P.T,
        "improper_permutation_offdiag": P @ np.diag([0.01, 0.25, 0.04]) @ P.T
                                        + 1e-4 * (1 - np.eye(3)),
    }


def hand_built_inputs():
    names = list(hand_built())
    S = np.stack([hand_built()[k] for k in names])
    n = len(names)
    rng = np.random.default_rng(7)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return names, (f(rng.normal(size=(n, 3))), f(triu(S)), f(rng.uniform(size=(n, 3))),
                   f(rng.uniform(0.1, 0.9, size=n)))


# ------------------------------------------------- float32 host restatement
def _rot_to_quat32(V):
    """float32 rotation -> (w, x, y, z), w >= 0, branch on the largest of
    (trace, R00, R11, R22); numpy float32 throughout."""
    V = V.astype(np.float32)
    out = np.empty((len(V), 4), np.float32)
    one = np.float32(1.0)
    for i, R in enumerate(V):
        tr = R[0, 0] + R[1, 1] + R[2, 2]
        k = int(np.argmax([tr, R[0, 0], R[1, 1], R[2, 2]]))
        if k == 0:
            s = np.float32(2.0) * np.sqrt(max(one + tr, np.float32(0)))
            q = [s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
        elif k == 1:
            s = np.float32(2.0) * np.sqrt(max(one + R[0, 0] - R[1, 1] - R[2, 2], np.float32(0)))
            q = [(R[2, 1] - R[1, 2]) / s, s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
        elif k == 2:
            s = np.float32(2.0) * np.sqrt(max(one + R[1, 1] - R[0, 0] - R[2, 2], np.float32(0)))
            q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s]
        else:
            s = np.float32(2.0) * np.sqrt(max(one + R[2, 2] - R[0, 0] - R[1, 1], np.float32(0)))
            q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4]
        q = np.asarray(q, np.float32)
        q = q / np.sqrt(np.sum(q * q, dtype=np.float32))
        out[i] = -q if q[0] < 0 else q
    return out


def host32_rows(means, cov_triu, colors, opacities, scale_min=SCALE_MIN):
    """The export in float32 on the host: torch.linalg.eigh (CPU float32),
    numpy float32 elementwise maps.  [n, 17] float32."""
    n = len(means)
    rows = np.zeros((n, 17), np.float32)
    rows[:, COLS["xyz"]] = means
    rows[:, COLS["f_dc"]] = (colors.astype(np.float32) - np.float32(0.5)) / np.float32(C0)
    o = np.clip(opacities.astype(np.float32), np.float32(1e-6), np.float32(1.0) - np.float32(1e-6))
    rows[:, COLS["opacity"]] = np.log(o / (np.float32(1.0) - o))
    lam, V = torch.linalg.eigh(torch.from_numpy(full(cov_triu.astype(np.float32))))
    lam, V = lam.numpy()[:, ::-1].copy(), V.numpy()[:, :, ::-1].copy()       # descending
    flip = np.linalg.det(V.astype(np.float64)) < 0
    V[flip, :, 2] *= -1
    rows[:, COLS["scale"]] = np.log(np.maximum(np.sqrt(np.maximum(lam, np.float32(0))),
                                               np.float32(scale_min)))
    rows[:, COLS["rot"]] = _rot_to_quat32(V)
    zero = ~np.any(cov_triu != 0, axis=1)
    rows[zero, COLS["scale"]] = np.log(np.float32(scale_min))
    rows[zero, COLS["rot"]] = (1, 0, 0, 0)
    return rows


def host32_import(rows14):
    """The import in numpy float32: (means, cov_triu, colors, opacities)."""
    r = rows14.astype(np.float32)
    R = quat_to_R(r[:, 10:14])
    s2 = np.exp(r[:, 7:10]) ** 2
    S = np.einsum("nij,nj,nkj->nik", R, s2, R).astype(np.float32)
    col = np.clip(r[:, 3:6] * np.float32(C0) + np.float32(0.5), 0, 1)
    op = np.float32(1.0) / (np.float32(1.0) + np.exp(-r[:, 6]))
    return r[:, :3], triu(S), col, op


# ----------------------------------------------------- float64 judgement ----
def reconstruct64(rows):
    """R diag(exp(2 scale)) R^T in float64 from [n, 17] rows."""
    r = np.asarray(rows, np.float64)
    R = quat_to_R(r[:, COLS["rot"]])
    return np.einsum("nij,nj,nkj->nik", R, np.exp(2.0 * r[:, COLS["scale"]]), R)


def export_errors(cov_triu, rows, scale_min=SCALE_MIN):
    """Per-Gaussian errors of export rows against float64:
      recon  ||R diag(exp(2 s)) R^T - Sigma||_F / ||Sigma||_F (nan for Sigma = 0)
      eig    max_i |exp(2 s_i) - max(lambda_i, scale_min^2)| / lambda_max (nan for Sigma = 0)
      qnorm  | |q| - 1 |"""
    S = full(np.asarray(cov_triu, np.float64))
    r = np.asarray(rows, np.float64)
    lam = np.linalg.eigvalsh(S)[:, ::-1]
    nS = np.linalg.norm(S, axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        recon = np.linalg.norm(reconstruct64(rows) - S, axis=(1, 2)) / nS
        eig = np.max(np.abs(np.exp(2.0 * r[:, COLS["scale"]])
                            - np.maximum(lam, scale_min ** 2)), axis=1) / lam[:, 0]
    zero = nS == 0
    recon[zero], eig[zero] = np.nan, np.nan
    qnorm = np.abs(np.linalg.norm(r[:, COLS["rot"]], axis=1) - 1.0)
    return dict(recon=recon, eig=eig, qnorm=qnorm)


def attribute_errors(colors, opacities, rows):
    """Absolute error of the colour and the (clamped) opacity that the rows'
    f_dc and opacity invert to, in float64."""
    r = np.asarray(rows, np.float64)
    col = r[:, COLS["f_dc"]] * C0 + 0.5
    op = 1.0 / (1.0 + np.exp(-r[:, COLS["opacity"]]))
    o_ref = np.clip(np.asarray(opacities, np.float64), 1e-6, 1 - 1e-6)
    return dict(color=np.abs(col - np.asarray(colors, np.float64)).max(axis=1),
                opacity=np.abs(op - o_ref))


def structure_ok(rows):
    """w >= 0, scales non-increasing, every output finite, normals zero."""
    r = np.asarray(rows)
    s = r[:, COLS["scale"]]
    return (bool(np.all(np.isfinite(r))) and bool(np.all(r[:, 13] >= 0))
            and bool(np.all(s[:, 0] >= s[:, 1])) and bool(np.all(s[:, 1] >= s[:, 2]))
            and bool(np.all(r[:, COLS["normal"]] == 0)))


def import_errors(ref, got):
    """(means, cov_triu, colors, opacities) pairs -> max errors: cov relative
    Frobenius per Gaussian, colours and opacities absolute."""
    S0, S1 = full(np.asarray(ref[1], np.float64)), full(np.asarray(got[1], np.float64))
    return dict(cov=float(np.max(np.linalg.norm(S1 - S0, axis=(1, 2))
                                 / np.linalg.norm(S0, axis=(1, 2)))),
                color=float(np.abs(np.asarray(got[2], np.float64) - ref[2]).max()),
                opacity=float(np.abs(np.asarray(got[3], np.float64).reshape(-1)
                                     - np.clip(ref[3], 1e-6, 1 - 1e-6)).max()))
