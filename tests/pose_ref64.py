"""Float64 reference of the pose gradient and the pose step (include/s3x.h),
for tests/test_pose_grad.py.  numpy, vectorised over the rows; it shares no
code with csrc/pose_grad_math.hpp.

The identity: the rasterizer's forward (SH degree 0 or colors_precomp) sees
the camera and the Gaussians only through view-space quantities, so the camera
move T_WC <- T_WC Exp(xi), xi = (rho, phi), is the move of every Gaussian by
Exp(-xi) in view space.  With A = vm[:3,:3]^T, b = vm[3,:3], t = A mu + b and
g = A^-T dL/dmu:
  dL/drho = -sum g,   dL/dphi = -sum (t x g + c)
  c = 2 axial(G_v S_v - S_v G_v), S_v = A S A^T, G_v = A^-T G A^-1   (covariance)
  c = R^T w, R the rotation of the camera-to-world block,
      w_k = 1/2 dL/dq . (e_k (x) q)                                 (unit quaternion)

`ablate` (sensitivity tests): "cov_term" drops c, "A_for_Ait" uses A where
A^-T belongs, "twist_side" is the gradient of T_WC <- Exp(xi) T_WC instead.
"""
import numpy as np

ABLATIONS = ("cov_term", "A_for_Ait", "twist_side")


def hat(w):
    x, y, z = w
    return np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])


def se3_exp(xi):
    """Exp of the twist (rho, phi) as a 4 x 4 matrix: the power series of the
    matrix exponential, summed in extended precision (no closed form, so the
    closed forms under test are checked against something else)."""
    M = np.zeros((4, 4), np.longdouble)
    M[:3, :3] = hat(np.asarray(xi[3:], np.float64))
    M[:3, 3] = np.asarray(xi[:3], np.float64)
    out = np.eye(4, dtype=np.longdouble)
    term = np.eye(4, dtype=np.longdouble)
    for k in range(1, 80):
        term = term @ M / np.longdouble(k)
        out = out + term
    return out.astype(np.float64)


def view_parts(vm):
    vm = np.asarray(vm, np.float64).reshape(4, 4)
    return vm[:3, :3].T.copy(), vm[3, :3].copy()


def _quat_left_imag(q):
    """[n, 3, 4]: row k is the quaternion e_k (x) q, (r, x, y, z) order."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    ex = np.stack([-x, r, -z, y], -1)       # i q
    ey = np.stack([-y, z, r, -x], -1)       # j q
    ez = np.stack([-z, -y, x, r], -1)       # k q
    return np.stack([ex, ey, ez], 1)


def contributions(vm, means3D, d_means3D, cov3D=None, d_cov3D=None, rotations=None,
                  d_rotations=None, ablate=()):
    """[n, 6] float64: every row's term of (dL/drho, dL/dphi), sign included."""
    assert (cov3D is None) != (rotations is None)
    for a in ablate:
        assert a in ABLATIONS, a
    A, b = view_parts(vm)
    if "twist_side" in ablate:      # a world-frame twist: the camera frame is the world's
        A, b = np.eye(3), np.zeros(3)
    Ait = np.linalg.inv(A).T
    mu = np.asarray(means3D, np.float64).reshape(-1, 3)
    dmu = np.asarray(d_means3D, np.float64).reshape(-1, 3)
    t = mu @ A.T + b
    g = dmu @ (A.T if "A_for_Ait" in ablate else Ait.T)
    phi = np.cross(t, g)
    if "cov_term" in ablate:
        pass
    elif cov3D is not None:
        c6 = np.asarray(cov3D, np.float64).reshape(-1, 6)
        d6 = np.asarray(d_cov3D, np.float64).reshape(-1, 6)
        ix = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
        S = c6[:, ix]
        G = d6[:, ix] * np.array([[1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 1.0]])
        Sv = A @ S @ A.T
        Gi = A if "A_for_Ait" in ablate else Ait
        Gv = Gi @ G @ Gi.T
        X = Gv @ Sv - Sv @ Gv
        phi = phi + 2.0 * np.stack([X[:, 2, 1], X[:, 0, 2], X[:, 1, 0]], -1)
    else:
        q = np.asarray(rotations, np.float64).reshape(-1, 4)
        dq = np.asarray(d_rotations, np.float64).reshape(-1, 4)
        w = 0.5 * np.einsum("nkj,nj->nk", _quat_left_imag(q), dq)
        # A = R^T / s for the camera-to-world block s R, so R^T = A / cbrt(det A)
        # (the definition include/s3x.h gives for an A that is a scaled
        # rotation only to float32 rounding); c = R^T w
        Rt = A / np.cbrt(np.linalg.det(A))
        phi = phi + w @ Rt.T
    return -np.concatenate([g, phi], 1)


def pose_gradient(vm, means3D, d_means3D, cov3D=None, d_cov3D=None, rotations=None,
                  d_rotations=None, radii=None, ablate=()):
    """(grad [6], abs_sum [6], skipped): the sum of the rows' contributions,
    the sum of their magnitudes (the scale of the rounding bound) and the
    number of visible rows left out because an input is not finite."""
    shape, d_shape = (cov3D, d_cov3D) if cov3D is not None else (rotations, d_rotations)
    n = len(np.asarray(means3D).reshape(-1, 3))
    keep = np.ones(n, bool) if radii is None else np.asarray(radii).reshape(-1) > 0
    rows = [np.asarray(a, np.float64).reshape(n, -1) for a in (means3D, d_means3D, shape, d_shape)]
    fin = np.all([np.isfinite(a).all(1) for a in rows], 0)
    skipped = int((keep & ~fin).sum())
    use = keep & fin
    rows = [a[use] for a in rows]
    kw = dict(cov3D=rows[2], d_cov3D=rows[3]) if cov3D is not None else \
        dict(rotations=rows[2], d_rotations=rows[3])
    c = contributions(vm, rows[0], rows[1], ablate=ablate, **kw)
    return c.sum(0), np.abs(c).sum(0), skipped


# ------------------------------------------------------- camera perturbation
def ext_of_view(vm):
    """Camera-to-world 4 x 4 of a (row-vector) view matrix."""
    return np.linalg.inv(np.asarray(vm, np.float64).reshape(4, 4).T)


def perturbed_settings(sd, xi, left=False):
    """The settings dict of the camera T_WC Exp(xi) (left: Exp(xi) T_WC): view
    matrix, full projection (the projection factor inv(vm) @ projmatrix is
    kept) and campos, float64."""
    vm = np.asarray(sd["viewmatrix"], np.float64).reshape(4, 4)
    pm = np.asarray(sd["projmatrix"], np.float64).reshape(4, 4)
    proj = np.linalg.solve(vm, pm)
    ext = ext_of_view(vm)
    ext = se3_exp(xi) @ ext if left else ext @ se3_exp(xi)
    vm2 = np.linalg.inv(ext).T
    out = dict(sd)
    out.update(viewmatrix=vm2.ravel(), projmatrix=(vm2 @ proj).ravel(), campos=ext[:3, 3].copy())
    return out


def scaled_camera(sd, s):
    """The settings of the camera whose camera-to-world block is s R instead
    of R (same centre), and the map from a Gaussian seen by the first camera
    to the one the second sees at the same view-space place:
    returns (settings, move) with move(means3D) -> means3D', covariances and
    scales growing by s^2 and s."""
    vm = np.asarray(sd["viewmatrix"], np.float64).reshape(4, 4)
    pm = np.asarray(sd["projmatrix"], np.float64).reshape(4, 4)
    proj = np.linalg.solve(vm, pm)
    ext = ext_of_view(vm)
    ext2 = ext.copy()
    ext2[:3, :3] *= s
    vm2 = np.linalg.inv(ext2).T
    out = dict(sd)
    out.update(viewmatrix=vm2.ravel(), projmatrix=(vm2 @ proj).ravel(), campos=ext2[:3, 3].copy())
    A, b = view_parts(vm)
    A2, b2 = view_parts(vm2)

    def move(means3D):
        t = np.asarray(means3D, np.float64) @ A.T + b
        return np.linalg.solve(A2, (t - b2).T).T
    return out, move


# ------------------------------------------------------------- the pose step
def adam_biases(betas, t):
    return 1.0 - betas[0] ** t, np.sqrt(1.0 - betas[1] ** t)


def pose_step(T, m, v, grad, t, lr_translation, lr_rotation, betas, eps, render_scale):
    """One step of s3x_pose_step in float64: returns (T, m, v), unchanged
    copies when the gradient is not finite."""
    T, m, v = np.array(T, np.float64), np.array(m, np.float64), np.array(v, np.float64)
    grad = np.asarray(grad, np.float64)
    if not np.isfinite(grad).all():
        return T, m, v
    g = grad * np.array([render_scale] * 3 + [1.0] * 3)
    lr = np.array([lr_translation] * 3 + [lr_rotation] * 3)
    b1, b2s = adam_biases(betas, t)
    m = betas[0] * m + (1.0 - betas[0]) * g
    v = betas[1] * v + (1.0 - betas[1]) * g * g
    delta = (lr / b1) * m / (np.sqrt(v) / b2s + eps)
    return T @ se3_exp(-delta), m, v


def camera(T, render_scale, proj_t):
    """(viewmatrix [4,4], projmatrix [4,4], campos [3]) in float64 of the pose
    T, as render.camera_settings forms them."""
    T = np.array(T, np.float64)
    ts = render_scale * T[:3, 3]
    Bi = np.linalg.inv(T[:3, :3])
    view = np.zeros((4, 4))             # (ext^-1)^T, ext^-1 = (B^-1 | -B^-1 ts)
    view[:3, :3] = Bi.T
    view[3, :3] = -Bi @ ts
    view[3, 3] = 1.0
    return view, view @ np.asarray(proj_t, np.float64).reshape(4, 4), ts


# -------------------------------------------- rigid move of the Gaussians --
def rigid_move_vjp(vm, means3D, d_means3D, cov3D=None, d_cov3D=None, rotations=None,
                   d_rotations=None):
    """dL/dxi at 0 by torch autograd (float64) through the move itself: the
    Gaussians as functions of xi, mu(xi) = A^-1 (Exp(-xi) (A mu + b) - b) with
    torch.matrix_exp, their covariances A^-1 Rd A S (A^-1 Rd A)^T or their
    quaternions dq(xi) (x) q, contracted with the given gradients.  None of
    the closed forms above enters."""
    import torch
    dt = torch.float64
    A, b = (torch.from_numpy(x) for x in view_parts(vm))
    xi = torch.zeros(6, dtype=dt, requires_grad=True)
    gen = torch.zeros(6, 4, 4, dtype=dt)
    for k in range(3):
        gen[k, k, 3] = 1.0
        gen[3 + k, :3, :3] = torch.from_numpy(hat(np.eye(3)[k]))
    E = torch.matrix_exp(-(xi[:, None, None] * gen).sum(0))
    Ai = torch.linalg.inv(A)
    mu = torch.as_tensor(np.asarray(means3D, np.float64)).reshape(-1, 3)
    t = mu @ A.T + b
    t2 = t @ E[:3, :3].T + E[:3, 3]
    L = ((t2 - b) @ Ai.T * torch.as_tensor(np.asarray(d_means3D, np.float64)).reshape(-1, 3)).sum()
    Rw = Ai @ E[:3, :3] @ A                 # the world rotation of every Gaussian
    if cov3D is not None:
        c6 = torch.as_tensor(np.asarray(cov3D, np.float64)).reshape(-1, 6)
        ix = torch.tensor([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
        S2 = Rw @ c6[:, ix] @ Rw.T
        iu = torch.triu_indices(3, 3)
        L = L + (S2[:, iu[0], iu[1]] * torch.as_tensor(np.asarray(d_cov3D, np.float64))
                 .reshape(-1, 6)).sum()
    else:
        # the unit quaternion of Rw: to first order (1, v / 2), v the axial part
        v = 0.5 * torch.stack([Rw[2, 1] - Rw[1, 2], Rw[0, 2] - Rw[2, 0], Rw[1, 0] - Rw[0, 1]])
        q = torch.as_tensor(np.asarray(rotations, np.float64)).reshape(-1, 4)
        r, qv = q[:, :1], q[:, 1:]
        hv = 0.5 * v[None]
        q2 = torch.cat([r - (hv * qv).sum(1, keepdim=True),
                        qv + r * hv + torch.cross(hv.expand_as(qv), qv, dim=1)], 1)
        L = L + (q2 * torch.as_tensor(np.asarray(d_rotations, np.float64)).reshape(-1, 4)).sum()
    L.backward()
    return xi.grad.numpy()
