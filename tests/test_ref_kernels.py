"""The matching kernels (iter_proj, refine_matches) and the Sim3 / pose_retr
math against the reference's OWN kernel text.

tests/golden/ref_kernels.npz holds inputs (oracle/ref_cases.py) and the outputs
that the reference's per-thread kernels gave for them, compiled for the host
from the reference tree by oracle/ref_build.py (the text itself is never
committed).  Three layers are held to those outputs:

  * the CPU restatements oracle/matching_ref.c, oracle/sim3_ref.c and the
    s3lie_*_host helpers: bit for bit;
  * the HIP kernels: refine_matches (every kernel variant), iter_proj, Sim3
    act / mul / inv bit for bit; exp / retr / pose_retr within a bound;
  * the fixture itself: recomputed with the library where it is built
    (test_fixture_is_fresh, the only test here that may skip).

"Bit for bit" is value equality of every element (NaN equal to NaN, -0 equal
to +0).  The reference has no group product or inverse of its own: `mul` is
its actSim3 + quat_comp followed by lietorch's quaternion normalisation
(oracle.lietorch_normalize), `inv` is its relSim3 against the identity.

Bound for HIP exp / retr / pose_retr (device sinf / cosf / expf are not
glibc's): per regime, E = max |reference fp32 - exact| with the exact Sim3
exponential and retraction evaluated in float64 (W = sum_n (sigma I +
[phi]x)^n / (n+1)!, 40 terms: no cancellation at any theta, sigma of the
fixture); then |hip - ref| <= 4 E + 2 spacing(|ref|) per element.  E of this
fixture (test_reference_error_per_regime prints it), as E exp / E retr, and
the largest |hip - ref| measured on an MI355X, exp / retr:

  regime            E exp     E retr      hip exp   hip retr
  zero              0.0e+00   1.2e-07     0.0e+00   0.0e+00
  theta_tiny        9.7e-07   1.0e-06     9.5e-07   1.1e-06
  sigma_tiny        8.4e-07   8.6e-07     1.8e-07   4.8e-07
  generic           5.2e-07   2.4e-06     4.8e-07   2.4e-06
  theta_1e-6_1e-3   2.3e-06   2.4e-06     4.1e-06   4.1e-06
  theta_1e-3_0.1    1.3e-06   1.4e-06     1.1e-06   9.5e-07
  sigma_1e-6_1e-2   3.0e-02   3.0e-02     3.0e-02   3.0e-02
  thr_theta_sq      5.7e-05   5.7e-05     4.8e-07   3.8e-06
  thr_theta         6.8e-07   6.9e-07     0.0e+00   0.0e+00
  thr_sigma         9.5e-02   9.5e-02     2.4e-07   2.4e-07
  pose_retr         9.6e-07               2.4e-07

(the large values are the reference's own cancellation in the W coefficients
for small sigma, gn_kernels.cu:359-370: (scale - 1) / sigma and the A, B that
build on it lose all but a few bits near |sigma| = 1e-6; the HIP kernels are
held to the reference, within its own error, not to the exact map).  The
largest |hip - ref| / (4 E + 2 ulp) over all regimes is 0.41.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
from conftest import GOLDEN
from oracle import ref_cases

FIXTURE = os.path.join(GOLDEN, "ref_kernels.npz")
_fx = None


def fixture():
    global _fx
    if _fx is None:
        with np.load(FIXTURE) as z:
            _fx = {k: z[k] for k in z.files}
    return _fx


def same(got, want, what):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want), err_msg=what)


def half_refine_cases(fx):
    return [c for c in ref_cases.refine_cases(fx) if c[1].dtype == np.float16]


# ------------------------------------------------------- the fixture itself
def test_fixture_is_fresh():
    """Every recorded output, recomputed by the reference library from the
    recorded inputs, and the recorded inputs against the generator."""
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref/libref_kernels.so not built (no reference tree)")
    fx = fixture()
    out = ref_cases.reference_outputs(fx)
    inputs = ref_cases.make_inputs()
    assert sorted(fx) == sorted(list(out) + list(inputs))
    for k, v in out.items():
        assert v.dtype == fx[k].dtype and v.shape == fx[k].shape, k
        same(v, fx[k], k)
    for k, v in inputs.items():
        same(v, fx[k], k)


def test_fixture_holds_the_edges():
    fx = fixture()
    assert os.path.getsize(FIXTURE) < 300 * 1024
    moved = np.any(fx["rf_low_out"] != fx["rf_low_p1"], -1)
    assert 0.2 < moved.mean() < 0.8, "low scores: queries that move and queries that stay"
    assert not np.any(fx["rf_neg_out"] != fx["rf_neg_p1"]), "all-negative scores keep the start"
    D11, D21 = fx["rf_low_D11"].astype(np.float64), fx["rf_low_D21"].astype(np.float64)
    sc = np.einsum("bhwf,bnf->bnhw", D11, D21)
    assert sc.min() < -1e-4 and sc.max() > 1e-4 and np.abs(sc).max() < 5e-4
    best = sc.max(axis=(2, 3))
    assert np.any((best > 0) & (best < 6.1e-5)), "best scores between 0 and the fp16 smallest normal"
    big = np.einsum("bhwf,bnf->bnhw", fx["rf_big_D11"].astype(np.float64),
                    fx["rf_big_D21"].astype(np.float64))
    assert 2048 < np.abs(big).max() and np.abs(fx["rf_big_D11"]).max() ** 2 * 16 < 65504
    for name, *_ in half_refine_cases(fx):
        n = fx[f"rf_{name}_p1"].shape[1]
        assert n % 16 and n % 64, name
    conv = fx["ip_b_smooth_conv"][-1]
    assert 0.5 < conv.mean() < 1.0, "smooth rays: converged and unconverged points"
    for name in ref_cases.ITER_CASES:
        assert not np.isnan(fx[f"ip_{name}_pinit"]).any()
        assert not np.isnan(fx[f"ip_{name}_p"]).any()
    p = fx["ip_a_outside_pinit"]
    h, w = fx["ip_rays_a"].shape[1:3]
    assert (p[..., 0] < 0).any() and (p[..., 0] > w).any() and (p[..., 1] < 0).any() \
        and (p[..., 1] > h).any()
    counts = np.bincount(fx["s3_regime"], minlength=len(ref_cases.REGIMES))
    assert (counts[:7] == ref_cases.ROWS).all() and (counts[7:] >= 10).all()


# ------------------------------------- float64 exact Sim3 (for the bound E)
def _quat_mul64(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], 1)


def _rot64(q):
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
                    -1).reshape(-1, 3, 3)


def exact_exp64(xi):
    """Exp of the Sim3 tangent (tau, phi, sigma) in float64: q = (sin(theta/2)
    / theta phi, cos(theta/2)), s = e^sigma, t = W tau with W = int_0^1
    exp(u (sigma I + [phi]x)) du = sum_n M^n / (n+1)!  (|M| <= 3.2 here: 40
    terms leave < 1e-15; no subtraction of nearly equal numbers anywhere)."""
    xi = np.asarray(xi, np.float64)
    tau, phi, sigma = xi[:, :3], xi[:, 3:6], xi[:, 6]
    n = len(xi)
    M = np.zeros((n, 3, 3))
    M[:, 0, 1], M[:, 0, 2] = -phi[:, 2], phi[:, 1]
    M[:, 1, 0], M[:, 1, 2] = phi[:, 2], -phi[:, 0]
    M[:, 2, 0], M[:, 2, 1] = -phi[:, 1], phi[:, 0]
    M += sigma[:, None, None] * np.eye(3)
    W = np.zeros_like(M)
    term = np.tile(np.eye(3), (n, 1, 1))          # M^k / (k+1)!
    for k in range(40):
        W += term
        term = term @ M / (k + 2)
    theta = np.linalg.norm(phi, axis=1)
    imag = 0.5 * np.sinc(theta / (2 * np.pi))     # sin(theta/2) / theta
    q = np.concatenate([imag[:, None] * phi, np.cos(0.5 * theta)[:, None]], 1)
    t = np.einsum("nij,nj->ni", W, tau)
    return np.concatenate([t, q, np.exp(sigma)[:, None]], 1)


def exact_retr64(T, xi):
    """Exp(xi) * T in float64 (T's quaternion taken as given, as retrSim3 does)."""
    T = np.asarray(T, np.float64)
    d = exact_exp64(xi)
    t = d[:, 7:8] * np.einsum("nij,nj->ni", _rot64(d[:, 3:7]), T[:, :3]) + d[:, :3]
    return np.concatenate([t, _quat_mul64(d[:, 3:7], T[:, 3:7]), d[:, 7:8] * T[:, 7:8]], 1)


def reference_error():
    """E per regime: {regime: (E_exp, E_retr)} and E of the pose_retr cases."""
    fx = fixture()
    xi, T = fx["s3_xi"], ref_cases.sim3_T(fx)
    e_exp = np.abs(fx["s3_exp"] - exact_exp64(xi)).max(1)
    e_retr = np.abs(fx["s3_retr"] - exact_retr64(T, xi)).max(1)
    E = {}
    for rid, name in enumerate(ref_cases.REGIMES):
        m = fx["s3_regime"] == rid
        E[name] = (float(e_exp[m].max()), float(e_retr[m].max()))
    e_pr = 0.0
    for nf in fx["pr_fix"]:
        nf = int(nf)
        P = fx["pr_poses"]
        want = exact_retr64(P[nf:], fx["pr_dx"][:len(P) - nf])
        e_pr = max(e_pr, float(np.abs(fx[f"pr_out_fix{nf}"][nf:] - want).max()))
    return E, e_pr


def within(hip, ref, E, what):
    """|hip - ref| <= 4 E + 2 spacing(|ref|), element by element."""
    hip, ref = np.asarray(hip, np.float64), np.asarray(ref, np.float32)
    bound = 4.0 * E + 2.0 * np.spacing(np.abs(ref)).astype(np.float64)
    dev = np.abs(hip - ref.astype(np.float64))
    print(f"{what}: E {E:.3e}  max |hip - ref| {dev.max():.3e}  max dev/bound "
          f"{(dev / bound).max():.3f}")
    assert np.all(dev <= bound), f"{what}: {int((dev > bound).sum())} elements over 4E + 2 ulp"
    return float(dev.max())


def test_reference_error_per_regime():
    """The float64 map is the map the reference computes: where nothing
    cancels the reference is a few ulp from it."""
    E, e_pr = reference_error()
    for name, (a, b) in E.items():
        print(f"E[{name}] exp {a:.1e} retr {b:.1e}")
    print(f"E[pose_retr] {e_pr:.1e}")
    assert E["zero"][0] == 0.0
    # |t| <= 8 in these regimes (spacing 9.5e-7 at 8) and a dozen roundings per element
    for name in ("theta_tiny", "sigma_tiny", "generic", "thr_theta"):
        assert max(E[name]) < 1e-5, (name, E[name])


# --------------------------------------- CPU: restatements vs the reference
def test_oracle_refine_matches_equals_reference():
    for name, D11, D21, p1, r, d, want in half_refine_cases(fixture()):
        same(oracle.refine_matches(D11, D21, p1, r, d), want, name)


def test_oracle_iter_proj_equals_reference():
    for name, rays, pts, p_init, iters, p_want, c_want in ref_cases.iter_cases(fixture()):
        for k, it in enumerate(iters):
            p, c = oracle.iter_proj(rays, pts, p_init, it, ref_cases.LAMBDA_INIT,
                                    ref_cases.COST_THRESH)
            same(p, p_want[k], f"{name} max_iter {it}: p")
            same(c, c_want[k], f"{name} max_iter {it}: converged")


def _per_regime(got, want, fx, what):
    for rid, name in enumerate(ref_cases.REGIMES):
        m = fx["s3_regime"] == rid
        same(got[m], want[m], f"{what}, regime {name}")


def test_oracle_sim3_exp_retr_equal_reference():
    fx = fixture()
    _per_regime(oracle.sim3_exp(fx["s3_xi"]), fx["s3_exp"], fx, "exp")
    _per_regime(oracle.sim3_retr(ref_cases.sim3_T(fx), fx["s3_xi"]), fx["s3_retr"], fx, "retr")


def test_oracle_pose_retr_equals_reference():
    fx = fixture()
    for nf in fx["pr_fix"]:
        nf = int(nf)
        dx = fx["pr_dx"][:len(fx["pr_poses"]) - nf]
        got = oracle.pose_retr(fx["pr_poses"], dx, nf)
        same(got, fx[f"pr_out_fix{nf}"], f"pose_retr num_fix {nf}")
        same(got[:nf], fx["pr_poses"][:nf], "pinned poses")


def test_oracle_sim3_act_mul_inv_equal_reference():
    fx = fixture()
    T, U = fx["g_T"], fx["g_U"]
    same(oracle.sim3_act(T, fx["g_X"]), fx["g_act"], "act")
    same(oracle.sim3_act(T[5:6], fx["g_X"]), fx["g_act1"], "act, one pose")
    same(oracle.sim3_mul(T, U), oracle.lietorch_normalize(fx["g_mul_raw"]), "mul")
    same(oracle.sim3_inv(T), fx["g_inv"], "inv")


def test_native_host_helpers_equal_reference():
    from splatt3r_amd import _lib
    lib = _lib.lib()
    fx = fixture()
    xi, T = fx["s3_xi"], ref_cases.sim3_T(fx)
    out = np.zeros(8, np.float32)
    got = np.zeros_like(fx["s3_retr"])
    for i in range(len(xi)):
        lib.s3lie_sim3_retr_host(T[i].ctypes.data, xi[i].ctypes.data, out.ctypes.data)
        got[i] = out
    _per_regime(got, fx["s3_retr"], fx, "s3lie_sim3_retr_host")
    ident = np.ascontiguousarray(ref_cases.IDENTITY)
    for i in range(len(xi)):
        lib.s3lie_sim3_retr_host(ident.ctypes.data, xi[i].ctypes.data, out.ctypes.data)
        got[i] = out
    _per_regime(got, fx["s3_exp"], fx, "s3lie_sim3_retr_host on the identity (exp)")
    A, B = fx["g_T"], fx["g_U"]
    mul, inv = np.zeros_like(A), np.zeros_like(A)
    for i in range(len(A)):
        lib.s3lie_sim3_mul_host(A[i].ctypes.data, B[i].ctypes.data, out.ctypes.data)
        mul[i] = out
        lib.s3lie_sim3_inv_host(A[i].ctypes.data, out.ctypes.data)
        inv[i] = out
    same(mul, oracle.lietorch_normalize(fx["g_mul_raw"]), "s3lie_sim3_mul_host")
    same(inv, fx["g_inv"], "s3lie_sim3_inv_host")


# ------------------------------------------------- GPU: HIP vs the reference
def _to(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


REFINE_VARIANTS = [(None, None)] + [(l, s) for l in (1, 2, 3, 4, 16) for s in (0, 0x33)]


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,sort", REFINE_VARIANTS)
def test_hip_refine_matches_equals_reference(lanes, sort):
    """Every refine kernel (default; k_refine_lane with 1 / 2 / 4 lanes,
    k_refine_px, k_refine_coop, and the generic k_refine they fall back to
    for radius 4 / fdim 8), in pixel order and binned into 8 x 8 tiles: each
    carries its own initial best score and its own tie rule."""
    import mast3r_slam_backends as be
    from splatt3r_amd import _lib
    L = _lib.lib()
    if lanes is not None:
        L.s3m_refine_set_lanes(lanes)
        L.s3m_refine_set_sort(sort)
    try:
        for name, D11, D21, p1, r, d, want in half_refine_cases(fixture()):
            (out,) = be.refine_matches(_to(D11), _to(D21), _to(p1), r, d)
            same(out.cpu().numpy(), want, name)
    finally:
        L.s3m_refine_set_lanes(-1)
        L.s3m_refine_set_prefetch(4)
        L.s3m_refine_set_sort(-1)


@pytest.mark.gpu
def test_hip_iter_proj_equals_reference():
    import mast3r_slam_backends as be
    for name, rays, pts, p_init, iters, p_want, c_want in ref_cases.iter_cases(fixture()):
        r, q, p0 = _to(rays), _to(pts), _to(p_init)
        for k, it in enumerate(iters):
            p, c = be.iter_proj(r, q, p0, it, ref_cases.LAMBDA_INIT, ref_cases.COST_THRESH)
            same(p.cpu().numpy(), p_want[k], f"{name} max_iter {it}: p")
            same(c.cpu().numpy(), c_want[k], f"{name} max_iter {it}: converged")


@pytest.mark.gpu
def test_hip_sim3_act_mul_inv_equal_reference():
    import lietorch
    fx = fixture()
    T, U = lietorch.Sim3(_to(fx["g_T"])), lietorch.Sim3(_to(fx["g_U"]))
    same(T.act(_to(fx["g_X"])).cpu().numpy(), fx["g_act"], "act")
    one = lietorch.Sim3(_to(fx["g_T"][5:6]))
    same(one.act(_to(fx["g_X"][None]))[0].cpu().numpy(), fx["g_act1"], "act, one pose")
    same((T * U).data.cpu().numpy(), oracle.lietorch_normalize(fx["g_mul_raw"]), "mul")
    same(T.inv().data.cpu().numpy(), fx["g_inv"], "inv")


@pytest.mark.gpu
def test_hip_sim3_exp_retr_within_reference_error(parity):
    import lietorch
    fx = fixture()
    E, _ = reference_error()
    xi = _to(fx["s3_xi"])
    exp = lietorch.Sim3.exp(xi).data.cpu().numpy()
    retr = lietorch.Sim3(_to(ref_cases.sim3_T(fx))).retr(xi).data.cpu().numpy()
    for rid, name in enumerate(ref_cases.REGIMES):
        m = fx["s3_regime"] == rid
        for op, got, want, e in (("exp", exp, fx["s3_exp"], E[name][0]),
                                 ("retr", retr, fx["s3_retr"], E[name][1])):
            dev = within(got[m], want[m], e, f"{op} {name}")
            parity(f"{op}_{name}", err=dev, tol=4 * e, E=e)


@pytest.mark.gpu
def test_hip_pose_retr_within_reference_error(parity):
    from splatt3r_amd import _lib
    fx = fixture()
    _, e = reference_error()
    for nf in fx["pr_fix"]:
        nf = int(nf)
        P = fx["pr_poses"]
        Pd = _to(P)
        dx = _to(fx["pr_dx"][:len(P) - nf])
        _lib.call("s3lie_pose_retr", Pd.data_ptr(), dx.data_ptr(), len(P), nf, _lib.stream())
        got = Pd.cpu().numpy()
        same(got[:nf], P[:nf], "pinned poses untouched")
        dev = within(got[nf:], fx[f"pr_out_fix{nf}"][nf:], e, f"pose_retr num_fix {nf}")
        parity(f"pose_retr_fix{nf}", err=dev, tol=4 * e, E=e)
