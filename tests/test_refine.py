"""Splat optimiser and photometric map refinement: the arithmetic
(csrc/splat_opt_math.hpp), the HIP kernels (csrc/splat_opt.hip, include/s3o.h
s3o_activate / s3o_adam_step) and the loop (splatt3r_amd/refine.py,
SharedGaussians.refine, Frontend.refine_map).

Reference: tests/splat_opt_ref64.py -- torch autograd through the activations
in float64, then torch.optim.Adam in float64, on the CPU, over 3 consecutive
steps with carried state, with the hyperparameters the ABI carries (betas and
eps rounded to float32).  1,000 rows: gradient magnitudes log-uniform over
1e-8..1e2 with 5 % exact zeros, logits in +-12, log-scales in -9..1, raw
quaternion norms in 0.1..10, one zero quaternion; render_scale 1 and 10.

Metrics (splat_opt_ref64.state_errors): a parameter's error is
|a - b| / max(|ref|, lr of its group), the worst entry; a moment's error is
taken per row relative to the row's largest entry of the group, the worst
row; an all-zero reference row must be matched exactly.  Activations as the
moments.  Each figure is the worst over the 3 steps.

Tolerances (the rule of test_splat_io.py): the floor of a quantity is the
error of the same torch composition run in float32 on the CPU against the
float64 reference, and the tolerance is 4 x floor rounded up to one
significant digit.  The floors are computed here on every run, printed, and
recorded through the `parity` fixture; nothing is derived from the code under
test.  Measured floors (render_scale 10; at 1 they differ in the second
digit), and what the code under test gave:

  quantity      floor    tolerance  host build  MI355X (n = 1000)
  p.means       1.5e-7   6e-7       1.5e-7      1.5e-7
  m.means       5.5e-6   3e-5       5.5e-6      5.5e-6
  v.means       2.3e-7   1e-6       2.6e-7      2.6e-7
  p.f_dc        1.6e-7   7e-7       1.6e-7      1.6e-7
  m.f_dc        8.0e-7   4e-6       1.1e-6      1.1e-6
  v.f_dc        1.8e-7   8e-7       1.7e-7      1.7e-7
  p.opacity     2.2e-5   9e-5       1.5e-7      1.5e-7
  m.opacity     7.1e-2   3e-1       4.3e-5      4.3e-5
  v.opacity     1.8e-2   8e-2       1.6e-6      1.6e-6
  p.scale       2.4e-7   1e-6       2.0e-7      2.0e-7
  m.scale       1.3e-5   6e-5       9.9e-6      9.9e-6
  v.scale       1.2e-6   5e-6       1.2e-6      1.2e-6
  p.rotation    2.2e-7   9e-7       2.8e-7      2.8e-7
  m.rotation    1.6e-6   7e-6       1.9e-6      1.9e-6
  v.rotation    1.0e-6   5e-6       6.9e-7      6.9e-7
  m.opacity6    4.1e-5   2e-4       1.5e-6      1.9e-6  (rows starting at
  v.opacity6    6.2e-5   3e-4       9.4e-7      1.0e-6   |logit| <= 6 only)
  act.opacity   1.1e-7   5e-7       5.6e-8      5.6e-8
  act.scale     1.0e-7   5e-7       5.8e-8      5.8e-8
  act.rotation  1.1e-7   5e-7       5.4e-8      5.4e-8
  act.means     5.9e-8   3e-7       5.9e-8      5.9e-8  (render_scale 1: exact)
  act.f_dc      0        0          0           0       (a copy)
(the floors move in the second digit with the host's float32 exp: the MI355X
host gave act.scale 9.5e-8, tolerance 4e-7)

The host build and the kernels run the same source with the same rounding
(-ffp-contract=off), so their figures agree except where the device's expf
differs from the host's.  The activations are formed in double and rounded
once, hence half an ulp.  The opacity floors are large because float32 torch
forms sigmoid's slope as o (1 - o): at |logit| = 12, 1 - o keeps two digits.
The code under test forms it from exp(-|logit|) and sits orders of magnitude
below that floor; because that floor would let a slope error of several
percent pass, the opacity moments are also held to the floor of the rows
that start at |logit| <= 6 (m.opacity6, v.opacity6).  The first moment is written as torch writes it,
m + (1 - beta1) (g - m); written as beta1 m + (1 - beta1) g it gave m.f_dc
3.2e-6 against the 4e-6 tolerance (cancellation of two rounded products).

Adam's update is invariant to a uniform scale of the gradient, so dropping
the render_scale factor from the chain rule shows in the moments, not in the
parameters (test_reference_is_sensitive_to).

End-to-end (test_hip_refine_descends_*): 2,048 Gaussians, three 16 x 32
views, 20 steps.  The bound on |fused - torch float32| final loss is 4 x
|torch float32 - torch with rows and moments carried in float64|, measured in
the test.  On the MI355X: loss 1.293e-2 -> 2.768e-3 (sparse); dense fused
2.764062e-3, torch float32 2.764057e-3, torch float64-carried 2.764134e-3:
difference 5.1e-9 against a distance of 7.7e-8 (bound 3.1e-7).

test_reference_*, test_float32_floors_are_finite: checks of the reference
itself (the issue asks for them); they exercise no code of the feature.
"""
import ctypes
import functools
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import splat_opt_ref64 as R
from conftest import REPO

N = 1000
SIZES = (1, 255, 256, 257, 1000)
SCALES = (1.0, 10.0)


# ------------------------------------------------------------ shared data --
@functools.lru_cache(maxsize=None)
def inputs():
    return R.make_inputs(N)


@functools.lru_cache(maxsize=None)
def ref64(s):
    rows, g = inputs()
    return R.run(rows, g, s), R.activations(rows, s)


@functools.lru_cache(maxsize=None)
def floors(s):
    """Errors of the float32 torch composition against float64."""
    rows, g = inputs()
    steps64, act64 = ref64(s)
    steps32 = R.run(rows, g, s, dtype=torch.float32)
    fl = R.run_errors(steps32, steps64)
    fl.update(R.act_errors(R.activations(rows, s, torch.float32), act64))
    fl.update(opacity6_errors(steps32, N, s))
    return fl


def opacity6_errors(got_steps, n, s):
    """The opacity moments over the rows that start at |logit| <= 6 only.  The
    float32 composition forms sigmoid's slope as o (1 - o), which keeps two
    digits at |logit| = 12, so the floors of m.opacity and v.opacity over all
    rows would let a slope error of several percent pass; on this subset
    1 - o keeps five digits or more and the floor is accordingly smaller."""
    keep = np.abs(inputs()[0][:n, 6]) <= 6.0
    out = {"m.opacity6": 0.0, "v.opacity6": 0.0}
    for a, b in zip(got_steps, ref64(s)[0]):
        for j, k in ((1, "m.opacity6"), (2, "v.opacity6")):
            e = R._row_norm_err(np.asarray(a[j])[:n][keep][:, 6:7], b[j][:n][keep][:, 6:7])
            out[k] = max(out[k], e)
    return out


def check(got_steps, got_act, s, n, label, parity):
    """One run of the code under test on rows [0, n) against float64."""
    steps64, act64 = ref64(s)
    errs = R.run_errors(got_steps, [tuple(x[:n] for x in st) for st in steps64])
    errs.update(opacity6_errors(got_steps, n, s))
    if got_act is not None:
        errs.update(R.act_errors(got_act, act64[:n]))
    fl = floors(s)
    bad = []
    for k, e in errs.items():
        tol = R.tolerance(fl[k]) if fl[k] > 0 else 0.0
        parity(f"{label}.{k}", err=e, tol=tol, floor=fl[k])
        print(f"{label}.{k}: err {e:.3e} floor {fl[k]:.3e} tol {tol:.1e}")
        if not e <= tol:
            bad.append((k, e, tol))
    assert not bad, (label, bad)


# ---------------------------------------------------- CPU: the reference --
def test_reference_adam_written_out_is_torch_adam():
    rows, g = inputs()
    e = R.run_errors(R.run(rows[:200], g[:, :200], 10.0, manual=True),
                     [tuple(x[:200] for x in st) for st in ref64(10.0)[0]])
    assert max(e.values()) <= 1e-12, e


def test_float32_floors_are_finite(parity):
    for s in SCALES:
        for k, v in floors(s).items():
            parity(f"floor.s{s:g}.{k}", floor=v, tol=R.tolerance(v) if v > 0 else 0.0)
            print(f"floor s={s:g} {k}: {v:.3e}")
            assert np.isfinite(v), (s, k)


@pytest.mark.parametrize("ablate,group,kinds", [("quat_jacobian", "rotation", "pmv"),
                                                ("bias_correction", "means", "p"),
                                                ("bias_correction", "f_dc", "p"),
                                                ("bias_correction", "opacity", "p"),
                                                ("bias_correction", "scale", "p"),
                                                ("bias_correction", "rotation", "p"),
                                                ("render_scale", "means", "mv"),
                                                ("render_scale", "scale", "mv")])
def test_reference_is_sensitive_to(ablate, group, kinds):
    """A kernel that dropped this term would miss the tolerance of the group
    it touches by >= 50 x."""
    rows, g = inputs()
    e = R.run_errors(R.run(rows, g, 10.0, ablate=(ablate,)), ref64(10.0)[0])
    for kind in kinds:
        k = f"{kind}.{group}"
        ratio = e[k] / R.tolerance(floors(10.0)[k])
        print(f"sensitivity {ablate} {k}: {e[k]:.3e} = {ratio:.0f} x tol")
        assert ratio >= 50.0, (ablate, k, ratio)


# ------------------------------------------------------------ CPU: the ABI --
def _hp(**kw):
    from splatt3r_amd.refine import S3oAdam
    v = dict(lr=(1e-3,) * 5, beta1=0.9, beta2=0.999, eps=1e-15, bias1=0.1, bias2_sqrt=0.03,
             render_scale=1.0)
    v.update(kw)
    return S3oAdam((ctypes.c_float * 5)(*v["lr"]), v["beta1"], v["beta2"], v["eps"], v["bias1"],
                   v["bias2_sqrt"], v["render_scale"])


def test_abi_rejects_bad_arguments_before_any_device_work():
    """Status 1 with a message; the pointers are never dereferenced (they are
    not device memory here)."""
    from splatt3r_amd import _lib
    lib = _lib.lib()
    act = lambda rows, n, s, rot=16: lib.s3o_activate(rows, n, s, 16, 16, 16, 16, rot, None)
    for args, msg in (((16, -1, 1.0), b"n < 0"), ((16, 5, 0.0), b"render_scale"),
                      ((None, 5, 1.0), b"null"), ((20, 5, 1.0), b"8-byte"),
                      ((16, 5, 1.0, 24), b"16-byte")):
        assert act(*args) == 1 and msg in lib.s3_last_error(), (args, lib.s3_last_error())
    assert lib.s3o_activate(None, 0, 1.0, None, None, None, None, None, None) == 0
    assert lib.s3_last_error() == b""

    def step(n=5, rows=16, m=16, v=16, drot=16, dsh=16, hp=None, null_hp=False):
        h = hp if hp is not None else _hp()
        return lib.s3o_adam_step(rows, m, v, n, 16, dsh, 16, 16, drot, None,
                                 None if null_hp else ctypes.byref(h), None, None)
    for kw, msg in ((dict(n=-1), b"n < 0"), (dict(null_hp=True), b"null hyperparameters"),
                    (dict(hp=_hp(lr=(1e-3, 1e-3, -1.0, 1e-3, 1e-3))), b"lr[2]"),
                    (dict(hp=_hp(lr=(float("nan"),) * 5)), b"lr[0]"),
                    (dict(hp=_hp(beta1=1.0)), b"beta1"), (dict(hp=_hp(beta2=-0.1)), b"beta2"),
                    (dict(hp=_hp(eps=0.0)), b"eps"), (dict(hp=_hp(bias1=0.0)), b"bias1"),
                    (dict(hp=_hp(bias2_sqrt=1.5)), b"bias2_sqrt"),
                    (dict(hp=_hp(render_scale=-1.0)), b"render_scale"),
                    (dict(rows=None), b"null parameter"), (dict(dsh=None), b"null gradient"),
                    (dict(m=20), b"8-byte"), (dict(drot=8), b"16-byte")):
        assert step(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    assert lib.s3o_adam_step(None, None, None, 0, None, None, None, None, None, None,
                             ctypes.byref(_hp()), None, None) == 0
    assert lib.s3_last_error() == b""


def test_python_validation_needs_no_gpu():
    from splatt3r_amd import refine
    with pytest.raises(TypeError):
        refine.activate(torch.zeros(4, 14, dtype=torch.float64))
    with pytest.raises(ValueError):
        refine.activate(torch.zeros(4, 17))
    with pytest.raises(RuntimeError, match="GPU only"):
        refine.activate(torch.zeros(4, 14))
    assert ctypes.sizeof(refine.S3oAdam) == 44


# ------------------------------------------- CPU: the arithmetic, host build
@functools.lru_cache(maxsize=None)
def _host_exe():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    import atexit
    import tempfile
    d = tempfile.mkdtemp(prefix="splat_opt_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "splat_opt_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(REPO, "splatt3r-slam_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "splat_opt_host.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _host_run(rows, grads, s):
    """(steps, activations) of the host build."""
    exe = _host_exe()
    if exe is None:
        pytest.skip("hipcc not available")
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    n, steps = len(rows), len(grads)
    np.concatenate([rows[None], grads]).astype(np.float32).tofile(fin)
    hp = [repr(R.LRS[g]) for g in R.GROUPS] + [repr(R.BETAS[0]), repr(R.BETAS[1]), repr(R.EPS)]
    subprocess.run([exe, fin, fout, str(steps), repr(float(s))] + hp, check=True, timeout=300)
    out = np.fromfile(fout, np.float32).reshape(1 + 3 * steps, n, 14)
    return [tuple(out[1 + 3 * t:4 + 3 * t]) for t in range(steps)], out[0]


@pytest.mark.parametrize("s", SCALES)
def test_host_math_vs_float64(s, parity):
    rows, g = inputs()
    steps, act = _host_run(rows, g, s)
    check(steps, act, s, N, f"host.s{s:g}", parity)
    # the zero quaternion: identity out, no movement, zero moments
    z = R.ZERO_QUAT_ROW
    assert np.array_equal(act[z, 10:14], np.array([1, 0, 0, 0], np.float32))
    for st in steps:
        assert not st[0][z, 10:14].any() and not st[1][z, 10:14].any()


def test_host_math_skips_non_finite_rows():
    rows, g = inputs()
    rows, g = rows[:8], g[:, :8].copy()
    g[0, 2, 4] = np.nan
    g[0, 5, 12] = -np.inf
    st = _host_run(rows, g[:1], 1.0)[0][0]
    for i in (2, 5):
        assert np.array_equal(st[0][i], rows[i]) and not st[1][i].any() and not st[2][i].any()
    assert not np.array_equal(st[0][3], rows[3])


# --------------------------------------------------------------------- GPU --
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _split_grads(g):
    """Packed [n, 14] gradients -> the five tensors SplatAdam.step takes."""
    g = _cuda(g)
    n = g.shape[0]
    return [g[:, 0:3].contiguous(), g[:, 3:6].reshape(n, 1, 3).contiguous(),
            g[:, 6:7].contiguous(), g[:, 7:10].contiguous(), g[:, 10:14].contiguous()]


def _gpu_run(rows, grads, s, radii=None):
    """(steps, activations, optimiser) of the HIP kernels."""
    from splatt3r_amd.refine import SplatAdam, activate
    p = _cuda(rows).clone()
    n = p.shape[0]
    act = torch.cat([t.reshape(n, -1) for t in activate(p, s)], 1).cpu().numpy()
    opt = SplatAdam(p, **{f"lr_{k}": v for k, v in R.LR.items()}, betas=R.BETAS, eps=R.EPS)
    steps = []
    for g in grads:
        opt.step(_split_grads(g), radii, s)
        steps.append((p.cpu().numpy(), opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy()))
    assert opt.t == len(grads)
    return steps, act, opt


@pytest.mark.gpu
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("n", SIZES)
def test_hip_kernels_vs_float64(n, s, parity):
    rows, g = inputs()
    steps, act, opt = _gpu_run(rows[:n], g[:, :n], s)
    check(steps, act, s, n, f"hip.n{n}.s{s:g}", parity)
    assert opt.skipped == 0


@pytest.mark.gpu
def test_hip_rows_are_independent_and_reproducible():
    rows, g = inputs()
    a, act_a, _ = _gpu_run(rows, g, 10.0)
    b, act_b, _ = _gpu_run(rows, g, 10.0)
    bits = lambda x: np.ascontiguousarray(x).view(np.int32)
    assert np.array_equal(bits(act_a), bits(act_b))
    for sa, sb in zip(a, b):
        for x, y in zip(sa, sb):
            assert np.array_equal(bits(x), bits(y))
    for i in (0, R.ZERO_QUAT_ROW, 255, 256, 511, 999):
        one, act1, _ = _gpu_run(rows[i:i + 1], g[:, i:i + 1], 10.0)
        assert np.array_equal(bits(act1[0]), bits(act_a[i])), i
        for s1, sa in zip(one, a):
            for x, y in zip(s1, sa):
                assert np.array_equal(bits(x[0]), bits(y[i])), i


@pytest.mark.gpu
def test_hip_sparse_and_non_finite_rows_are_left_untouched():
    from splatt3r_amd.refine import SplatAdam
    rows, g = inputs()
    n = 600
    radii = torch.ones(n, dtype=torch.int32, device="cuda")
    dead = torch.arange(n, device="cuda") % 3 == 1
    radii[dead] = 0
    radii[4::30] = -5
    dead = radii <= 0
    p = _cuda(rows[:n]).clone()
    opt = SplatAdam(p)
    opt.step(_split_grads(g[0, :n]), None, 10.0)          # dense: every row moves
    assert bool((p != _cuda(rows[:n])).any(1).all())
    assert bool((opt.exp_avg != 0).any(1).all())
    before = [t.clone() for t in (p, opt.exp_avg, opt.exp_avg_sq)]
    opt.step(_split_grads(g[1, :n]), radii, 10.0)
    for t, b in zip((p, opt.exp_avg, opt.exp_avg_sq), before):
        assert torch.equal(t[dead], b[dead])
        assert bool((t[~dead] != b[~dead]).any(1).all())
    # a NaN and an Inf in two live rows' gradients
    live = torch.nonzero(~dead).flatten()[:2].tolist()
    bad = g[2, :n].copy()
    bad[live[0], 8] = np.nan
    bad[live[1], 0] = np.inf
    before = [t.clone() for t in (p, opt.exp_avg, opt.exp_avg_sq)]
    opt.step(_split_grads(bad), radii, 10.0)
    frozen = dead.clone()
    frozen[live] = True
    for t, b in zip((p, opt.exp_avg, opt.exp_avg_sq), before):
        assert torch.equal(t[frozen], b[frozen])
        assert bool((t[~frozen] != b[~frozen]).any(1).all())
        assert bool(torch.isfinite(t).all())
    assert opt.skipped == 2 and opt.t == 3


# ------------------------------------------------ GPU: the rendering loop --
H, W = 16, 32
P = 2048
K_SMALL = np.array([[40.0, 0.0, W / 2], [0.0, 40.0, H / 2], [0.0, 0.0, 1.0]], np.float32)


@functools.lru_cache(maxsize=None)
def _scene():
    """(true rows14 [P, 14] on the GPU, T_WC [3, 4, 4], K): the Gaussians of
    synthetic.raster_microbench_scene as splat rows, seen from three poses."""
    from splatt3r_amd.gaussian_map import splats_from_cov
    from splatt3r_amd.synthetic import raster_microbench_scene
    sc = raster_microbench_scene(P, H=H, W=W, K=K_SMALL, seed=3)
    r17 = splats_from_cov(_cuda(sc["means"]), _cuda(sc["cov6"]),
                          torch.full((P, 3), 0.5, device="cuda"), _cuda(sc["opacities"]))
    rows = torch.cat([r17[:, :3], r17[:, 6:]], 1).contiguous()
    rows[:, 3:6] = _cuda(sc["shs"][:, 0])
    T = torch.eye(4).repeat(3, 1, 1)
    T[1, :3, 3] = torch.tensor([0.15, -0.05, 0.1])
    T[2, :3, 3] = torch.tensor([-0.2, 0.08, -0.1])
    c, s_ = np.cos(0.04), np.sin(0.04)
    T[2, :3, :3] = torch.tensor([[c, 0, s_], [0, 1, 0], [-s_, 0, c]], dtype=torch.float32)
    return rows, T.cuda(), torch.from_numpy(K_SMALL)


def _perturbed(rows, seed=11):
    """Seeded perturbation of means, f_dc, logits and log-scales, each of the
    size 20 steps of its group's learning rate can cover."""
    g = torch.Generator().manual_seed(seed)
    d = torch.zeros(rows.shape[0], 14)
    d[:, 0:3] = 0.003 * torch.randn(rows.shape[0], 3, generator=g)
    d[:, 3:6] = 0.05 * torch.randn(rows.shape[0], 3, generator=g)
    d[:, 6] = 0.5 * torch.randn(rows.shape[0], generator=g)
    d[:, 7:10] = 0.1 * torch.randn(rows.shape[0], 3, generator=g)
    return (rows + d.to(rows.device)).contiguous()


def _torch_activate(parts, s):
    xyz, fdc, logit, lsc, q = parts
    n = xyz.shape[0]
    return (s * xyz, fdc.reshape(n, 1, 3), torch.sigmoid(logit), s * torch.exp(lsc),
            q / q.norm(dim=1, keepdim=True))


def _torch_refine(rows, images, T_WC, K, iters, dtype):
    """The torch composition of refine_splats: autograd activations and
    torch.optim.Adam over five groups carried in `dtype`, cast to float32 only
    for the rasterizer; dense.  Returns the per-step losses."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from splatt3r_amd.photometric import photometric_loss
    from splatt3r_amd.refine import _cameras
    settings, s = _cameras(T_WC, K, H, W, 0.1, 1000.0, None, rows.device)
    parts = [rows[:, R.SL[g]].to(dtype).clone().requires_grad_(True) for g in R.GROUPS]
    opt = torch.optim.Adam([dict(params=[p], lr=R.LRS[g]) for p, g in zip(parts, R.GROUPS)],
                           betas=R.BETAS, eps=R.EPS, foreach=False)
    hist = []
    for it in range(iters):
        opt.zero_grad(set_to_none=True)
        m, sh, o, sc, q = [t.float() for t in _torch_activate(parts, s)]
        img, _ = GaussianRasterizer(settings[it % len(settings)])(
            means3D=m, means2D=torch.zeros_like(m), opacities=o, shs=sh, scales=sc, rotations=q)
        v = it % len(settings)
        loss = photometric_loss(img[None], images[v:v + 1], None, mse_weight=0.0, l1_weight=0.8,
                                ssim_weight=0.2)
        loss.backward()
        hist.append(loss.detach())
        opt.step()
    return torch.stack(hist)


@pytest.mark.gpu
def test_hip_autograd_wiring(parity):
    """Two pipelines, each through GaussianRasterizer and photometric_loss:
    (1) activate -> rasterizer -> loss -> backward, the gradients of the
    activated tensors pushed through the float64 chain rule; (2) float64
    autograd on the rows through a torch activation (cast to float32 for the
    rasterizer) into a rasterizer and loss call of its own.  Tolerances: the
    rasterizer gradient tolerances of tests/test_raster_grad.py, metric
    max |a - b| / max |ref| per group.

    With a float32 activation (expf, one ulp from the float32 cast of the
    float64 activation in 666 opacities, 1,700 scales and 2,378 quaternion
    entries of this scene) the groups differed by 4.4e-6, 4.6e-6, 1.3e-6,
    2.3e-6 and 3.5e-6, rotation over its 3e-6.  Measured cause:
    not the rasterizer's backward (each side within 2.6e-6 of float64 on its
    own inputs, the same inputs twice bit-identical, no fragile Gaussian among
    the worst rows) but the loss: the images differ by 1.8e-7 and
    photometric_loss's dL/dimage by 1e-5 of its largest entry; with one
    side's dL/dimage given to both, the float64 rasterizer gradients of the
    two input sets agree to 1.9e-7.  activate now rounds its outputs
    correctly (formed in double), so both pipelines get the same bits.  That
    is checked first, to 4 x the error of the float32 torch activation, and
    the number of differing entries is printed."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from splatt3r_amd.photometric import photometric_loss
    from splatt3r_amd.refine import _cameras, activate, render_splats
    from test_raster_grad import TOL as RT, rel_err
    tol = dict(means=RT["dL_dmeans3D"], f_dc=RT["dL_dsh"], opacity=RT["dL_dopacity"],
               scale=RT["dL_dscales"], rotation=RT["dL_drotations"])
    true, T_WC, K = _scene()
    target = render_splats(true, T_WC, K, H, W)[1:2]
    rows = _perturbed(true)
    settings, s = _cameras(T_WC, K, H, W, 0.1, 1000.0, None, rows.device)

    def loss_of(m, sh, o, sc, q):
        img, _ = GaussianRasterizer(settings[1])(means3D=m, means2D=torch.zeros_like(m),
                                                 opacities=o, shs=sh, scales=sc, rotations=q)
        return photometric_loss(img[None], target, None, mse_weight=0.0, l1_weight=0.8,
                                ssim_weight=0.2)
    acts = [t.requires_grad_(True) for t in activate(rows, s)]
    loss_of(*acts).backward()
    packed = torch.cat([a.grad.reshape(P, -1) for a in acts], 1).cpu().numpy()
    got = R.chain_rule64(rows.cpu().numpy(), packed, s)
    parts = [rows[:, R.SL[g]].double().clone().requires_grad_(True) for g in R.GROUPS]
    t64 = _torch_activate(parts, s)
    act_hip = torch.cat([a.detach().reshape(P, -1) for a in acts], 1).cpu().numpy()
    act64 = torch.cat([t.detach().reshape(P, -1) for t in t64], 1).cpu().numpy()
    fl = R.act_errors(R.activations(rows.cpu().numpy(), s, torch.float32), act64)
    for k, e in R.act_errors(act_hip, act64).items():
        t = R.tolerance(fl[k]) if fl[k] > 0 else 0.0
        parity(f"hip.wiring.{k}", err=e, tol=t, floor=fl[k])
        print(f"hip.wiring.{k}: err {e:.3e} floor {fl[k]:.3e} tol {t:.1e}")
        assert e <= t, (k, e, t)
    differ = sum(int((a.detach() != t.detach().float()).sum()) for a, t in zip(acts, t64))
    print(f"hip.wiring: {differ} of {P * 14} activation entries differ from float32(float64)")
    loss_of(*[t.float() for t in t64]).backward()
    want = torch.cat([p.grad for p in parts], 1).cpu().numpy()
    assert np.abs(want).max() > 0
    bad = []
    for g in R.GROUPS:
        e = rel_err(got[:, R.SL[g]], want[:, R.SL[g]])
        parity(f"hip.wiring.{g}", max_rel=e, tol=tol[g])
        print(f"hip.wiring.{g}: err {e:.3e} tol {tol[g]:.1e}")
        if not e <= tol[g]:
            bad.append((g, e, tol[g]))
    assert not bad, bad
    # the fused step fed with that call's gradients as refine_splats feeds it,
    # against float64 Adam on the same gradients; floors: the float32 torch
    # composition on these rows and gradients
    from splatt3r_amd.refine import SplatAdam
    p = rows.clone()
    opt = SplatAdam(p)
    opt.step([a.grad for a in acts], None, s)
    r = rows.cpu().numpy()
    ref = R.run(r, packed[None], s)[0]
    fl = R.state_errors(R.run(r, packed[None], s, dtype=torch.float32)[0], ref)
    errs = R.state_errors((p.cpu().numpy(), opt.exp_avg.cpu().numpy(),
                           opt.exp_avg_sq.cpu().numpy()), ref)
    for k, e in errs.items():
        t = R.tolerance(fl[k]) if fl[k] > 0 else 0.0
        parity(f"hip.wiring.step.{k}", err=e, tol=t, floor=fl[k])
        print(f"hip.wiring.step.{k}: err {e:.3e} floor {fl[k]:.3e} tol {t:.1e}")
        if not e <= t:
            bad.append((k, e, t))
    assert not bad, bad


@pytest.mark.gpu
def test_hip_refine_descends_deterministically_and_matches_torch(parity):
    """20 steps over three 16 x 32 views from a perturbed start (see the
    module docstring)."""
    from splatt3r_amd.refine import refine_splats, render_splats
    true, T_WC, K = _scene()
    images = render_splats(true, T_WC, K, H, W)
    assert float(images.std()) > 0.02
    start = _perturbed(true)
    keep = start.clone()
    rows_a, hist_a = refine_splats(start, images, T_WC, K, 20)
    rows_b, hist_b = refine_splats(start, images, T_WC, K, 20)
    assert torch.equal(start, keep)
    assert torch.equal(hist_a, hist_b) and torch.equal(rows_a, rows_b)
    assert hist_a.shape == (20,) and hist_a.is_cuda
    ha = hist_a.cpu().numpy().astype(np.float64)
    print("fused sparse losses:", ha[0], ha[-1])
    assert ha[-1] < ha[0]
    # the torch composition is dense: compare the dense fused loop
    _, hist_d = refine_splats(start, images, T_WC, K, 20, sparse=False)
    hd = hist_d.cpu().numpy().astype(np.float64)
    assert hd[-1] < hd[0]
    h32 = _torch_refine(start, images, T_WC, K, 20, torch.float32).cpu().numpy().astype(np.float64)
    h64 = _torch_refine(start, images, T_WC, K, 20, torch.float64).cpu().numpy().astype(np.float64)
    dist = abs(h32[-1] - h64[-1])
    err = abs(hd[-1] - h32[-1])
    parity("hip.refine.final_loss", err=err, tol=4.0 * dist, floor=dist)
    print(f"hip.refine.final_loss: fused {hd[-1]:.9e} torch32 {h32[-1]:.9e} torch64 {h64[-1]:.9e} "
          f"err {err:.3e} distance {dist:.3e}")
    assert err <= 4.0 * dist


def _map_of(rows14, kf_ids, cap=2048):
    """A SharedGaussians holding splat rows (through s3w_map_from_splats)."""
    from splatt3r_amd import _lib
    from splatt3r_amd.gaussian_map import SharedGaussians
    gm = SharedGaussians(max_gaussians=cap, device="cuda")
    _lib.call("s3w_map_from_splats", ctypes.byref(gm._c), rows14.data_ptr(), rows14.shape[0], 0,
              _lib.stream(gm.device))
    gm.kf_id[:rows14.shape[0]] = kf_ids
    return gm


def _map_rows():
    """1,000 rows: 900 of the scene, perturbed, then 100 behind every camera."""
    true, T_WC, K = _scene()
    t = true[:1000].clone()
    t[900:, 2] = -t[900:, 2] - 5.0
    start = _perturbed(t, seed=12)
    start[900:] = t[900:]
    kf = (torch.arange(1000, device="cuda") % 7).to(torch.int32)
    return t, start, kf


@pytest.mark.gpu
def test_hip_map_refine_keeps_count_ids_and_unseen_gaussians():
    from splatt3r_amd.refine import render_splats
    _, T_WC, K = _scene()
    t, start, kf = _map_rows()
    images = render_splats(t, T_WC, K, H, W)
    gm = _map_of(start, kf)
    fields = lambda: [x[:1000].clone() for x in (gm.means, gm.cov_triu, gm.colors, gm.opacities)]
    before = fields()
    hist = gm.refine(images, T_WC, K, 12)
    assert gm.n_gaussians == 1000 and torch.equal(gm.kf_id[:1000], kf)
    h = hist.cpu().numpy()
    print("map refine losses:", h[0], h[-1])
    assert h.shape == (12,) and h[-1] < h[0]
    after = fields()
    for a, b in zip(after, before):
        assert torch.equal(a[900:], b[900:])
    assert float((after[0][:900] != before[0][:900]).any(1).float().mean()) > 0.5
    from splatt3r_amd.gaussian_map import SharedGaussians
    assert SharedGaussians(max_gaussians=16, device="cuda").refine(images, T_WC, K, 2) is None


@pytest.mark.gpu
def test_hip_frontend_refine_map():
    """Hand-built keyframes, no network: the frontend hands its keyframes'
    images (keyframe_target), poses and default intrinsics to
    SharedGaussians.refine."""
    import lietorch
    from splatt3r_amd.evaluate import keyframe_target
    from splatt3r_amd.frame import create_frame
    from splatt3r_amd.refine import render_splats
    from splatt3r_amd.slam import Frontend
    from splatt3r_amd.splatt3r_utils import _estimate_default_intrinsics, _sim3_to_4x4
    dev = torch.device("cuda", 0)
    t, start, kf = _map_rows()
    poses = torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1], [0.15, -0.05, 0.1, 0, 0, 0, 1, 1]],
                         dtype=torch.float32, device=dev)
    T_WC = torch.cat([_sim3_to_4x4(lietorch.Sim3(p[None])) for p in poses]).to(dev)
    K = _estimate_default_intrinsics(H, W, "cpu")
    images = render_splats(t, T_WC, K, H, W)
    fe = Frontend(types.SimpleNamespace(), device=dev, render=False, viz=True, max_gaussians=2048)
    assert fe.refine_map(3) is None                   # no keyframe, empty map
    for i in range(2):
        fe.keyframes.append(create_frame(i, (images[i:i + 1] * 2.0 - 1.0).contiguous(),
                                         lietorch.Sim3(poses[i:i + 1].clone()), device=dev))
    fe.gmap = _map_of(start, kf)
    other = _map_of(start, kf)
    hist = fe.refine_map(6)
    targets = torch.cat([keyframe_target(fe.keyframes[i]) for i in range(2)]).contiguous()
    want = other.refine(targets, T_WC, K, 6)
    assert torch.equal(hist, want) and float(hist[-1]) < float(hist[0])
    for a, b in zip((fe.gmap.means, fe.gmap.cov_triu, fe.gmap.colors, fe.gmap.opacities),
                    (other.means, other.cov_triu, other.colors, other.opacities)):
        assert torch.equal(a, b)
    assert torch.equal(fe.gmap.kf_id[:1000], kf)
    fe.close()
