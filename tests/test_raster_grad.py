"""Rasterizer gradients against a float64 autograd reference.

tests/raster_ref64.py restates the forward of include/gsr.h densely in
float64 PyTorch and lets autograd differentiate it; it shares no backward
code with csrc/raster.hip or oracle/raster_ref.c.  The CPU tests hold the
oracle's backward to it (and check that the scenes are sensitive to the terms
a transposed index or a dropped factor would break); the GPU tests add the
HIP kernels: forward bit-exact against the oracle, backward against the
oracle (BWD_TOL) and against the float64 reference (TOL below).

Scenes: 41 x 59 pixels (partial right and bottom tiles), <= 206 Gaussians,
one camera rotated 25 degrees about (1, 2, 3) and translated, so every entry
of the view matrix's rotation block is non-zero and campos != 0.  Gaussians
the reference flags as fragile (a discrete rule within float32 reach of its
threshold) are resampled; fragile pixels get dL_dout = 0 and are left out of
image comparisons (cap: 2 % of the pixels per case).

Metric: max|a - b| / max|ref| per tensor (the image: max|a - b|, absolute).

Floors and tolerances.  floor = float32 rounding measured WITHOUT the kernel:
for tensors the oracle produces, oracle minus reference (worst case over the
cases, test_reference_vs_oracle prints them); for dL_dscales, dL_drotations
and dL_dmeans3D with SH degree > 0, the reference run in float32 minus the
reference in float64 (test_float32_floor).  tol = 4 x floor rounded up to one
significant digit; the factor covers the kernel's different summation order
(float atomics, wave reductions).  A kernel error above tol is a finding.

  tensor         floor     worst case  measured as          tol
  image          4.9e-6    sh3         oracle               2e-05
  dL_dmeans2D    2.0e-6    sh1_M4      oracle               8e-06
  dL_dopacity    1.3e-6    jclamp      oracle               6e-06
  dL_dcolors     1.7e-6    culled      oracle               7e-06
  dL_dmeans3D    1.9e-6    sh1         float32 reference    8e-06
  dL_dcov3D      2.2e-6    jclamp      oracle               9e-06
  dL_dsh         1.3e-6    sh1         oracle               6e-06
  dL_dscales     1.6e-6    scale_rot   float32 reference    7e-06
  dL_drotations  7.2e-7    scale_rot   float32 reference    3e-06
(floors rounded up to two digits; dL_dmeans3D over the oracle for SH degree 0
and the float32 reference for degrees 1..3)
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import oracle
import raster_ref64 as R64
from splatt3r_amd.synthetic import raster_grad, settings_to_dict
from test_raster import BWD_TOL

#            floor (measured)   tol = roundup_1sig(4 x floor)
FLOOR = {
    "image":          4.9e-6,
    "dL_dmeans2D":    2.0e-6,
    "dL_dopacity":    1.3e-6,
    "dL_dcolors":     1.7e-6,
    "dL_dmeans3D":    1.9e-6,
    "dL_dcov3D":      2.2e-6,
    "dL_dsh":         1.3e-6,
    "dL_dscales":     1.6e-6,
    "dL_drotations":  7.2e-7,
}


def _roundup_1sig(x):
    e = np.floor(np.log10(x))
    return float(np.ceil(x / 10 ** e - 1e-9) * 10 ** e)


TOL = {k: _roundup_1sig(4.0 * v) for k, v in FLOOR.items()}

H, W, FX = 41, 59, 55.0
BG = (0.2, 0.5, 0.8)
FRAGILE_CAP = 0.02

CASES = {
    "view":      dict(seed=11, groups=(("std", 170),), color="sh", D=0, M=1, cov="pre"),
    "scale_rot": dict(seed=12, groups=(("std", 170),), color="pre", D=0, M=0, cov="sr", mod=1.7),
    "sh1":       dict(seed=13, groups=(("std", 150),), color="sh", D=1, M=16, cov="pre"),
    "sh2":       dict(seed=14, groups=(("std", 150),), color="sh", D=2, M=16, cov="pre"),
    "sh3":       dict(seed=15, groups=(("std", 150),), color="sh", D=3, M=16, cov="pre"),
    "sh1_M4":    dict(seed=16, groups=(("std", 150),), color="sh", D=1, M=4, cov="pre"),
    "jclamp":    dict(seed=17, groups=(("std", 110), ("big", 16)), color="sh", D=0, M=1, cov="pre"),
    "sat":       dict(seed=18, groups=(("sat", 90),), color="sh", D=0, M=1, cov="pre"),
    "culled":    dict(seed=11, groups=(("std", 170), ("behind", 12), ("near", 12), ("off", 12)),
                      color="sh", D=0, M=1, cov="pre"),
    # no convention active (no Jacobian clamp, alpha < 0.99): finite differences
    "fd":        dict(seed=19, groups=(("inner", 40),), color="sh", D=2, M=9, cov="sr", mod=1.3),
}
MAIN = [c for c in CASES if c != "fd"]
# DC offset (in colour units) that puts 10..40 % of the SH channels below zero
SH_DC = {0: 0.0, 1: 0.5, 2: 0.5, 3: 0.5}


# ------------------------------------------------------------------ scenes
def camera(D, mod=1.0, device="cpu"):
    """One rotated, translated camera through render.camera_settings."""
    from splatt3r_amd.render import camera_settings, normalize_intrinsics
    K = torch.tensor([[[FX, 0, W / 2], [0, FX, H / 2], [0, 0, 1]]], dtype=torch.float32)
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    th = np.deg2rad(25.0)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rc = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    ext = np.eye(4)
    ext[:3, :3] = Rc
    ext[:3, 3] = (0.03, -0.02, 0.05)          # x scale (1 / near = 10) inside camera_settings
    st, _ = camera_settings(torch.tensor(ext[None], dtype=torch.float32),
                            normalize_intrinsics(K, (H, W)), torch.full((1,), 0.1),
                            torch.full((1,), 1000.0), (H, W), torch.tensor([BG]), D)
    rs = st[0]._replace(scale_modifier=mod)
    if device != "cpu":
        rs = rs._replace(bg=rs.bg.to(device), viewmatrix=rs.viewmatrix.to(device),
                         projmatrix=rs.projmatrix.to(device), campos=rs.campos.to(device))
    return rs


def _rot(q):
    r, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def _draw(kind, rng, cfg, tanx, tany):
    """One Gaussian in view space (rasterizer units)."""
    cx, cy = W / 2, H / 2
    z = rng.uniform(2.0, 3.3)
    u, v = rng.uniform(-3, W + 3), rng.uniform(-3, H + 3)
    spx = rng.uniform(1.5, 4.5)
    op = rng.uniform(0.05, 0.95)
    if kind == "inner":
        u, v = rng.uniform(8, W - 8), rng.uniform(8, H - 8)
        op = rng.uniform(0.05, 0.8)
    elif kind == "big":
        # centre 1.35 .. 1.6 x the half image outside the optical axis: past the
        # 1.3 tan(fov) Jacobian clamp, rectangle (3 sigma >= 24 px) still on screen
        spx, op = rng.uniform(8.0, 12.0), rng.uniform(0.5, 0.9)
        k = rng.uniform(1.35, 1.6) * rng.choice([-1.0, 1.0])
        if rng.random() < 0.5:
            u, v = cx + k * cx, rng.uniform(5, H - 5)
        else:
            u, v = rng.uniform(5, W - 5), cy + k * cy
    elif kind == "sat":
        spx, op = rng.uniform(3.0, 7.0), rng.uniform(0.99, 1.0)
    elif kind == "behind":
        z = -rng.uniform(0.5, 5.0)
    elif kind == "near":
        z = rng.uniform(0.02, 0.19)
    elif kind == "off":
        u = cx + rng.uniform(3.0, 5.0) * W * rng.choice([-1.0, 1.0])
    fx, fy = W / (2 * tanx), H / (2 * tany)
    pv = np.array([(u - (cx - 0.5)) / fx * z, (v - (cy - 0.5)) / fy * z, z])
    s3 = spx * abs(z) / fx * np.exp(rng.uniform(-0.5, 0.5, 3))
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    row = dict(pv=pv, s3=s3, q=q, op=op, qn=rng.uniform(0.8, 1.25),
               col=rng.uniform(0.0, 1.0, 3))
    M, D = cfg["M"], cfg["D"]
    if M:
        sh = rng.uniform(1.0, 3.0, (M, 3)) * rng.choice([-1.0, 1.0], (M, 3))
        sh[0] = (SH_DC[D] + rng.normal(size=3) * 0.5) / R64.SH_C0
        row["sh"] = sh
    return row


def _assemble(rows, cfg, Rw, tw):
    pv = np.stack([r["pv"] for r in rows])
    out = dict(means3D=((pv - tw) @ Rw).astype(np.float32),     # Rw^T (pv - tw)
               opacities=np.array([[r["op"]] for r in rows], np.float32))
    if cfg["cov"] == "pre":
        cov = np.stack([_rot(r["q"]) @ np.diag(r["s3"] ** 2) @ _rot(r["q"]).T for r in rows])
        iu = np.triu_indices(3)
        out["cov3D_precomp"] = cov[:, iu[0], iu[1]].astype(np.float32)
    else:
        # raw quaternion of norm 0.8 .. 1.25; the scales undo scale_modifier
        out["scales"] = np.stack([r["s3"] / cfg["mod"] for r in rows]).astype(np.float32)
        out["rotations"] = np.stack([r["q"] * r["qn"] for r in rows]).astype(np.float32)
    if cfg["color"] == "sh":
        out["shs"] = np.stack([r["sh"] for r in rows]).astype(np.float32)
    else:
        out["colors_precomp"] = np.stack([r["col"] for r in rows]).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def scene(name):
    """Inputs, dL_dout and the float64 reference of one case (computed once,
    shared by every test; treat as read-only)."""
    cfg = CASES[name]
    rs = camera(cfg["D"], cfg.get("mod", 1.0))
    sd = settings_to_dict(rs)
    vm = np.asarray(sd["viewmatrix"], np.float64).reshape(4, 4)
    Rw, tw = vm[:3, :3].T, vm[3, :3]
    rng = np.random.Generator(np.random.PCG64(cfg["seed"]))
    kinds = [k for k, n in cfg["groups"] for _ in range(n)]
    rows = [_draw(k, rng, cfg, sd["tanfovx"], sd["tanfovy"]) for k in kinds]
    for _ in range(100):
        inp = _assemble(rows, cfg, Rw, tw)
        fr = R64.render(sd, **inp)["fragile_g"]
        if not fr.any():
            break
        for i in np.nonzero(fr)[0]:
            rows[i] = _draw(kinds[i], rng, cfg, sd["tanfovx"], sd["tanfovy"])
    else:
        raise AssertionError(f"{name}: fragile Gaussians remain")
    fwd = R64.render(sd, **inp)
    g = raster_grad(H, W, seed=100 + cfg["seed"])
    g[:, fwd["fragile_px"]] = 0.0
    ref = R64.render(sd, **inp, dL_dout=g)
    return dict(name=name, cfg=cfg, rs=rs, sd=sd, inp=inp, g=g, ref=ref, kinds=np.array(kinds),
                ok_px=~ref["fragile_px"])


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    sc = scene(name)
    return oracle.raster(sc["sd"], dL_dout=sc["g"], **sc["inp"])


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a.reshape(b.shape) - b).max() / (np.abs(b).max() + 1e-300))


def oracle_names(cfg):
    n = ["dL_dmeans2D", "dL_dopacity", "dL_dcolors", "dL_dcov3D"]
    if cfg["color"] == "sh":
        n.append("dL_dsh")
    if cfg["D"] == 0:
        n.append("dL_dmeans3D")     # the oracle has no view-direction term
    return n


# --------------------------------------------------------------- CPU tests
def test_camera_is_general():
    sd = scene("view")["sd"]
    vm = np.asarray(sd["viewmatrix"]).reshape(4, 4)
    assert np.abs(vm[:3, :3]).min() > 0.05
    assert np.abs(np.asarray(sd["campos"])).min() > 0.1


@pytest.mark.parametrize("name", MAIN)
def test_fragile_pixel_cap(name):
    sc = scene(name)
    frac = sc["ref"]["fragile_px"].mean()
    print(f"{name}: fragile pixels {frac:.4%}")
    assert not sc["ref"]["fragile_g"].any()
    assert frac <= FRAGILE_CAP


@pytest.mark.parametrize("name", MAIN)
def test_reference_vs_oracle(name, parity):
    """The oracle (forward and its hand-written backward) against autograd."""
    sc, o = scene(name), oracle_run(name)
    ref = sc["ref"]
    np.testing.assert_array_equal(o["radii"], ref["radii"])
    d = float(np.abs(o["color"] - ref["color"])[:, sc["ok_px"]].max())
    errs = {"image": d}
    for n in oracle_names(sc["cfg"]):
        errs[n] = rel_err(o[n], ref[n])
    for n, e in errs.items():
        print(f"floor {name} {n} {e:.3e}")
        parity(f"ref64_oracle_{name}_{n}", max_rel=e, tol=TOL[n])
    for n, e in errs.items():
        assert e <= TOL[n], (name, n, e)


@pytest.mark.parametrize("name", ["scale_rot", "sh1", "sh2", "sh3", "sh1_M4"])
def test_float32_floor(name, parity):
    """Rounding floor of the tensors the oracle does not produce: the
    reference in float32 against itself in float64."""
    sc = scene(name)
    r32 = R64.render(sc["sd"], **sc["inp"], dL_dout=sc["g"], dtype=torch.float32)
    np.testing.assert_array_equal(r32["radii"], sc["ref"]["radii"])
    names = ["dL_dscales", "dL_drotations"] if name == "scale_rot" else ["dL_dmeans3D"]
    for n in names:
        e = rel_err(r32[n], sc["ref"][n])
        print(f"floor32 {name} {n} {e:.3e}")
        parity(f"ref64_ref32_{name}_{n}", max_rel=e, tol=TOL[n])
        assert e <= TOL[n], (name, n, e)


@pytest.mark.parametrize("name", ["sh1", "sh2", "sh3", "sh1_M4"])
def test_sh_cases_clamp_share_and_unused_coefficients(name):
    sc = scene(name)
    vis = sc["ref"]["visible"]
    share = sc["ref"]["sh_clamped"][vis].mean()
    print(f"{name}: clamped SH channels {share:.3f}")
    assert 0.10 <= share <= 0.40
    D, M = sc["cfg"]["D"], sc["cfg"]["M"]
    nb = (D + 1) ** 2
    assert np.abs(sc["inp"]["shs"][:, 1:]).min() >= 1.0
    assert np.all(sc["ref"]["dL_dsh"][:, nb:] == 0.0)
    assert np.abs(sc["ref"]["dL_dsh"][:, :nb]).max() > 0
    if M > nb:
        assert np.all(oracle_run(name)["dL_dsh"][:, nb:] == 0.0)


def test_jclamp_case_has_active_clamp():
    sc = scene("jclamp")
    ref = sc["ref"]
    gsum = np.abs(ref["dL_dmeans3D"]).sum(1) * np.abs(ref["dL_dcov3D"]).sum(1)
    n = int((ref["jclamp"] & (gsum > 0)).sum())
    print(f"jclamp: {n} clamped Gaussians with a gradient")
    assert n >= 10


def test_sat_case_has_active_alpha_clamp():
    """Pixels where o G >= 0.99: the straight-through clamp is exercised."""
    sc = scene("sat")
    assert sc["inp"]["opacities"].min() >= 0.99
    n = sc["ref"]["alpha_clamped"]
    print(f"sat: {n} blended pairs with o G > 0.99")
    assert n >= 20
    for name in MAIN:
        if name != "sat":
            assert scene(name)["ref"]["alpha_clamped"] == 0


def test_culled_case_has_all_three_kinds():
    sc = scene("culled")
    vis, kinds = sc["ref"]["visible"], sc["kinds"]
    for k in ("behind", "near", "off"):
        assert (kinds == k).sum() >= 10 and not vis[kinds == k].any()
    assert vis[kinds == "std"].mean() > 0.9
    for n in ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh"):
        assert np.all(sc["ref"][n][~vis] == 0.0)
        assert np.all(oracle_run("culled")[n][~vis] == 0.0)


@pytest.mark.parametrize("name,ablate,tensor", [("sh2", "viewdir", "dL_dmeans3D"),
                                                ("sh3", "viewdir", "dL_dmeans3D"),
                                                ("view", "bg", "dL_dopacity"),
                                                ("view", "vm_T", "dL_dmeans3D"),
                                                ("scale_rot", "scale_mod", "dL_dscales")])
def test_scene_is_sensitive_to(name, ablate, tensor):
    """A kernel that dropped this term would miss the tolerance by >= 50x."""
    sc = scene(name)
    cut = R64.render(sc["sd"], **sc["inp"], dL_dout=sc["g"], ablate=(ablate,))
    np.testing.assert_allclose(cut["color"], sc["ref"]["color"], rtol=0, atol=1e-12)
    e = rel_err(cut[tensor], sc["ref"][tensor])
    print(f"sensitivity {name} {ablate} {tensor}: {e:.3e} = {e / TOL[tensor]:.0f} x tol")
    assert e >= 50.0 * TOL[tensor]


def test_reference_forward_finite_differences():
    """Central differences of the float64 forward against autograd, on a case
    where no convention is active (guards a misplaced detach)."""
    sc = scene("fd")
    ref = sc["ref"]
    assert not ref["jclamp"].any()
    assert sc["inp"]["opacities"].max() < 0.99
    g = sc["g"].astype(np.float64)
    L = lambda inp: float((R64.render(sc["sd"], **inp)["color"] * g).sum())
    rng = np.random.Generator(np.random.PCG64(5))
    vis = np.nonzero(ref["visible"])[0]
    for key, gname in (("scales", "dL_dscales"), ("rotations", "dL_drotations"),
                       ("shs", "dL_dsh"), ("means3D", "dL_dmeans3D")):
        a = ref[gname]
        scale = np.abs(a).max()
        for _ in range(3):
            while True:     # an entry that carries gradient (not a clamped SH channel)
                i = int(rng.choice(vis))
                j = tuple(int(rng.integers(0, s)) for s in a.shape[1:])
                if abs(a[(i,) + j]) > 1e-3 * scale:
                    break
            x0 = np.asarray(sc["inp"][key], np.float64)
            h = 1e-6 * max(1.0, abs(x0[(i,) + j])) if key != "scales" else 1e-6 * x0[(i,) + j]
            p, m = x0.copy(), x0.copy()
            p[(i,) + j] += h
            m[(i,) + j] -= h
            fd = (L({**sc["inp"], key: p}) - L({**sc["inp"], key: m})) / (2 * h)
            print(f"fd {key}[{i},{j}]: autograd {a[(i,) + j]:.9e} fd {fd:.9e}")
            assert abs(fd - a[(i,) + j]) <= 1e-6 * scale + 1e-5 * abs(fd), (key, i, j)


def test_sh_basis_and_grad_native(tmp_path):
    """gsr::sh_basis / sh_basis_grad (raster_math.hpp) for deg 0..3 against
    double closed forms and their central differences; the bound is derived
    in tests/native/sh_basis_check.cpp.  Host code built by hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "splatt3r-slam_amd", "csrc")
    exe = str(tmp_path / "sh_basis_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", csrc, os.path.join(here, "native", "sh_basis_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    out = subprocess.run([exe, "20000"], check=True, capture_output=True, text=True, timeout=300)
    n, wb, wg, stray = out.stdout.split()
    print("sh_basis_check:", out.stdout.strip())
    assert int(n) == 20000 and int(stray) == 0
    assert 0.0 < float(wb) <= 1.0, out.stdout
    assert 0.0 < float(wg) <= 1.0, out.stdout


# --------------------------------------------------------------- GPU tests
def _cuda(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def gpu_run(name):
    """One forward + backward of the HIP rasterizer per case."""
    from diff_gaussian_rasterization import GaussianRasterizer
    sc = scene(name)
    rs = camera(sc["cfg"]["D"], sc["cfg"].get("mod", 1.0), "cuda")
    kw = {k: _cuda(v, True) for k, v in sc["inp"].items()}
    kw["means2D"] = torch.zeros_like(kw["means3D"], requires_grad=True)
    img, radii = GaussianRasterizer(rs)(**kw)
    (img * _cuda(sc["g"])).sum().backward()
    gname = dict(means3D="dL_dmeans3D", means2D="dL_dmeans2D", opacities="dL_dopacity",
                 shs="dL_dsh", colors_precomp="dL_dcolors", scales="dL_dscales",
                 rotations="dL_drotations", cov3D_precomp="dL_dcov3D")
    out = {gname[k]: v.grad.detach().cpu().numpy() for k, v in kw.items()}
    out["color"], out["radii"] = img.detach().cpu().numpy(), radii.cpu().numpy()
    out["rs"] = rs
    out["kw"] = {k: v.detach() for k, v in kw.items() if k != "means2D"}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAIN)
def test_hip_forward_bitexact_vs_oracle(name):
    got, o = gpu_run(name), oracle_run(name)
    np.testing.assert_array_equal(got["radii"], o["radii"])
    np.testing.assert_array_equal(got["color"], o["color"])


@pytest.mark.gpu
def test_hip_sh3_deferred_and_per_tile_binning_bitexact():
    import diff_gaussian_rasterization as dgr
    from splatt3r_amd import _lib
    got, o = gpu_run("sh3"), oracle_run("sh3")
    c, r, info = dgr.rasterize_deferred(got["rs"], capacity=1 << 16, key_bits=32, **got["kw"])
    assert info.tolist()[0] == 0
    np.testing.assert_array_equal(r.cpu().numpy(), o["radii"])
    np.testing.assert_array_equal(c.cpu().numpy(), o["color"])
    _lib.lib().gsr_set_binning(1)
    try:
        kw = dict(got["kw"])
        kw["means2D"] = torch.zeros_like(kw["means3D"])
        img, radii = dgr.GaussianRasterizer(got["rs"])(**kw)
    finally:
        _lib.lib().gsr_set_binning(-1)
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
    np.testing.assert_array_equal(img.cpu().numpy(), o["color"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAIN)
def test_hip_backward_vs_oracle(name, parity):
    got, o = gpu_run(name), oracle_run(name)
    errs = {n: rel_err(got[n], o[n]) for n in oracle_names(scene(name)["cfg"]) if n in got}
    for n, e in errs.items():
        parity(f"grad_oracle_{name}_{n}", max_rel=e, tol=BWD_TOL)
    for n, e in errs.items():
        assert e <= BWD_TOL, (name, n, e)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAIN)
def test_hip_backward_vs_float64_reference(name, parity):
    """Every gradient the autograd surface returns for the case, against the
    float64 autograd reference; over the cases all eight outputs of
    gsr_backward are covered."""
    got, sc = gpu_run(name), scene(name)
    d = float(np.abs(got["color"] - sc["ref"]["color"])[:, sc["ok_px"]].max())
    parity(f"grad_ref64_{name}_image", max_abs=d, tol=TOL["image"])
    errs = {n: rel_err(got[n], sc["ref"][n]) for n in R64.GRAD_NAMES if n in got}
    assert len(errs) == 5 + (sc["cfg"]["cov"] == "sr")
    for n, e in errs.items():
        parity(f"grad_ref64_{name}_{n}", max_rel=e, tol=TOL[n])
    assert d <= TOL["image"], (name, "image", d)
    for n, e in errs.items():
        assert e <= TOL[n], (name, n, e)


def _gsr_backward_direct(name):
    """include/gsr.h called as the autograd wrapper calls it, but returning all
    eight gradient outputs, from buffers pre-filled with NaN ("caller-zeroed
    not required; every output is written")."""
    import ctypes
    import diff_gaussian_rasterization as dgr
    from splatt3r_amd import _lib
    sc, got = scene(name), gpu_run(name)
    dev = torch.device("cuda")
    t = {k: v.contiguous() for k, v in got["kw"].items()}
    P = t["means3D"].shape[0]
    M = t["shs"].shape[1] if "shs" in t else 0
    s, keep = dgr._settings_struct(got["rs"], dev)
    L, stream = _lib.lib(), _lib.stream(dev)
    p = lambda k: _lib.ptr(t.get(k))
    u8 = lambda n: torch.empty(int(n), device=dev, dtype=torch.uint8)
    radii = torch.empty(P, device=dev, dtype=torch.int32)
    color = torch.empty(3, H, W, device=dev, dtype=torch.float32)
    geom, img = u8(L.gsr_geom_bytes(P)), u8(L.gsr_image_bytes(H, W))
    nr = ctypes.c_int64(0)
    _lib.check(L.gsr_preprocess(ctypes.byref(s), P, M, p("means3D"), p("scales"), p("rotations"),
                                p("cov3D_precomp"), p("shs"), p("colors_precomp"), p("opacities"),
                                radii.data_ptr(), geom.data_ptr(), ctypes.byref(nr), stream),
               "gsr_preprocess")
    binning = u8(L.gsr_binning_bytes(nr.value))
    _lib.check(L.gsr_render(ctypes.byref(s), P, nr.value, radii.data_ptr(), geom.data_ptr(),
                            binning.data_ptr(), img.data_ptr(), color.data_ptr(), stream),
               "gsr_render")
    g = _cuda(sc["g"])
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=torch.float32)
    o = dict(dL_dmeans2D=nan(P, 3), dL_dconic=nan(P, 4), dL_dopacity=nan(P, 1),
             dL_dcolors=nan(P, 3), dL_dmeans3D=nan(P, 3), dL_dcov3D=nan(P, 6),
             dL_dsh=nan(P, M, 3) if M else None,
             dL_dscales=nan(P, 3) if "scales" in t else None,
             dL_drotations=nan(P, 4) if "scales" in t else None)
    _lib.check(L.gsr_backward(
        ctypes.byref(s), P, M, nr.value, p("means3D"), p("scales"), p("rotations"),
        p("cov3D_precomp"), p("shs"), p("colors_precomp"), p("opacities"), radii.data_ptr(),
        geom.data_ptr(), binning.data_ptr(), img.data_ptr(), g.data_ptr(),
        *[_lib.ptr(o[k]) for k in ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors",
                                   "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
                                   "dL_drotations")], stream), "gsr_backward")
    torch.cuda.synchronize()
    del keep
    return color.cpu().numpy(), {k: v.cpu().numpy() for k, v in o.items() if v is not None}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scale_rot", "sh2", "culled"])
def test_hip_gsr_backward_outputs_the_wrapper_drops(name, parity):
    """dL_dcov3D on the scale / rotation path and dL_dcolors on the SH path
    are computed by gsr_backward but not returned through autograd: read them
    from the C entry point, with every output buffer pre-filled with NaN."""
    color, o = _gsr_backward_direct(name)
    sc = scene(name)
    np.testing.assert_array_equal(color, oracle_run(name)["color"])
    for n, a in o.items():
        assert np.isfinite(a).all(), n
    errs = {n: rel_err(o[n], sc["ref"][n]) for n in R64.GRAD_NAMES if n in o}
    assert len(errs) == 6 + (sc["cfg"]["cov"] == "sr")
    for n, e in errs.items():
        parity(f"gsr_direct_ref64_{name}_{n}", max_rel=e, tol=TOL[n])
    for n, e in errs.items():
        assert e <= TOL[n], (name, n, e)
    for n in ("dL_dcolors", "dL_dcov3D"):
        assert rel_err(o[n], oracle_run(name)[n]) <= BWD_TOL, n
    dead = ~sc["ref"]["visible"]
    for n, a in o.items():
        assert np.all(a[dead] == 0.0), n


@pytest.mark.gpu
def test_hip_culled_gaussians_get_exactly_zero_gradient():
    got, sc = gpu_run("culled"), scene("culled")
    dead = ~sc["ref"]["visible"]
    assert dead.sum() >= 30 and np.all(got["radii"][dead] == 0)
    for n in R64.GRAD_NAMES:
        if n in got:
            assert np.all(got[n][dead] == 0.0), n
