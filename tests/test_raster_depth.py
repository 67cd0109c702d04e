"""Depth and accumulated opacity from the rasterizer's blend pass
(include/gsr.h gsr_render_depth / gsr_forward_deferred_depth /
gsr_backward_depth; GaussianRasterizer(..., return_depth=True)).

  depth = sum z_i alpha_i T_i      alpha = sum alpha_i T_i

with the colour blend's own alpha_i, T_i, skip rules and stop rule, z_i the
Gaussian's view-space z, no background term.

Reference without new derivative code: the float64 autograd reference
(tests/raster_ref64.py) renders colours, so depth and alpha are its channels
0 and 1 for colors_precomp = (z64, 1, 0), bg = 0, z64 = m @ Rw[2] + tw[2] in
float64 from the float32 inputs.  With ref1 the scene's colour run (dL_dout =
g) and ref2 that second run (dL_dout = (g_d, g_a, 0)), the loss
sum(g C) + sum(g_d depth) + sum(g_a alpha) is linear in the three output
gradients, so the expected gradients are ref1 + ref2 for every geometric
tensor, ref1 alone for the colour tensors, and for dL_dmeans3D the chain
through z: + ref2.dL_dcolors[:, 0:1] * Rw[2].  g_d and g_a are zeroed at the
scene's fragile pixels like g; images are compared on the other pixels.

Bit-exact checks use no tolerance: the oracle (oracle/raster_ref.c) fed the
kernel's own view_z as a colour channel blends exactly what the depth
variant blends.

Floors and tolerances (rule of tests/test_raster_grad.py: floor = float32
rounding measured WITHOUT the kernel, tol = 4 x floor rounded up to one
significant digit).  The floor of the new tensors is the same composition
run with dtype=float32 against float64 (test_float32_floor_of_composition
prints it; worst case over GRAD_SCENES); for gradient tensors the larger of
that and the FLOOR entry of test_raster_grad.py counts.  Images: max|a - b|
on the non-fragile pixels; gradients: max|a - b| / max|ref|.

  tensor         float32 floor  worst case  FLOOR     tol
  depth          1.7e-6         view        -         7e-06
  alpha          5.2e-7         view        -         3e-06
  dL_dmeans2D    1.5e-6         view        2.0e-6    8e-06
  dL_dopacity    1.1e-6         culled      1.3e-6    6e-06
  dL_dcolors     1.7e-6         culled      1.7e-6    7e-06
  dL_dmeans3D    1.5e-6         culled      1.9e-6    8e-06
  dL_dcov3D      1.7e-6         scale_rot   2.2e-6    9e-06
  dL_dsh         4.8e-7         jclamp      1.3e-6    6e-06
  dL_dscales     1.0e-6         scale_rot   1.6e-6    7e-06
  dL_drotations  6.5e-7         scale_rot   7.2e-7    3e-06
(floors rounded up to two digits, as measured on the build host; a host with
another vector ISA sums float32 in another order and reads up to 2.7e-6 on
dL_dmeans2D / 2.4e-6 on dL_dmeans3D of `culled`: the test asserts <= tol)
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import oracle
import raster_ref64 as R64
from conftest import REPO
from splatt3r_amd.synthetic import (identity_camera_settings, raster_grad, settings_to_dict)
from test_raster import BWD_TOL, small_scene
from test_raster_grad import (CASES, FLOOR, H, MAIN, TOL, W, _roundup_1sig, camera, rel_err,
                              scene)

# scenes of the backward test (CASES of test_raster_grad.py)
GRAD_SCENES = ("view", "scale_rot", "sh2", "jclamp", "sat", "culled")
# dL/d depth has the scale of dL/d colour (unit normal): the depth-to-mean
# term then moves dL_dmeans3D by > 50 x tol (test_scene_is_sensitive_to_z_term)
G_D_SCALE = 1.0

#                float32 floor of the composition (measured, two digits up)
DFLOOR = {
    "depth":          1.7e-6,
    "alpha":          5.2e-7,
    "dL_dmeans2D":    1.5e-6,
    "dL_dopacity":    1.1e-6,
    "dL_dcolors":     1.7e-6,
    "dL_dmeans3D":    1.5e-6,
    "dL_dcov3D":      1.7e-6,
    "dL_dsh":         4.8e-7,
    "dL_dscales":     1.0e-6,
    "dL_drotations":  6.5e-7,
}
DTOL = {k: _roundup_1sig(4.0 * max(v, FLOOR.get(k, 0.0))) for k, v in DFLOOR.items()}

SUMMED = ("dL_dmeans2D", "dL_dopacity", "dL_dcov3D", "dL_dscales", "dL_drotations")
COLOUR_ONLY = ("dL_dsh", "dL_dcolors")


# ------------------------------------------------------------- composition
def _geometry(inp):
    return {k: v for k, v in inp.items() if k not in ("shs", "colors_precomp")}


def _view_rows(sd):
    vm = np.asarray(sd["viewmatrix"], np.float64).reshape(4, 4)
    return vm, vm[:3, :3].T, vm[3, :3]


@functools.lru_cache(maxsize=None)
def pixel_grads(name):
    """(g_d, g_a) [H, W] float32, seeds of their own, zero at fragile pixels."""
    sc = scene(name)
    seed = CASES[name]["seed"]
    g_d = raster_grad(H, W, seed=200 + seed)[0] * np.float32(G_D_SCALE)
    g_a = raster_grad(H, W, seed=300 + seed)[0].copy()
    g_d[sc["ref"]["fragile_px"]] = 0.0
    g_a[sc["ref"]["fragile_px"]] = 0.0
    return g_d, g_a


def _fake_run(name, dtype, with_grad=True):
    """The reference on colours (z64, 1, 0) with bg = 0."""
    sc = scene(name)
    _, Rw, tw = _view_rows(sc["sd"])
    z64 = np.asarray(sc["inp"]["means3D"], np.float64) @ Rw[2] + tw[2]
    col = np.stack([z64, np.ones_like(z64), np.zeros_like(z64)], 1)
    sd0 = dict(sc["sd"], bg=np.zeros(3))
    kw = {}
    if with_grad:
        g_d, g_a = pixel_grads(name)
        kw["dL_dout"] = np.stack([g_d, g_a, np.zeros_like(g_d)])
    return R64.render(sd0, **_geometry(sc["inp"]), colors_precomp=col, dtype=dtype, **kw), z64


def _compose(sc, ref1, ref2, z_term=True):
    _, Rw, _ = _view_rows(sc["sd"])
    out = dict(depth=ref2["color"][0], alpha=ref2["color"][1])
    for n in SUMMED:
        if n in ref1:
            out[n] = ref1[n] + ref2[n]
    for n in COLOUR_ONLY:
        if n in ref1:
            out[n] = ref1[n]
    out["dL_dmeans3D"] = ref1["dL_dmeans3D"] + ref2["dL_dmeans3D"]
    if z_term:
        out["dL_dmeans3D"] = out["dL_dmeans3D"] + ref2["dL_dcolors"][:, 0:1] * Rw[2][None]
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """Float64 expectation of one scene (computed once; read-only)."""
    sc = scene(name)
    ref2, z64 = _fake_run(name, torch.float64)
    out = _compose(sc, sc["ref"], ref2)
    out["z64"], out["ref2"] = z64, ref2
    return out


def _returned(name):
    """Gradient names the autograd surface returns for the case."""
    cfg = CASES[name]
    n = ["dL_dmeans2D", "dL_dopacity", "dL_dmeans3D"]
    n.append("dL_dsh" if cfg["color"] == "sh" else "dL_dcolors")
    n += ["dL_dcov3D"] if cfg["cov"] == "pre" else ["dL_dscales", "dL_drotations"]
    return n


# --------------------------------------------------------------- CPU tests
NEW_SYMBOLS = ("gsr_render_depth", "gsr_forward_deferred_depth", "gsr_backward_depth")


def test_library_exports_and_binds_the_depth_entry_points():
    import diff_gaussian_rasterization  # noqa: F401  (registers the signatures)
    from splatt3r_amd import _lib
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), f"{n} not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    header = open(f"{REPO}/include/gsr.h").read()
    for n in NEW_SYMBOLS:
        assert f"int {n}(" in header


def test_workspace_sizes_are_unchanged():
    """gsr_geom_bytes / gsr_image_bytes / gsr_binning_bytes: the layout
    formulas restated (256-B aligned carve of the existing fields)."""
    import diff_gaussian_rasterization  # noqa: F401
    from splatt3r_amd import _lib
    L = _lib.lib()
    al = lambda n: (n + 255) // 256 * 256
    cdiv = lambda a, b: -(-a // b)
    for P in (1, 206, 5000, 1 << 20):
        segs = max(1, cdiv(P, 4096))
        want = (2 * al(16 * P) + al(4 * P) + al(P) + al(16 * P) + al(64 * 64) + 4 * al(4 * P) +
                al(4 * 512 * segs) + al(4 * 512) + al(16 * P) + al(4 * max(1, cdiv(P, 512))) +
                al(16))
        assert L.gsr_geom_bytes(P) == want, P
        assert L.gsr_binning_bytes(P) == 4 * al(4 * P) + al(4 * 512 * segs) + al(4 * 512)
    for h, w in ((41, 59), (540, 960)):
        tiles = cdiv(w, 16) * cdiv(h, 16)
        assert L.gsr_image_bytes(h, w) == al(8 * tiles) + al(4 * tiles) + 2 * al(4 * h * w)


@pytest.mark.parametrize("name", MAIN)
def test_reference_alpha_telescopes(name):
    """sum alpha_i T_i + T_final = 1: the alpha channel of the composition
    plus the T_final image (zero colours, bg = 1) is 1 to 1e-12."""
    sc = scene(name)
    ref2, z64 = _fake_run(name, torch.float64, with_grad=False)
    tfin = R64.render(dict(sc["sd"], bg=np.ones(3)), **_geometry(sc["inp"]),
                      colors_precomp=np.zeros((len(z64), 3)))["color"][0]
    e = float(np.abs(ref2["color"][1] + tfin - 1.0).max())
    print(f"telescoping {name}: {e:.3e}")
    assert e <= 1e-12
    assert ref2["color"][1].max() > 0.5 and ref2["color"][0].max() > 1.0
    assert np.all(ref2["color"][2] == 0.0)


@pytest.mark.parametrize("name", GRAD_SCENES)
def test_scene_is_sensitive_to_z_term(name):
    """A kernel that dropped dL_dz_i (vm[2], vm[6], vm[10]) would miss the
    dL_dmeans3D tolerance by >= 50x."""
    sc, ex = scene(name), expected(name)
    cut = _compose(sc, sc["ref"], ex["ref2"], z_term=False)
    e = rel_err(cut["dL_dmeans3D"], ex["dL_dmeans3D"])
    print(f"sensitivity {name} z term: {e:.3e} = {e / DTOL['dL_dmeans3D']:.0f} x tol")
    assert e >= 50.0 * DTOL["dL_dmeans3D"]
    assert e >= 50.0 * TOL["dL_dmeans3D"]


@pytest.mark.parametrize("name", GRAD_SCENES)
def test_float32_floor_of_composition(name, parity):
    """Rounding floor of the new tensors: the composition in float32 against
    itself in float64 (the way test_float32_floor measures)."""
    sc, ex = scene(name), expected(name)
    r1 = R64.render(sc["sd"], **sc["inp"], dL_dout=sc["g"], dtype=torch.float32)
    r2, _ = _fake_run(name, torch.float32)
    np.testing.assert_array_equal(r1["radii"], sc["ref"]["radii"])
    np.testing.assert_array_equal(r2["radii"], sc["ref"]["radii"])
    got = _compose(sc, r1, r2)
    ok = sc["ok_px"]
    errs = {"depth": float(np.abs(got["depth"] - ex["depth"])[ok].max()),
            "alpha": float(np.abs(got["alpha"] - ex["alpha"])[ok].max())}
    for n in R64.GRAD_NAMES:
        if n in got:
            errs[n] = rel_err(got[n], ex[n])
    for n, e in errs.items():
        print(f"floor32 depth {name} {n} {e:.3e}")
        parity(f"depth_ref64_ref32_{name}_{n}", max_err=e, tol=DTOL[n])
    for n, e in errs.items():
        assert e <= DTOL[n], (name, n, e)


# --------------------------------------------------------------- GPU tests
def _cuda(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(grad)


GNAME = dict(means3D="dL_dmeans3D", means2D="dL_dmeans2D", opacities="dL_dopacity",
             shs="dL_dsh", colors_precomp="dL_dcolors", scales="dL_dscales",
             rotations="dL_drotations", cov3D_precomp="dL_dcov3D")


def _leaves(inp):
    kw = {k: _cuda(v, True) for k, v in inp.items()}
    kw["means2D"] = torch.zeros_like(kw["means3D"], requires_grad=True)
    return kw


def _grads(kw):
    return {GNAME[k]: v.grad.detach().cpu().numpy() for k, v in kw.items() if v.grad is not None}


@functools.lru_cache(maxsize=None)
def gpu_depth_run(name):
    """One return_depth=True forward + fused backward per case."""
    import diff_gaussian_rasterization as dgr
    sc = scene(name)
    rs = camera(sc["cfg"]["D"], sc["cfg"].get("mod", 1.0), "cuda")
    kw = _leaves(sc["inp"])
    img, radii, depth, alpha = dgr.GaussianRasterizer(rs)(**kw, return_depth=True)
    view_z = dgr.last_view_z
    g_d, g_a = pixel_grads(name)
    ((img * _cuda(sc["g"])).sum() + (depth * _cuda(g_d)).sum() +
     (alpha * _cuda(g_a)).sum()).backward()
    out = _grads(kw)
    out.update(color=img.detach().cpu().numpy(), radii=radii.cpu().numpy(),
               depth=depth.detach().cpu().numpy(), alpha=alpha.detach().cpu().numpy(),
               view_z=view_z.cpu().numpy(), rs=rs,
               kw={k: v.detach() for k, v in kw.items()})
    return out


@functools.lru_cache(maxsize=None)
def gpu_colour_run(name):
    """The existing colour path (return_depth=False) with the same loss on
    colour."""
    import diff_gaussian_rasterization as dgr
    sc = scene(name)
    rs = camera(sc["cfg"]["D"], sc["cfg"].get("mod", 1.0), "cuda")
    kw = _leaves(sc["inp"])
    img, radii = dgr.GaussianRasterizer(rs)(**kw)
    (img * _cuda(sc["g"])).sum().backward()
    out = _grads(kw)
    out.update(color=img.detach().cpu().numpy(), radii=radii.cpu().numpy())
    return out


SMALL = {"small2000": (2000, 0, "shs"), "small5000": (5000, 1, "colors"), "one": (1, 2, "shs")}


def _small_inputs(key, grad=False):
    """The small_scene cases of test_raster.py as rasterizer inputs."""
    P, seed, mode = SMALL[key]
    sc = small_scene(P, seed)
    rs, scale = identity_camera_settings(sc["K"], sc["H"], sc["W"], "cuda")
    inp = dict(means3D=sc["means"] * scale, opacities=sc["opacities"],
               cov3D_precomp=sc["cov6"] * scale * scale)
    if mode == "shs":
        inp["shs"] = sc["shs"]
    else:
        inp["colors_precomp"] = np.clip(sc["shs"][:, 0, :] + 0.5, 0, 1)
    inp = {k: np.ascontiguousarray(v, np.float32) for k, v in inp.items()}
    return rs, inp


def _fake_colours(view_z):
    return np.stack([view_z, np.ones_like(view_z), np.zeros_like(view_z)], 1).astype(np.float32)


def _check_depth_bitexact(rs, inp, depth, alpha, view_z):
    """depth / alpha == channels 0 / 1 of the oracle and of the HIP colour
    path on colours (view_z, 1, 0) with bg = 0."""
    import diff_gaussian_rasterization as dgr
    sd0 = dict(settings_to_dict(rs), bg=np.zeros(3, np.float32))
    fake = _fake_colours(view_z)
    o = oracle.raster(sd0, **_geometry(inp), colors_precomp=fake)
    np.testing.assert_array_equal(depth, o["color"][0])
    np.testing.assert_array_equal(alpha, o["color"][1])
    rs0 = rs._replace(bg=torch.zeros(3, device="cuda"))
    kw = {k: _cuda(v) for k, v in _geometry(inp).items()}
    img, _ = dgr.GaussianRasterizer(rs0)(means2D=torch.zeros_like(kw["means3D"]),
                                         colors_precomp=_cuda(fake), **kw)
    img = img.cpu().numpy()
    np.testing.assert_array_equal(depth, img[0])
    np.testing.assert_array_equal(alpha, img[1])
    assert np.all(img[2] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAIN)
def test_hip_colour_untouched_and_depth_bitexact(name):
    """return_depth=True: colour and radii are those of return_depth=False
    bit for bit; depth and alpha are the oracle's blend of the kernel's own
    view_z (rotated, translated camera)."""
    got, base, sc = gpu_depth_run(name), gpu_colour_run(name), scene(name)
    np.testing.assert_array_equal(got["radii"], base["radii"])
    np.testing.assert_array_equal(got["color"], base["color"])
    assert got["depth"].shape == (H, W) and got["alpha"].shape == (H, W)
    assert got["alpha"].max() > 0.5 and got["depth"].max() > 1.0
    _check_depth_bitexact(got["rs"], sc["inp"], got["depth"], got["alpha"], got["view_z"])


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(SMALL))
def test_hip_small_scenes_colour_untouched_and_depth_bitexact(key):
    """Several staging rounds per tile and the early stop (2000 / 5000
    Gaussians at 48 x 64), and P = 1; identity camera: view_z is means z."""
    import diff_gaussian_rasterization as dgr
    rs, inp = _small_inputs(key)
    kw = {k: _cuda(v) for k, v in inp.items()}
    kw["means2D"] = torch.zeros_like(kw["means3D"])
    img0, radii0 = dgr.GaussianRasterizer(rs)(**kw)
    if key == "small5000":
        assert dgr.last_num_rendered > 12 * 256      # 12 tiles: > 1 staging round on average
    img, radii, depth, alpha = dgr.GaussianRasterizer(rs)(**kw, return_depth=True)
    view_z = dgr.last_view_z.cpu().numpy()
    assert torch.equal(img, img0) and torch.equal(radii, radii0)
    np.testing.assert_array_equal(view_z, inp["means3D"][:, 2])
    _check_depth_bitexact(rs, inp, depth.cpu().numpy(), alpha.cpu().numpy(), view_z)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAIN)
def test_hip_view_z_vs_float64(name):
    """Three products and three sums, each rounded once: |view_z - z64| <=
    8 * 2^-24 * (|vm2 x| + |vm6 y| + |vm10 z| + |vm14|) (factor 2 of slack),
    culled Gaussians included."""
    got, sc = gpu_depth_run(name), scene(name)
    vm, Rw, tw = _view_rows(sc["sd"])
    m = np.asarray(sc["inp"]["means3D"], np.float64)
    z64 = m @ Rw[2] + tw[2]
    mag = np.abs(m * Rw[2][None]).sum(1) + abs(tw[2])
    assert got["view_z"].shape == (m.shape[0],)
    err = np.abs(got["view_z"].astype(np.float64) - z64)
    print(f"view_z {name}: worst {float((err / mag).max()) * 2 ** 24:.2f} x 2^-24")
    assert np.all(err <= 8.0 * 2.0 ** -24 * mag)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(SMALL))
def test_hip_deferred_depth_equals_two_call(key):
    """gsr_forward_deferred_depth == gsr_preprocess + gsr_render_depth bit
    for bit when the frame fits; too small a capacity sets status bit 0."""
    import diff_gaussian_rasterization as dgr
    rs, inp = _small_inputs(key)
    kw = {k: _cuda(v) for k, v in inp.items()}
    img, radii, depth, alpha = dgr.GaussianRasterizer(rs)(
        means2D=torch.zeros_like(kw["means3D"]), **kw, return_depth=True)
    R = dgr.last_num_rendered
    view_z = dgr.last_view_z.clone()
    for cap, bits in ((R + 1000, 32), (max(R, 1), 32), (2 * R + 1, 24)):
        c, r, info, d, a = dgr.rasterize_deferred(rs, capacity=cap, key_bits=bits,
                                                  return_depth=True, **kw)
        st, tot, live = info.tolist()
        assert tot == R and live <= 32
        if live <= bits:
            assert st == 0, (cap, bits, st)
            assert torch.equal(c, img) and torch.equal(r, radii)
            assert torch.equal(d, depth) and torch.equal(a, alpha)
            assert torch.equal(dgr.last_view_z, view_z)
    # the colour-only deferred forward is the same image
    c, r, info = dgr.rasterize_deferred(rs, capacity=R + 1000, key_bits=32, **kw)
    assert info.tolist()[0] == 0 and torch.equal(c, img)
    if R > 1:
        out = dgr.rasterize_deferred(rs, capacity=R // 2, key_bits=32, return_depth=True, **kw)
        assert len(out) == 5 and out[2].tolist()[0] & 1


def _assert_all_zero(grads, rows=slice(None)):
    for n, a in grads.items():
        assert np.all(a[rows] == 0.0), n


@pytest.mark.gpu
def test_hip_no_gaussians():
    """P = 0: depth and alpha are zero, colour is the background, the
    backward runs and returns (empty) zeros."""
    import diff_gaussian_rasterization as dgr
    rs = camera(0, 1.0, "cuda")
    z = lambda *s: torch.zeros(*s, device="cuda", requires_grad=True)
    kw = dict(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), shs=z(0, 1, 3),
              cov3D_precomp=z(0, 6))
    img, radii, depth, alpha = dgr.GaussianRasterizer(rs)(**kw, return_depth=True)
    assert radii.shape == (0,)
    assert torch.all(depth == 0) and torch.all(alpha == 0)
    assert depth.shape == (H, W) and alpha.shape == (H, W)
    assert torch.equal(img, rs.bg.reshape(3, 1, 1).expand(3, H, W))
    (img.sum() + depth.sum() + alpha.sum()).backward()
    for k in ("means3D", "means2D", "opacities"):
        assert kw[k].grad is not None and kw[k].grad.shape == kw[k].shape, k
    # the sync-free entry point (an empty tensor has no address: dummies
    # stand in for the unused SH / covariance arrays)
    from splatt3r_amd import _lib
    L, dev = _lib.lib(), torch.device("cuda")
    s, keep = dgr._settings_struct(rs, dev)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    c, d, a, dummy = nan(3, H, W), nan(H, W), nan(H, W), nan(16)
    u8 = lambda n: torch.empty(int(n), device=dev, dtype=torch.uint8)
    geom, img_ws, binning = u8(L.gsr_geom_bytes(0)), u8(L.gsr_image_bytes(H, W)), u8(
        L.gsr_binning_bytes(16))
    info = torch.full((3,), -1, device=dev, dtype=torch.int64)
    _lib.check(L.gsr_forward_deferred_depth(
        ctypes.byref(s), 0, 1, None, None, None, dummy.data_ptr(), dummy.data_ptr(), None, None,
        None, geom.data_ptr(), binning.data_ptr(), 16, 32, img_ws.data_ptr(), c.data_ptr(),
        d.data_ptr(), a.data_ptr(), None, info.data_ptr(), _lib.stream(dev)),
        "gsr_forward_deferred_depth")
    assert info.tolist() == [0, 0, 0] and torch.equal(c, img.detach())
    assert torch.all(d == 0) and torch.all(a == 0)
    del keep


@pytest.mark.gpu
def test_hip_all_culled():
    """Only the culled Gaussians of the `culled` scene (behind, near, off
    screen): zero depth and alpha, background colour, zero gradients."""
    import diff_gaussian_rasterization as dgr
    sc = scene("culled")
    dead = ~sc["ref"]["visible"]
    assert dead.sum() >= 30
    rs = camera(0, 1.0, "cuda")
    kw = _leaves({k: v[dead] for k, v in sc["inp"].items()})
    img, radii, depth, alpha = dgr.GaussianRasterizer(rs)(**kw, return_depth=True)
    assert torch.all(radii == 0)
    assert torch.all(depth == 0) and torch.all(alpha == 0)
    assert torch.equal(img, rs.bg.reshape(3, 1, 1).expand(3, H, W))
    g_d, g_a = pixel_grads("culled")
    ((img * _cuda(sc["g"])).sum() + (depth * _cuda(g_d)).sum() +
     (alpha * _cuda(g_a)).sum()).backward()
    grads = _grads(kw)
    assert len(grads) == 5
    _assert_all_zero(grads)


@pytest.mark.gpu
def test_hip_culled_gaussians_get_exactly_zero_gradient_with_depth():
    got, sc = gpu_depth_run("culled"), scene("culled")
    g_d, g_a = pixel_grads("culled")
    assert np.abs(g_d).max() > 1 and np.abs(g_a).max() > 1
    dead = ~sc["ref"]["visible"]
    assert dead.sum() >= 30 and np.all(got["radii"][dead] == 0)
    grads = {n: got[n] for n in _returned("culled")}
    _assert_all_zero(grads, dead)
    assert all(np.abs(a).max() > 0 for a in grads.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAD_SCENES)
def test_hip_depth_backward_vs_float64_composition(name, parity):
    """Depth and alpha images and every gradient the autograd surface returns,
    for the loss sum(g C) + sum(g_d depth) + sum(g_a alpha)."""
    got, sc, ex = gpu_depth_run(name), scene(name), expected(name)
    ok = sc["ok_px"]
    errs = {"depth": float(np.abs(got["depth"] - ex["depth"])[ok].max()),
            "alpha": float(np.abs(got["alpha"] - ex["alpha"])[ok].max())}
    names = _returned(name)
    assert all(n in got for n in names) and len(names) == 5 + (sc["cfg"]["cov"] == "sr")
    for n in names:
        errs[n] = rel_err(got[n], ex[n])
    for n, e in errs.items():
        print(f"depth_ref64 {name} {n} {e:.3e} (tol {DTOL[n]:.0e})")
        parity(f"depth_ref64_{name}_{n}", max_err=e, tol=DTOL[n])
    for n, e in errs.items():
        assert e <= DTOL[n], (name, n, e)


def _hip_backward(rs, inp, losses, return_depth):
    """Gradients of sum_k sum(out_k * g_k) through the autograd surface;
    losses: {output index: g}."""
    import diff_gaussian_rasterization as dgr
    kw = _leaves(inp)
    out = dgr.GaussianRasterizer(rs)(**kw, return_depth=return_depth)
    sum((out[k] * _cuda(g)).sum() for k, g in losses.items()).backward()
    return _grads(kw), out


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["small2000", "small5000"])
def test_hip_fused_backward_at_several_staging_rounds(key, parity):
    """small_scene(2000, 0) (and (5000, 1): more than one 256-record staging
    round in every tile): the fused backward (colour + depth + alpha
    gradients in one call) against two colour backwards of the existing
    kernels (colour with g_c; colours (view_z, 1, 0) with (g_d, g_a, 0)) plus
    the z term from the second one's dL_dcolors[:, 0]."""
    import diff_gaussian_rasterization as dgr
    rs, inp = _small_inputs(key)
    Hs, Ws = rs.image_height, rs.image_width
    g_c = raster_grad(Hs, Ws, seed=7)
    g_d, g_a = raster_grad(Hs, Ws, seed=8)[0], raster_grad(Hs, Ws, seed=9)[0]
    fused, _ = _hip_backward(rs, inp, {0: g_c, 2: g_d, 3: g_a}, True)
    view_z = dgr.last_view_z.cpu().numpy()
    first, _ = _hip_backward(rs, inp, {0: g_c}, False)
    inp2 = dict(_geometry(inp), colors_precomp=_fake_colours(view_z))
    rs0 = rs._replace(bg=torch.zeros(3, device="cuda"))
    second, _ = _hip_backward(rs0, inp2, {0: np.stack([g_d, g_a, np.zeros_like(g_d)])}, False)
    vm = rs.viewmatrix.detach().cpu().numpy().astype(np.float64).reshape(4, 4)
    want = {n: first[n].astype(np.float64) + second[n] for n in
            ("dL_dmeans2D", "dL_dopacity", "dL_dcov3D", "dL_dmeans3D")}
    z_term = second["dL_dcolors"][:, 0:1].astype(np.float64) * vm[:3, 2][None]
    # without the z term the comparison below would miss by >= 50 x the bar
    assert rel_err(want["dL_dmeans3D"], want["dL_dmeans3D"] + z_term) >= 50.0 * BWD_TOL
    want["dL_dmeans3D"] = want["dL_dmeans3D"] + z_term
    cname = "dL_dsh" if "shs" in inp else "dL_dcolors"
    want[cname] = first[cname]
    for n, w in want.items():
        e = rel_err(fused[n], w)
        parity(f"depth_fused_vs_two_pass_{key}_{n}", max_rel=e, tol=BWD_TOL)
        assert e <= BWD_TOL, (n, e)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["view", "scale_rot"])
def test_hip_unused_depth_outputs_take_the_colour_backward(name):
    """return_depth=True with a loss on colour only: the gradients of the
    return_depth=False call (same kernels, float atomics reorder sums)."""
    from splatt3r_amd import _lib
    sc = scene(name)
    rs = camera(sc["cfg"]["D"], sc["cfg"].get("mod", 1.0), "cuda")
    L = _lib.lib()
    depth_entry = L.gsr_backward_depth

    def refuse(*a):
        raise AssertionError("gsr_backward_depth called without a depth or alpha gradient")

    L.gsr_backward_depth = refuse
    try:
        got, _ = _hip_backward(rs, sc["inp"], {0: sc["g"]}, True)
    finally:
        L.gsr_backward_depth = depth_entry
    base = gpu_colour_run(name)
    assert set(got) == set(_returned(name))
    for n, a in got.items():
        assert rel_err(a, base[n]) <= BWD_TOL, n


@pytest.mark.gpu
def test_hip_loss_on_depth_and_alpha_only():
    """No colour gradient arrives: the loss is linear in the pixel gradients,
    so these gradients are the fused ones minus the colour ones, and the
    colour coefficients get exactly zero."""
    sc = scene("view")
    rs = camera(sc["cfg"]["D"], sc["cfg"].get("mod", 1.0), "cuda")
    g_d, g_a = pixel_grads("view")
    got, _ = _hip_backward(rs, sc["inp"], {2: g_d, 3: g_a}, True)
    fused, colour = gpu_depth_run("view"), gpu_colour_run("view")
    assert np.all(got["dL_dsh"] == 0.0)
    for n in ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D"):
        want = fused[n].astype(np.float64) - colour[n]
        assert np.abs(got[n] - want).max() <= 2 * BWD_TOL * np.abs(fused[n]).max(), n
        assert np.abs(want).max() > 0.1 * np.abs(fused[n]).max(), n


def _gsr_direct(name, variant):
    """include/gsr.h called directly, every output pre-filled with NaN.
    variant: "colour" (gsr_render + gsr_backward), "null" (gsr_render_depth +
    gsr_backward_depth with both new gradients NULL), "depth" (with g_d, g_a)."""
    import diff_gaussian_rasterization as dgr
    from splatt3r_amd import _lib
    sc = scene(name)
    dev = torch.device("cuda")
    rs = camera(sc["cfg"]["D"], sc["cfg"].get("mod", 1.0), "cuda")
    t = {k: _cuda(v) for k, v in sc["inp"].items()}
    P = t["means3D"].shape[0]
    M = t["shs"].shape[1] if "shs" in t else 0
    s, keep = dgr._settings_struct(rs, dev)
    L, stream = _lib.lib(), _lib.stream(dev)
    p = lambda k: _lib.ptr(t.get(k))
    u8 = lambda n: torch.empty(int(n), device=dev, dtype=torch.uint8)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=torch.float32)
    radii = torch.empty(P, device=dev, dtype=torch.int32)
    color, depth, alpha, view_z = nan(3, H, W), nan(H, W), nan(H, W), nan(P)
    geom, img = u8(L.gsr_geom_bytes(P)), u8(L.gsr_image_bytes(H, W))
    nr = ctypes.c_int64(0)
    _lib.check(L.gsr_preprocess(ctypes.byref(s), P, M, p("means3D"), p("scales"), p("rotations"),
                                p("cov3D_precomp"), p("shs"), p("colors_precomp"), p("opacities"),
                                radii.data_ptr(), geom.data_ptr(), ctypes.byref(nr), stream),
               "gsr_preprocess")
    binning = u8(L.gsr_binning_bytes(nr.value))
    if variant == "colour":
        _lib.check(L.gsr_render(ctypes.byref(s), P, nr.value, radii.data_ptr(), geom.data_ptr(),
                                binning.data_ptr(), img.data_ptr(), color.data_ptr(), stream),
                   "gsr_render")
    else:
        _lib.check(L.gsr_render_depth(ctypes.byref(s), P, nr.value, radii.data_ptr(),
                                      geom.data_ptr(), binning.data_ptr(), img.data_ptr(),
                                      p("means3D"), color.data_ptr(), depth.data_ptr(),
                                      alpha.data_ptr(), view_z.data_ptr(), stream),
                   "gsr_render_depth")
    g = _cuda(sc["g"])
    o = dict(dL_dmeans2D=nan(P, 3), dL_dconic=nan(P, 4), dL_dopacity=nan(P, 1),
             dL_dcolors=nan(P, 3), dL_dmeans3D=nan(P, 3), dL_dcov3D=nan(P, 6),
             dL_dsh=nan(P, M, 3) if M else None,
             dL_dscales=nan(P, 3) if "scales" in t else None,
             dL_drotations=nan(P, 4) if "scales" in t else None)
    head = (ctypes.byref(s), P, M, nr.value, p("means3D"), p("scales"), p("rotations"),
            p("cov3D_precomp"), p("shs"), p("colors_precomp"), p("opacities"), radii.data_ptr(),
            geom.data_ptr(), binning.data_ptr(), img.data_ptr())
    outs = [_lib.ptr(o[k]) for k in ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors",
                                     "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
                                     "dL_drotations")]
    if variant == "colour":
        _lib.check(L.gsr_backward(*head, g.data_ptr(), *outs, stream), "gsr_backward")
    else:
        gd = ga = None
        if variant == "depth":
            gd, ga = (_cuda(x) for x in pixel_grads(name))
        o["dL_dz"] = nan(P)
        _lib.check(L.gsr_backward_depth(*head, view_z.data_ptr(), g.data_ptr(), _lib.ptr(gd),
                                        _lib.ptr(ga), *outs, o["dL_dz"].data_ptr(), stream),
                   "gsr_backward_depth")
    torch.cuda.synchronize()
    del keep
    res = {k: v.cpu().numpy() for k, v in o.items() if v is not None}
    res.update(color=color.cpu().numpy(), depth=depth.cpu().numpy(), alpha=alpha.cpu().numpy(),
               view_z=view_z.cpu().numpy())
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sh2", "scale_rot", "culled"])
def test_hip_gsr_backward_depth_direct(name):
    """The C entry points with NaN-filled outputs: both new gradients NULL ==
    gsr_backward within BWD_TOL (dL_dz all zero); with g_d, g_a every output
    is written, dL_dz carries the depth gradient, culled rows are zero, and
    the result is that of the autograd surface."""
    base, null, full = (_gsr_direct(name, v) for v in ("colour", "null", "depth"))
    sc, got = scene(name), gpu_depth_run(name)
    np.testing.assert_array_equal(null["color"], base["color"])
    np.testing.assert_array_equal(null["depth"], got["depth"])
    np.testing.assert_array_equal(null["alpha"], got["alpha"])
    np.testing.assert_array_equal(null["view_z"], got["view_z"])
    assert np.all(null["dL_dz"] == 0.0)
    for n in R64.GRAD_NAMES + ("dL_dconic",):
        if n in base:
            assert np.isfinite(null[n]).all() and np.isfinite(full[n]).all(), n
            assert rel_err(null[n], base[n]) <= BWD_TOL, n
    dead = ~sc["ref"]["visible"]
    for n in R64.GRAD_NAMES + ("dL_dz",):
        if n in full:
            assert np.all(full[n][dead] == 0.0), n
    assert np.abs(full["dL_dz"]).max() > 0
    ex = expected(name)
    assert rel_err(full["dL_dz"], ex["ref2"]["dL_dcolors"][:, 0]) <= DTOL["dL_dcolors"]
    for n in _returned(name):
        assert rel_err(full[n], got[n]) <= BWD_TOL, n


# -------------------------------------------------------------------- glue
def _same_scaled(depth_glue, depth_direct, s):
    """depth_glue is depth_direct / s (one float32 division, so equal bit for
    bit to the same division of the direct call's depth); multiplied back by
    s it is the direct depth to one rounding of each of the two operations."""
    assert torch.equal(depth_glue, depth_direct / s)
    back = depth_glue * s
    assert torch.all((back - depth_direct).abs() <= 2.0 ** -22 * depth_direct.abs())


@pytest.mark.gpu
def test_hip_render_cuda_depth():
    from diff_gaussian_rasterization import GaussianRasterizer
    from splatt3r_amd.render import camera_settings, normalize_intrinsics, render_cuda
    sc = small_scene(2000, 0)
    Hs, Ws = sc["H"], sc["W"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    iu = np.triu_indices(3)
    cov = np.zeros((2000, 3, 3), np.float32)
    cov[:, iu[0], iu[1]] = sc["cov6"]
    cov = cov + np.triu(cov, 1).transpose(0, 2, 1)
    ext = torch.eye(4, device="cuda")[None]
    intr = normalize_intrinsics(t(sc["K"])[None], (Hs, Ws))
    near, far = torch.full((1,), 0.1, device="cuda"), torch.full((1,), 1000.0, device="cuda")
    bg = torch.tensor([[0.1, 0.2, 0.3]], device="cuda")
    args = (ext, intr, near, far, (Hs, Ws), bg, t(sc["means"])[None], t(cov)[None],
            t(sc["shs"]).permute(0, 2, 1)[None].contiguous(), t(sc["opacities"])[None, :, 0])
    base = render_cuda(*args)
    img, depth, alpha = render_cuda(*args, return_depth=True)
    assert torch.equal(img, base)
    assert depth.shape == (1, Hs, Ws) and alpha.shape == (1, Hs, Ws)
    st, scale = camera_settings(ext, intr, near, far, (Hs, Ws), bg, 0)
    s = scale[0]
    assert float(s) == 10.0
    means = t(sc["means"]) * s
    row, col = torch.triu_indices(3, 3)
    c2, _, d2, a2 = GaussianRasterizer(st[0])(
        means3D=means, means2D=torch.zeros_like(means), shs=t(sc["shs"]),
        opacities=t(sc["opacities"]), cov3D_precomp=(t(cov) * s ** 2)[:, row, col],
        return_depth=True)
    assert torch.equal(img[0], c2) and torch.equal(alpha[0], a2)
    _same_scaled(depth[0], d2, s)
    assert 1.0 < float(depth.detach().max()) < 8.0     # caller's units
    # not scale-invariant: the rasterizer's own depth
    img1, depth1, alpha1 = render_cuda(*args, scale_invariant=False, return_depth=True)
    assert torch.equal(img1, render_cuda(*args, scale_invariant=False))
    assert alpha1.shape == alpha.shape
    assert 1.0 < float(depth1.detach().max()) < 8.0     # rasterizer units == caller's here


def _fake_frames(h=24, w=32, seed=3):
    """Two views of Gaussian head outputs in front of an identity pose, as
    splatt3r_render reads them from a frame."""
    import lietorch
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = lambda *sh: torch.rand(*sh, generator=g, device="cuda")

    def view():
        z = 1.0 + 2.0 * u(1, h, w, 1)
        ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"),
                                indexing="ij")
        x = ((xs + 0.5) / w - 0.5)[None, ..., None] * z * 1.2
        y = ((ys + 0.5) / h - 0.5)[None, ..., None] * z * 0.9
        q = torch.nn.functional.normalize(torch.randn(1, h, w, 4, generator=g, device="cuda"),
                                          dim=-1)
        return dict(means=torch.cat([x, y, z], -1), scales=0.01 + 0.04 * u(1, h, w, 3),
                    rotations=q, sh=u(1, h, w, 3, 1) - 0.5, opacities=0.1 + 0.8 * u(1, h, w, 1))

    T = lietorch.Sim3(torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1]], dtype=torch.float32,
                                   device="cuda"))
    frame = types.SimpleNamespace(gaussian_pred=view(), gaussian_pred_cross=view(),
                                  img=u(1, 3, h, w) * 2 - 1, T_WC=T)
    ref_frame = types.SimpleNamespace(img=u(1, 3, h, w) * 2 - 1)
    model = types.SimpleNamespace(decoder=types.SimpleNamespace(
        background_color=torch.tensor([0.1, 0.2, 0.3], device="cuda")))
    return model, frame, ref_frame, (h, w)


@pytest.mark.gpu
def test_hip_splatt3r_render_depth_both_paths():
    """Two-call and sync-free path: colour as the default call, the triple's
    depth / alpha as a direct rasterizer call on the same packed inputs; the
    check rides on the image and its re-render returns the triple."""
    import diff_gaussian_rasterization as dgr
    from splatt3r_amd.render import camera_settings_sim3, pack_splats
    from splatt3r_amd.splatt3r_utils import (RasterSizing, _estimate_default_intrinsics,
                                             splatt3r_render)
    model, f, kf, (h, w) = _fake_frames()
    base = splatt3r_render(model, f, kf)
    img, depth, alpha = splatt3r_render(model, f, kf, return_depth=True)
    assert torch.equal(img, base) and not hasattr(img, "_gsr_check")
    assert img.shape == (1, 1, 3, h, w) and depth.shape == (1, 1, h, w) == alpha.shape
    # the same packed inputs, directly
    K = _estimate_default_intrinsics(h, w, "cpu")
    settings, scale = camera_settings_sim3(f.T_WC.data, f.T_WC.data, K.reshape(-1, 3, 3)[0],
                                           (h, w), model.decoder.background_color, near=0.1,
                                           far=1000.0, sh_degree=0)
    s = float(scale[0])
    views = [dict(means=g["means"].reshape(-1, 3), scales=g["scales"].reshape(-1, 3),
                  rotations=g["rotations"].reshape(-1, 4), sh=g["sh"].reshape(-1, 3, 1),
                  opacities=g["opacities"].reshape(-1, 1), img=im)
             for g, im in ((f.gaussian_pred, f.img), (f.gaussian_pred_cross, kf.img))]
    means, cov6, shs, opac = pack_splats(views, s, img_chw_normalized=True)
    c2, _, d2, a2 = dgr.GaussianRasterizer(settings[0])(
        means3D=means, means2D=torch.zeros_like(means), shs=shs, opacities=opac,
        cov3D_precomp=cov6, return_depth=True)
    assert torch.equal(img[0, 0], c2) and torch.equal(alpha[0, 0], a2)
    _same_scaled(depth[0, 0], d2, s)
    assert float(alpha.max()) > 0.5 and 1.0 < float(depth.max()) < 3.0     # frame units
    # sync-free path
    sizing = RasterSizing()
    first = splatt3r_render(model, f, kf, sizing=sizing, return_depth=True)
    assert sizing.capacity is not None and torch.equal(first[1], depth)
    img3, depth3, alpha3 = splatt3r_render(model, f, kf, sizing=sizing, return_depth=True)
    assert img3._gsr_check.info.tolist()[0] == 0
    assert torch.equal(img3, img) and torch.equal(depth3, depth) and torch.equal(alpha3, alpha)
    plain = splatt3r_render(model, f, kf, sizing=sizing)
    assert torch.equal(plain, base) and plain._gsr_check.info.tolist()[0] == 0
    # capacity too small: status bit 0, the re-render returns the valid triple
    sizing.capacity = max(1, dgr.last_num_rendered // 2)
    bad = splatt3r_render(model, f, kf, sizing=sizing, return_depth=True)
    assert bad[0]._gsr_check.info.tolist()[0] & 1
    again = bad[0]._gsr_check.rerender()
    assert len(again) == 3
    for a, b in zip(again, (img, depth, alpha)):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_hip_render_map_depth():
    """300-Gaussian map at 96 x 64: colour as the default call, depth in world
    units, alpha; against a direct rasterizer call on the scaled map."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from splatt3r_amd.gaussian_map import SharedGaussians, VIZ_BG, render_map, viz_camera
    from splatt3r_amd.synthetic import c5_map_batches
    n, Wm, Hm = 300, 96, 64
    gm = SharedGaussians(max_gaussians=1024, device="cuda")
    for k, b in enumerate(c5_map_batches(n, seed=0, device="cuda")):
        gm.append(*b, kf_idx=k, opacity_threshold=0.3)
    assert gm.n_gaussians == n
    T = np.eye(4, dtype=np.float32)
    cam = viz_camera(T, Wm, Hm, 45.0)
    for clamp in (True, False):
        base = render_map(gm, T, Wm, Hm, 45.0, camera=cam, clamp=clamp)
        img, depth, alpha = render_map(gm, T, Wm, Hm, 45.0, camera=cam, clamp=clamp,
                                       return_depth=True)
        assert torch.equal(img, base)
    assert depth.shape == (Hm, Wm) == alpha.shape
    tx, ty, view_t, proj, campos, s, s2 = cam
    st = GaussianRasterizationSettings(
        image_height=Hm, image_width=Wm, tanfovx=tx, tanfovy=ty,
        bg=torch.tensor(VIZ_BG, dtype=torch.float32, device="cuda"), scale_modifier=1.0,
        viewmatrix=view_t.cuda(), projmatrix=proj.cuda(), sh_degree=0, campos=campos.cuda(),
        prefiltered=False, debug=False)
    means = gm.means[:n] * np.float32(s)
    c2, _, d2, a2 = GaussianRasterizer(st)(
        means3D=means, means2D=torch.zeros_like(means), colors_precomp=gm.colors[:n],
        opacities=gm.opacities[:n, None], cov3D_precomp=gm.cov_triu[:n] * np.float32(s2),
        return_depth=True)
    assert torch.equal(img, c2) and torch.equal(alpha, a2)
    _same_scaled(depth, d2, float(s))
    assert float(alpha.max()) > 0.3 and 2.0 < float(depth.max()) < 6.0     # world units (metres)
