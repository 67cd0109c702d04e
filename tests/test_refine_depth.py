"""Depth-supervised map refinement on the GPU: refine.DepthControl in
refine_splats, SharedGaussians.refine / render_depth_alpha,
Frontend.refine_map(depth=...) and Frontend.eval_depth, on a tiny synthetic
scene: a textured fronto-parallel plane 2 units in front of the first of
three views at 48 x 64, one Gaussian per pixel of that view (and a margin),
seen again from two views that are shifted sideways and towards the plane.
A fronto-parallel plane has one depth per view, whatever the intrinsics:
2.0, 1.8 and 1.9 in each view's own units.

The same scene is built with a Sim3 scale: poses (s R | t) and world points s x
the unit scene.  Depth in a view's own units must not change, which pins both
the 1 / render-scale handling and the claim that view-space z of an (s R | t)
pose is in the keyframe's units.
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

H, W = 48, 64
DEPTHS = (2.0, 1.8, 1.9)                      # of the plane, per view, own units
OFFSETS = ((0.0, 0.0, 0.0), (0.1, 0.0, 0.2), (-0.1, 0.05, 0.1))   # camera centres, own units
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _plane(scale=1.0):
    """(rows14 [P, 14] cuda, T_WC [3, 4, 4] cuda, poses [3, 8] cuda (lietorch
    Sim3 rows), K [3, 3] cpu, targets [3, H, W] cuda, images [3, 3, H, W])."""
    import lietorch
    from splatt3r_amd.refine import render_splats
    from splatt3r_amd.splatt3r_utils import _estimate_default_intrinsics, _sim3_to_4x4
    from splatt3r_amd.synthetic import smooth_texture
    K = _estimate_default_intrinsics(H, W, "cpu")
    f, cx, cy = float(K[0, 0]), float(K[0, 2]), float(K[1, 2])
    mx, my = 10, 8                                           # margin, pixels of view 0
    v, u = np.meshgrid(np.arange(-my, H + my), np.arange(-mx, W + mx), indexing="ij")
    d = DEPTHS[0]
    xyz = np.stack([(u + 0.5 - cx) / f * d, (v + 0.5 - cy) / f * d, np.full(u.shape, d)], -1)
    P = xyz.shape[0] * xyz.shape[1]
    tex = smooth_texture(H + 2 * my, W + 2 * mx, 5).transpose(1, 2, 0).reshape(P, 3)
    rows = np.zeros((P, 14), np.float32)
    rows[:, 0:3] = scale * xyz.reshape(P, 3)
    rows[:, 3:6] = (tex - 0.5) / 0.28209479177387814         # SH degree 0
    rows[:, 6] = 4.0                                         # opacity 0.98
    foot = scale * d / f                                     # one pixel of view 0 on the plane
    rows[:, 7:9] = np.log(0.7 * foot)
    rows[:, 9] = np.log(0.15 * foot)
    rows[:, 10] = 1.0
    poses = torch.tensor([[scale * o[0], scale * o[1], scale * o[2], 0, 0, 0, 1, scale]
                          for o in OFFSETS], dtype=torch.float32, device="cuda")
    T_WC = torch.cat([_sim3_to_4x4(lietorch.Sim3(p[None])) for p in poses]).cuda()
    targets = torch.tensor(DEPTHS, device="cuda").reshape(3, 1, 1).repeat(1, H, W).contiguous()
    rows = torch.from_numpy(rows).cuda()
    images = render_splats(rows, T_WC, K, H, W)
    return rows, T_WC, poses, K, targets, images


def _map_of(rows14, cap=16384):
    """A SharedGaussians holding splat rows (through s3w_map_from_splats)."""
    from splatt3r_amd import _lib
    from splatt3r_amd.gaussian_map import SharedGaussians
    gm = SharedGaussians(max_gaussians=cap, device="cuda")
    _lib.call("s3w_map_from_splats", ctypes.byref(gm._c), rows14.data_ptr(), rows14.shape[0], 0,
              _lib.stream(gm.device))
    return gm


def _pushed(rows, seed=5):
    """Every Gaussian moved along its ray from view 0 by +-5 % of its depth."""
    g = torch.Generator().manual_seed(seed)
    sign = (torch.randint(0, 2, (rows.shape[0], 1), generator=g) * 2 - 1).to(rows)
    out = rows.clone()
    out[:, :3] *= 1.0 + 0.05 * sign
    return out


def _abs_rel(rows, T_WC, K, targets):
    from splatt3r_amd.depth import depth_metrics
    D, A = _map_of(rows).render_depth_alpha(T_WC, K, H, W)
    m = depth_metrics(D, A, targets)
    return float(m["abs_rel"].mean()), float(m["valid"].min())


@pytest.mark.parametrize("scale", (1.0, 2.0))
def test_units_of_the_rendered_depth(scale, parity):
    from splatt3r_amd.depth import depth_metrics
    from splatt3r_amd.refine import DepthControl, refine_splats
    rows, T_WC, _, K, targets, images = _plane(scale)
    D, A = _map_of(rows).render_depth_alpha(T_WC[:2], K, H, W)
    assert D.shape == A.shape == (2, H, W) and D.dtype == torch.float32
    m = depth_metrics(D, A, targets[:2], align=None)
    h = {k: v.cpu().numpy() for k, v in m.items()}
    print("abs_rel", h["abs_rel"], "valid", h["valid"], "l1", h["l1"])
    parity(f"units.abs_rel.s{scale}", err=float(h["abs_rel"].max()), tol=1e-2)
    assert h["abs_rel"].max() < 1e-2 and h["valid"].min() > 0.9 and (h["scale"] == 1).all()
    # render_depths is this render with its division and threshold
    ref = _map_of(rows).render_depths(T_WC[:2], K, H, W)[0]
    mine = torch.where(A >= 0.5, D / A, torch.zeros_like(D))
    assert float((ref - mine).abs().max()) < 1e-5 and float(ref.max()) > 1.5
    # the loop's own folding of the render scale: the true rows have no depth loss
    dc = DepthControl(targets[:2], weight=1.0)
    refine_splats(rows, images[:2], T_WC[:2], K, 2, l1_weight=0.0, ssim_weight=0.0, depth=dc)
    first = dc.history.cpu().numpy()
    print("depth loss of the true rows:", first)
    assert first.shape == (2,) and (first < 1e-2 * 2.0).all()


def test_depth_only_refinement_descends(parity):
    from splatt3r_amd.refine import DepthControl, refine_splats
    rows, T_WC, _, K, targets, images = _plane(1.0)
    start = _pushed(rows)
    dc = DepthControl(targets[:2], weight=1.0)
    out, hist = refine_splats(start, images[:2], T_WC[:2], K, 40, l1_weight=0.0, ssim_weight=0.0,
                              depth=dc, lr_means=1e-3)
    h, hd = hist.cpu().numpy(), dc.history.cpu().numpy()
    print("depth-only losses:", h)
    assert h.shape == (40,) and np.isfinite(h).all() and np.array_equal(h, hd)   # weight 1, no colour term
    parity("descent.depth_only", err=float(h[-5:].mean()), tol=float(h[:5].mean()))
    assert h[-5:].mean() < h[:5].mean()
    assert out.shape == start.shape and not torch.equal(out[:, :3], start[:, :3])


def test_photometric_plus_depth_refinement(parity):
    from splatt3r_amd.refine import DepthControl, refine_splats
    rows, T_WC, _, K, targets, images = _plane(1.0)
    start = _pushed(rows)
    before, valid = _abs_rel(start, T_WC[:2], K, targets[:2])
    dc = DepthControl(targets[:2])
    out, hist = refine_splats(start, images[:2], T_WC[:2], K, 40, depth=dc)
    h = hist.cpu().numpy()
    after, _ = _abs_rel(out, T_WC[:2], K, targets[:2])
    print("losses:", h[:3], h[-3:], "abs_rel before", before, "after", after, "valid", valid)
    parity("descent.photo_plus_depth.abs_rel", err=after, tol=before)
    assert np.isfinite(h).all() and np.isfinite(dc.history.cpu().numpy()).all()
    assert before > 1e-3 and after <= before


def _random_scene():
    """The scene tests/test_refine.py compares two runs of the loop on: 2,048
    Gaussians of synthetic.raster_microbench_scene at random depths, 16 x 32
    (two rasterizer tiles), two views.  Two runs of the loop agree to the bit
    there.  On the plane above two identical calls without any depth argument
    differ in the last bits (thousands of exactly equal depths, float atomics
    in the rasterizer's backward), so it cannot carry this comparison."""
    from splatt3r_amd.gaussian_map import splats_from_cov
    from splatt3r_amd.refine import render_splats
    from splatt3r_amd.synthetic import raster_microbench_scene
    h, w, P = 16, 32, 2048
    K = np.array([[40.0, 0.0, w / 2], [0.0, 40.0, h / 2], [0.0, 0.0, 1.0]], np.float32)
    sc = raster_microbench_scene(P, H=h, W=w, K=K, seed=3)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r17 = splats_from_cov(cu(sc["means"]), cu(sc["cov6"]), torch.full((P, 3), 0.5, device="cuda"),
                          cu(sc["opacities"]))
    rows = torch.cat([r17[:, :3], r17[:, 6:]], 1).contiguous()
    rows[:, 3:6] = cu(sc["shs"][:, 0])
    T = torch.eye(4).repeat(2, 1, 1)
    T[1, :3, 3] = torch.tensor([0.15, -0.05, 0.1])
    T, K = T.cuda(), torch.from_numpy(K)
    images = render_splats(rows, T, K, h, w)
    g = torch.Generator().manual_seed(11)
    start = rows.clone()
    start[:, :3] += 0.003 * torch.randn(P, 3, generator=g).cuda()
    return start.contiguous(), T, K, images


def test_depth_none_is_the_loop_as_it_was():
    from splatt3r_amd.refine import DepthControl, refine_splats
    start, T_WC, K, images = _random_scene()
    a, ha = refine_splats(start, images, T_WC, K, 4)
    b, hb = refine_splats(start, images, T_WC, K, 4, depth=None)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ha.view(torch.int32), hb.view(torch.int32))
    # and a control does change the fit
    c, _ = refine_splats(start, images, T_WC, K, 4,
                         depth=DepthControl(torch.full((2, 16, 32), 4.0), weight=1.0))
    assert not torch.equal(a, c)


def test_map_and_frontend_entry_points():
    """SharedGaussians.refine(depth=...), Frontend.refine_map(depth="own") and
    Frontend.eval_depth on a hand-built session of three keyframes."""
    import lietorch
    from splatt3r_amd.depth import METRIC_NAMES
    from splatt3r_amd.evaluate import load_depth_metrics, save_depth_metrics
    from splatt3r_amd.frame import create_frame
    from splatt3r_amd.refine import DepthControl
    from splatt3r_amd.slam import Frontend
    rows, T_WC, poses, K, targets, images = _plane(2.0)
    start = _pushed(rows)
    gm = _map_of(start)
    hist = gm.refine(images, T_WC, K, 6, depth=DepthControl(targets, grad_weight=0.5))
    assert hist.shape == (6,) and torch.isfinite(hist).all() and gm.n_gaussians == rows.shape[0]

    dev = torch.device("cuda", 0)
    fe = Frontend(types.SimpleNamespace(), device=dev, render=False, viz=True, max_gaussians=16384)
    assert fe.eval_depth("own") is None and fe.refine_map(2, depth="own") is None
    f, cx, cy = float(K[0, 0]), float(K[0, 2]), float(K[1, 2])
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32),
                          indexing="ij")
    conf = torch.full((H, W), 2.0)
    conf[:10, :10] = 1.0                                       # below conf_min
    for i, d in enumerate(DEPTHS):
        kf = create_frame(i, (images[i:i + 1] * 2.0 - 1.0).contiguous(),
                          lietorch.Sim3(poses[i:i + 1].clone()), device=dev)
        X = torch.stack([(u + 0.5 - cx) / f * d, (v + 0.5 - cy) / f * d, torch.full((H, W), d)], -1)
        kf.X_canon, kf.C, kf.N = X.reshape(-1, 3).to(dev), conf.reshape(-1, 1).to(dev), 1
        fe.keyframes.append(kf)
    fe.gmap = _map_of(start)
    own_t, own_w = fe._own_depth([fe.keyframes[i] for i in range(3)], H, W, 1.5, dev)
    assert torch.equal(own_t, targets) and int(own_w.sum()) == 3 * (H * W - 100)
    assert not own_w[:, :10, :10].any()
    before = fe.eval_depth("own", align=None)
    assert len(before) == 3 and all(tuple(r) == METRIC_NAMES for r in before)
    assert all(0.5 < r["valid"] <= 1.0 - 100.0 / (H * W) and np.isfinite(r["abs_rel"]) for r in before)
    hist = fe.refine_map(6, depth="own")
    assert hist.shape == (6,) and torch.isfinite(hist).all()
    assert torch.isfinite(fe.refine_map(3, depth=targets, depth_weights=own_w)).all()
    with pytest.raises(ValueError, match="own"):
        fe.refine_map(2, depth="sensor")
    after = fe.eval_depth(targets)                              # align="global"
    assert len(after) == 3 and after[0]["scale"] == after[1]["scale"] == after[2]["scale"]
    assert abs(after[0]["scale"] - 1.0) < 0.05
    print("abs_rel before", [r["abs_rel"] for r in before], "after", [r["abs_rel"] for r in after])
    fe.close()


def test_depth_metrics_file_round_trip(tmp_path):
    from splatt3r_amd.depth import METRIC_NAMES
    from splatt3r_amd.evaluate import eval_depth_renders, load_depth_metrics, save_depth_metrics
    rows, T_WC, _, K, targets, _ = _plane(1.0)
    out = eval_depth_renders(_map_of(rows), T_WC, K, targets, align="scale")
    assert len(out) == 3 and all(tuple(r) == METRIC_NAMES for r in out)
    assert all(r["abs_rel"] < 1e-2 and abs(r["scale"] - 1.0) < 1e-2 and r["d1"] == 1.0 for r in out)
    save_depth_metrics(tmp_path, "depth.json", out)
    assert load_depth_metrics(tmp_path / "depth.json") == out
    from splatt3r_amd.gaussian_map import SharedGaussians
    assert eval_depth_renders(SharedGaussians(max_gaussians=16, device="cuda"), T_WC, K, targets) is None
