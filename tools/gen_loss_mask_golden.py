"""Write tests/golden/loss_mask.npz: inputs, the reference's loss mask and its
three conditions, and the measured float32 floors.

Needs the reference tree ($S3_REFERENCE_DIR, default /root/reference) with
torch and einops; it is imported at run time and runs on the CPU.  Only
inputs and outputs are stored.

    python tools/gen_loss_mask_golden.py [--out tests/golden/loss_mask.npz]

Cases
  r0..r2  seeded random scenes: a slanted plane z = 3 + 0.2 x - 0.1 y behind a
          rectangular occluder at z = 1.6, ray-cast per camera (so depth has a
          step); rotations up to 0.35 rad, translations up to 0.8, per-view
          focal max(h, w) U(0.9, 1.2), fy = 1.05 fx, off-centre principal
          point; 6 % of the target and 3 % of the context depths set to 0.
  a       a pixel inside view A's frustum with mismatched depth there, whose
          only depth match is in view B, where it is outside the frustum
          (u just below 0: the sample mixes the zero padding with column 0).
  b       a point 0.05 behind a context camera, projecting inside its image,
          where depth_2 is 0.
  c       the scene of r* seen by cameras with a Sim3 scale of 1.7 in c2w and
          a skewed K.
For a, b and c the generator asserts what each is built to show and that no
pixel lies within a band of 1e-3 px / 1e-3 depth, far wider than the measured
one, so tests may compare them exactly.

The conditions are recomputed with the reference's own geometry functions and
grid_sample in the order calculate_in_frustum_mask uses them; their AND is
asserted equal to the mask it returns.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
from loss_mask_ref64 import loss_mask_ref  # noqa: E402

RANDOM_SHAPES = ((2, 2, 2, 24, 40), (1, 1, 3, 37, 53), (1, 3, 1, 16, 16))
OCCLUDER = dict(z=1.6, x=(-0.7, 0.5), y=(-0.4, 0.6))
WIDE_PX, WIDE_D = 1e-3, 1e-3


def reference_dir():
    return os.environ.get("S3_REFERENCE_DIR", "/root/reference")


def import_reference():
    core = os.path.join(reference_dir(), "splatt3r_core")
    if core not in sys.path:
        sys.path.insert(0, core)
    import utils.geometry as geometry
    import utils.loss_mask as loss_mask
    return loss_mask, geometry


# ------------------------------------------------------------------ scenes --
def rotation(rng, max_angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-max_angle, max_angle)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def camera(rng, h, w, scale=1.0, skew=0.0):
    f = max(h, w) * rng.uniform(0.9, 1.2)
    K = np.array([[f, skew, w * rng.uniform(0.4, 0.6)],
                  [0, 1.05 * f, h * rng.uniform(0.4, 0.6)], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = scale * rotation(rng, 0.35)
    T[:3, 3] = rng.uniform(-0.8, 0.8, size=3) * np.array([1, 1, 0.5])
    return K, T


def raycast(K, T, h, w):
    """z-depth (in the camera's own units) of the scene along the ray of every
    integer pixel (x, y); 0 where the ray hits nothing in front."""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64),
                         indexing="ij")
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T      # cam, z = 1
    dirs, o = rays @ T[:3, :3].T, T[:3, 3]
    n = np.array([-0.2, 0.1, 1.0])                                            # n . p = 3
    with np.errstate(divide="ignore", invalid="ignore"):
        t_plane = (3.0 - n @ o) / (dirs @ n)
        t_occ = (OCCLUDER["z"] - o[2]) / dirs[..., 2]
    hit = o + t_occ[..., None] * dirs
    on_occ = ((t_occ > 0) & (hit[..., 0] > OCCLUDER["x"][0]) & (hit[..., 0] < OCCLUDER["x"][1])
              & (hit[..., 1] > OCCLUDER["y"][0]) & (hit[..., 1] < OCCLUDER["y"][1]))
    depth = np.where(on_occ, t_occ, np.where(t_plane > 0, t_plane, 0.0))
    return np.nan_to_num(depth, nan=0.0, posinf=0.0, neginf=0.0)


def scene(rng, shape, scale=1.0, skew=0.0, holes=(0.06, 0.03)):
    b, v1, v2, h, w = shape
    out = []
    for nv, hole in ((v1, holes[0]), (v2, holes[1])):
        d, Ks, Ts = np.zeros((b, nv, h, w)), np.zeros((b, nv, 3, 3)), np.zeros((b, nv, 4, 4))
        for bb in range(b):
            for i in range(nv):
                Ks[bb, i], Ts[bb, i] = camera(rng, h, w, scale, skew)
                d[bb, i] = raycast(Ks[bb, i], Ts[bb, i], h, w)
        d[rng.uniform(size=d.shape) < hole] = 0.0
        out += [d, Ks, Ts]
    return [torch.from_numpy(a.astype(np.float32)) for a in out]


def pinhole(f, c):
    return np.array([[f, 0, c], [0, f, c], [0, 0, 1.0]])


def pose(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def case_a():
    """8 x 8, target depth 2.  Probe pixel (4, 4) -> world (0, 0, 2).  View A
    (shifted by (0.1, 0.05, 0)) sees it at (3.6, 3.8) with depth 5 there;
    view B (shifted by (1.05, 0.05, 0)) sees it at u = -0.2, v = 3.8, where the
    sample is 0.3 (0.7 D[3, 0] + 0.3 D[4, 0]) = 2 with column 0 at 2 / 0.3."""
    h = w = 8
    K = pinhole(8.0, 4.0)
    d1 = np.full((1, 1, h, w), 2.0)
    d2 = np.full((1, 2, h, w), 5.0)
    d2[0, 1, :, 0] = 2.0 / 0.3
    K1, T1 = K[None, None], pose([0, 0, 0])[None, None]
    K2 = np.stack([K, K])[None]
    T2 = np.stack([pose([0.1, 0.05, 0]), pose([1.05, 0.05, 0])])[None]
    return [torch.from_numpy(a.astype(np.float32)) for a in (d1, K1, T1, d2, K2, T2)], (4, 4)


def case_b():
    """8 x 8, target depth 2.  Probe pixel (4, 4) -> world (0, 0, 2), 0.05
    behind the context camera at (0, 0, 2.05), which projects it to (4, 4);
    depth_2 is 0 everywhere, so |z - s| = 0.05 <= 0.1."""
    h = w = 8
    K = pinhole(8.0, 4.0)
    d1 = np.full((1, 1, h, w), 2.0)
    d2 = np.zeros((1, 1, h, w))
    arrs = (d1, K[None, None], pose([0, 0, 0])[None, None], d2, K[None, None],
            pose([0, 0, 2.05])[None, None])
    return [torch.from_numpy(a.astype(np.float32)) for a in arrs], (4, 4)


def case_c(ref_fn):
    """The first seed whose 12 x 12 scaled / skewed scene keeps every pixel
    clear of the wide band and has both mask values."""
    for seed in range(200):
        args = scene(np.random.default_rng(1000 + seed), (1, 1, 1, 12, 12), scale=1.7, skew=0.8,
                     holes=(0.0, 0.0))
        r = loss_mask_ref(*args)
        clear = not bool(((r["m_fr"] < WIDE_PX) | (r["m_md"].abs() < WIDE_D)).any())
        frac = r["mask"].float().mean().item()
        if clear and 0.2 < frac < 0.8:
            return args
    raise RuntimeError("case c: no clear seed")


# --------------------------------------------------------------- reference --
def run_reference(loss_mask, geometry, args):
    """(mask, fr, nz, md, u, v, z, s): the reference's mask, and its three
    conditions and intermediates recomputed with its own functions in the order
    calculate_in_frustum_mask uses them."""
    depth_1, K_1, c2w_1, depth_2, K_2, c2w_2 = args
    mask = loss_mask.calculate_in_frustum_mask(*[a.clone() for a in args])
    b, v1, h, w = depth_1.shape
    v2 = depth_2.shape[1]
    with torch.no_grad():
        points_3d = geometry.unproject_depth(depth_1[..., None], K_1, c2w_1)
        camera_points = geometry.world_space_to_camera_space(points_3d, c2w_2)
        points_2d = geometry.camera_space_to_pixel_space(camera_points, K_2)
        z = camera_points[..., 2]
        u, v = points_2d[..., 0].clone(), points_2d[..., 1].clone()
        fr = ((u > 0) & (u < w) & (v > 0) & (v < h)).any(dim=-3)
        nz = depth_1 > 1e-6
        grid = torch.stack([u / w, v / h], -1) * 2 - 1
        s = torch.empty_like(z)
        for bb in range(b):
            for i in range(v1):
                for j in range(v2):
                    s[bb, i, j] = torch.nn.functional.grid_sample(
                        depth_2[bb, j][None, None], grid[bb, i, j][None], align_corners=False)[0, 0]
        md = torch.isclose(z, s, atol=1e-1).any(dim=-3)
    assert torch.equal(fr & nz & md, mask), "conditions do not AND to the reference's mask"
    return mask, fr, nz, md, u, v, z, s


def floors(ref32, r64):
    """Largest |float32 reference - float64 restatement| of u, v (px) and of
    the depth margin, over the entries finite in both."""
    _, _, _, _, u, v, z, s = ref32
    z, s = z.double(), s.double()
    m_md = (z - s).abs() - (1e-1 + 1e-5 * s.abs())
    def dmax(a, b):
        d = (a.double() - b).abs()
        d = d[torch.isfinite(d)]
        return float(d.max()) if d.numel() else 0.0
    return max(dmax(u, r64["u"]), dmax(v, r64["v"])), dmax(m_md, r64["m_md"])


def build_cases():
    loss_mask, geometry = import_reference()
    cases = {}
    for k, shape in enumerate(RANDOM_SHAPES):
        cases[f"r{k}"] = scene(np.random.default_rng(20 + k), shape)
    (cases["a"], probe_a), (cases["b"], probe_b) = case_a(), case_b()
    cases["c"] = case_c(loss_mask_ref)

    out, floor_px, floor_d = {}, 0.0, 0.0
    for name, args in cases.items():
        ref32 = run_reference(loss_mask, geometry, args)
        r64 = loss_mask_ref(*args)
        mask, fr, nz, md = ref32[:4]
        fpx, fd = floors(ref32, r64)
        floor_px, floor_d = max(floor_px, fpx), max(floor_d, fd)
        wide = ((r64["m_fr"] < WIDE_PX) | (r64["m_md"].abs() < WIDE_D)).any(2)
        differ = ((r64["mask"] != mask) | (r64["fr"] != fr) | (r64["md"] != md)) & ~wide
        assert not bool(differ.any()), f"{name}: restatement and reference differ off the band"
        if name in ("a", "b", "c"):
            assert not bool(wide.any()), f"{name}: a pixel lies inside the wide band"
        print(f"{name}: shape {tuple(args[0].shape)} v2 {args[3].shape[1]}  mask "
              f"{mask.float().mean().item():.3f}  fr {fr.float().mean().item():.3f}  nz "
              f"{nz.float().mean().item():.3f}  md {md.float().mean().item():.3f}  "
              f"md&~fr {int((md & ~fr).sum())}  fr&nz&~md {int((fr & nz & ~md).sum())}  "
              f"wide-band {int(wide.sum())}  floor px {fpx:.3g} d {fd:.3g}")
        for key, a in zip(("depth_1", "K_1", "c2w_1", "depth_2", "K_2", "c2w_2"), args):
            out[f"{name}.{key}"] = a.numpy()
        for key, a in (("mask", mask), ("fr", fr), ("nz", nz), ("md", md)):
            out[f"{name}.{key}"] = a.numpy()

    # what the hand-built cases are built to show
    x, y = probe_a
    ra = loss_mask_ref(*cases["a"])
    fr_j = (ra["u"] > 0) & (ra["u"] < 8) & (ra["v"] > 0) & (ra["v"] < 8)
    md_j = ra["m_md"] <= 0
    assert fr_j[0, 0, :, y, x].tolist() == [True, False]
    assert md_j[0, 0, :, y, x].tolist() == [False, True]
    assert bool(out["a.mask"][0, 0, y, x]) and not bool((fr_j & md_j).any(2)[0, 0, y, x])
    x, y = probe_b
    rb = loss_mask_ref(*cases["b"])
    assert abs(float(rb["z"][0, 0, 0, y, x]) + 0.05) < 1e-6 and bool(out["b.mask"][0, 0, y, x])

    out["names"] = np.array(list(cases))
    out["probe_a"], out["probe_b"] = np.array(probe_a), np.array(probe_b)
    out["floor_px"], out["floor_d"] = np.float64(floor_px), np.float64(floor_d)
    print(f"floors: u, v {floor_px:.3g} px, m_md {floor_d:.3g}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "loss_mask.npz"))
    a = ap.parse_args()
    out = build_cases()
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
