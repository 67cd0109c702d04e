"""Geometry against ground truth: evaluate.align_umeyama, associate,
read_traj, eval_trajectory (host, numpy float64) and eval_reconstruction on
the device (splatt3r_amd.nn: exact nearest neighbours, fixed-order sums).

Reference: tests/nn_search_ref64.py.  Tolerances: Umeyama is a float64 SVD of
a well-conditioned 3 x 3 matrix, 1e-9 is four orders above n 2^-52; the rmse
of the offset trajectory is a closed form, 1e-12.  The reconstruction scores
are compared exactly: the distances are bit for bit the oracle's and the sums
are taken in the order include/s3k.h fixes, which the oracle restates
(stats_in_order); on the two planes every distance is a float32 within a
factor 2 of 0.25, so any order of 4,096 of them sums without rounding.
"""
import functools
import math

import numpy as np
import pytest
import torch

import nn_search_ref64 as R

f32 = np.float32


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def known():
    rng = np.random.default_rng(17)
    return 1.7, _rotation(rng), np.array([0.4, -2.0, 3.1])


def _traj(n=40, seed=5):
    rng = np.random.default_rng(seed)
    ts = 100.0 + 0.1 * np.arange(n)
    pos = np.cumsum(rng.normal(0, 0.2, (n, 3)), 0)
    quat = rng.normal(size=(n, 4))
    return ts, np.concatenate([pos, quat / np.linalg.norm(quat, axis=1, keepdims=True)], 1)


# --------------------------------------------------------------------- CPU --
def test_umeyama_recovers_a_known_similarity(parity):
    from splatt3r_amd.evaluate import align_umeyama
    s, Rm, t = known()
    src = np.random.default_rng(1).normal(size=(50, 3))
    assert np.linalg.matrix_rank(src - src.mean(0)) == 3
    dst = s * src @ Rm.T + t
    gs, gR, gt = align_umeyama(src, dst)
    err = max(abs(gs - s), np.abs(gR - Rm).max(), np.abs(gt - t).max())
    parity("umeyama.known", err=err, tol=1e-9)
    assert err <= 1e-9
    assert abs(np.linalg.det(gR) - 1) < 1e-12
    gs, gR, gt = align_umeyama(src, dst, with_scale=False)
    assert gs == 1.0 and np.abs(gR - Rm).max() <= 1e-9
    # a mirrored target still gives a rotation
    gs, gR, gt = align_umeyama(src, dst * [1, 1, -1])
    assert abs(np.linalg.det(gR) - 1) < 1e-12
    for bad_src in (src[:2], np.outer(np.arange(10.0), [1, 2, 3]), np.ones((5, 3))):
        with pytest.raises(ValueError):
            align_umeyama(bad_src, bad_src * 2 + 1)
    with pytest.raises(ValueError):
        align_umeyama(src, dst[:-1])
    with pytest.raises(ValueError):
        align_umeyama(np.where(np.arange(50)[:, None] == 3, np.nan, src), dst)


def test_associate_is_one_to_one_and_bounded():
    from splatt3r_amd.evaluate import associate
    a = np.array([0.0, 0.1, 0.2, 0.3, 5.0])
    b = np.array([0.105, 0.0, 0.315, 0.22, 0.101, 9.0])
    ia, ib = associate(a, b)
    assert list(zip(ia.tolist(), ib.tolist())) == [(0, 1), (1, 4), (2, 3), (3, 2)]
    assert len(set(ib.tolist())) == len(ib)
    ia, ib = associate(a, b, max_dt=0.015)               # 0.3 <-> 0.315, 0.2 <-> 0.22 are dropped
    assert list(zip(ia.tolist(), ib.tolist())) == [(0, 1), (1, 4)]
    # two estimates compete for one stamp: the nearer takes it, the other takes nothing twice
    ia, ib = associate([1.0, 1.01], [1.004], max_dt=0.02)
    assert (ia.tolist(), ib.tolist()) == ([0], [0])
    ia, ib = associate([1.0, 1.01], [1.004, 1.02], max_dt=0.02)
    assert (ia.tolist(), ib.tolist()) == ([0, 1], [0, 1])
    ia, ib = associate([], [1.0])
    assert len(ia) == 0 and len(ib) == 0
    ia, ib = associate([1.0], [1.25], max_dt=0.25)        # exactly max_dt apart counts
    assert len(ia) == 1


def test_read_traj_reads_what_save_traj_writes(tmp_path):
    from splatt3r_amd.evaluate import read_traj, traj_line
    ts, poses = _traj(7)
    p = tmp_path / "traj.txt"
    with open(p, "w") as f:
        f.write("# timestamp tx ty tz qx qy qz qw\n\n")
        for t, row in zip(ts, poses):
            f.write(traj_line(t, row))
    gts, gp = read_traj(p)
    assert np.array_equal(gts, ts) and np.array_equal(gp, poses.astype(f32).astype(np.float64))
    with open(p, "a") as f:
        f.write("1.0 2.0 3.0\n")
    with pytest.raises(ValueError, match="8 columns"):
        read_traj(p)


def test_eval_trajectory(parity, tmp_path):
    from splatt3r_amd.evaluate import align_umeyama, eval_trajectory, traj_line
    s, Rm, t = known()
    ts, est = _traj()
    gt = est.copy()
    gt[:, :3] = s * est[:, :3] @ Rm.T + t
    r = eval_trajectory((ts, est), (ts + 0.004, gt))
    parity("ate.exact", err=r["rmse"], tol=1e-9)
    assert r["rmse"] <= 1e-9 and r["n"] == 40 and abs(r["scale"] - s) <= 1e-9
    assert np.abs(r["R"] - Rm).max() <= 1e-9 and np.abs(r["t"] - t).max() <= 1e-9
    assert r["min"] <= r["median"] <= r["max"] and r["mean"] <= r["rmse"] + 1e-15
    # SE3 alignment of a scaled trajectory cannot reach zero
    assert eval_trajectory((ts, est), (ts, gt), with_scale=False)["rmse"] > 1e-2
    # ground truth offset by (0.3, 0, 0) on every second pose
    off = est.copy()
    off[1::2, 0] += 0.3
    r = eval_trajectory((ts, est), (ts, off), align=False)
    parity("ate.offset", err=abs(r["rmse"] - 0.3 / math.sqrt(2)), tol=1e-12)
    assert abs(r["rmse"] - 0.3 / math.sqrt(2)) <= 1e-12
    assert r["scale"] == 1.0 and np.array_equal(r["R"], np.eye(3)) and r["n"] == 40
    assert abs(r["mean"] - 0.15) <= 1e-12 and abs(r["std"] - 0.15) <= 1e-12
    assert abs(r["max"] - 0.3) <= 1e-12 and r["min"] == 0.0
    got, want = align_umeyama(est[:, :3], off[:, :3]), R.umeyama(est[:, :3], off[:, :3])
    err = max(abs(got[0] - want[0]), np.abs(got[1] - want[1]).max(), np.abs(got[2] - want[2]).max())
    parity("umeyama.offset", err=err, tol=1e-9)
    assert err <= 1e-9
    r = eval_trajectory((ts, est), (ts, off))
    e = R.ate(est[:, :3], off[:, :3], want)
    assert abs(r["rmse"] - math.sqrt((e ** 2).mean())) <= 1e-9 and r["rmse"] < 0.3 / math.sqrt(2)
    # files, and stamps further apart than max_dt
    pe, pg = tmp_path / "est.txt", tmp_path / "gt.txt"
    for p, (tt, rows) in ((pe, (ts, est)), (pg, (ts + 0.004, gt))):
        with open(p, "w") as f:
            f.write("# t x y z qx qy qz qw\n")
            for a, row in zip(tt, rows):
                f.write(traj_line(repr(float(a)), row))
    assert eval_trajectory(pe, pg)["rmse"] <= 1e-5         # float32 rows in the file
    assert eval_trajectory(str(pe), pg, max_dt=0.005)["n"] == 40
    with pytest.raises(ValueError, match="max_dt"):
        eval_trajectory(pe, pg, max_dt=0.001)


def test_apply_transform_and_metrics_file(tmp_path):
    from splatt3r_amd.evaluate import (apply_transform, load_geometry_metrics,
                                       save_geometry_metrics)
    s, Rm, t = known()
    p = np.random.default_rng(3).normal(size=(100, 3)).astype(f32)
    got = apply_transform(p, (s, Rm, t))
    assert got.dtype == f32
    assert np.abs(got - (s * p.astype(np.float64) @ Rm.T + t)).max() <= 2.0 ** -22
    assert np.array_equal(got, apply_transform(torch.from_numpy(p), (s, Rm, t)))
    m = dict(accuracy=0.25, completion=0.5, chamfer=0.375, precision=1.0, recall=0.5,
             fscore=2 / 3, n_rec=10, n_gt=20, threshold=0.05,
             trajectory=dict(rmse=np.float64(0.1), n=3, scale=s, R=Rm, t=t))
    save_geometry_metrics(tmp_path / "logs", "geometry.json", m)
    text = open(tmp_path / "logs" / "geometry.json").read()
    assert text.count("\n") == 1 and text.endswith("\n")
    back = load_geometry_metrics(tmp_path / "logs" / "geometry.json")
    assert back["fscore"] == 2 / 3 and back["n_gt"] == 20
    assert np.array_equal(back["trajectory"]["R"], Rm) and np.array_equal(back["trajectory"]["t"], t)


def test_a_list_of_two_points_is_not_a_mesh():
    from splatt3r_amd.evaluate import _is_faces
    two = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
    assert not _is_faces(two[1]) and not _is_faces(np.zeros((5, 3), f32))
    assert not _is_faces(torch.zeros(5, 3)) and not _is_faces(np.zeros((5, 2), np.int32))
    assert _is_faces(np.zeros((5, 3), np.int32)) and _is_faces(torch.zeros(0, 3, dtype=torch.int64))
    assert _is_faces([[0, 1, 2]])


def test_eval_reconstruction_needs_a_gpu_and_says_so():
    from splatt3r_amd.evaluate import eval_reconstruction
    with pytest.raises(RuntimeError):
        eval_reconstruction(torch.zeros(4, 3), torch.zeros(4, 3), device="cpu")


# --------------------------------------------------------------------- GPU --
def _planes():
    g = np.arange(64, dtype=np.float64) / 64.0
    y, x = np.meshgrid(g, g, indexing="ij")
    low = np.stack([x, y, np.zeros_like(x)], -1).reshape(-1, 3)
    return low.astype(f32), (low + [0, 0, 0.25]).astype(f32)


def _oracle_scores(p_rec, p_gt, thr, fast=False):
    near = R.nearest_prefiltered if fast else R.nearest
    a = R.stats_in_order(near(p_rec, p_gt)[1], thr)
    b = R.stats_in_order(near(p_gt, p_rec)[1], thr)
    P, Rc = a[3] / len(p_rec), b[3] / len(p_gt)
    acc, comp = a[1] / a[0], b[1] / b[0]
    return dict(accuracy=acc, completion=comp, chamfer=0.5 * (acc + comp), precision=P, recall=Rc,
                fscore=2 * P * Rc / (P + Rc) if P + Rc > 0 else 0.0)


@pytest.mark.gpu
def test_hip_two_planes(tmp_path, parity):
    from splatt3r_amd.evaluate import eval_reconstruction, write_mesh_ply
    rec, gt = _planes()
    r = eval_reconstruction(torch.from_numpy(rec).cuda(), gt, threshold=0.3)
    for k in ("accuracy", "completion", "chamfer"):
        parity(f"planes.{k}", err=abs(r[k] - 0.25), tol=0.0)
    parity("planes.fscore", err=abs(r["fscore"] - 1.0), tol=0.0)
    assert r["accuracy"] == 0.25 and r["completion"] == 0.25 and r["chamfer"] == 0.25
    assert r["precision"] == 1.0 and r["recall"] == 1.0 and r["fscore"] == 1.0
    assert r["n_rec"] == 4096 and r["n_gt"] == 4096 and r["threshold"] == 0.3
    r = eval_reconstruction(rec, gt, threshold=0.2, cell=0.1)
    assert r["accuracy"] == 0.25 and r["fscore"] == 0.0 and r["precision"] == 0.0
    # a .ply without faces is a point cloud; max_dist below the gap leaves nothing
    p = tmp_path / "rec.ply"
    write_mesh_ply(p, rec, np.zeros_like(rec), np.zeros((0, 3), np.int32))
    r = eval_reconstruction(p, gt, threshold=0.3)
    assert r["chamfer"] == 0.25 and r["fscore"] == 1.0
    two = eval_reconstruction([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.0, 0.5], [1.0, 0.0, 0.5]],
                              threshold=0.3)
    assert two["n_rec"] == 2 and two["accuracy"] == 0.5          # two points, not a mesh
    r = eval_reconstruction(p, gt, threshold=0.3, max_dist=0.2)
    assert math.isnan(r["accuracy"]) and r["fscore"] == 0.0


@pytest.mark.gpu
def test_hip_two_planes_transformed(parity):
    from splatt3r_amd.evaluate import apply_transform, eval_reconstruction
    s, Rm, t = known()
    rec, gt = _planes()
    moved = (((rec.astype(np.float64) - t) / s) @ Rm).astype(f32)      # R^T (p - t) / s
    for thr in (0.3, 0.2):
        r = eval_reconstruction(moved, gt, threshold=thr, transform=(s, Rm, t))
        back = apply_transform(moved, (s, Rm, t))
        assert np.abs(back - rec).max() <= 2.0 ** -20 and not np.array_equal(back, rec)
        w = _oracle_scores(back, gt, thr)
        for k, v in w.items():
            parity(f"planes.moved.{thr}.{k}", err=abs(r[k] - v), tol=0.0, off=abs(r[k] - 0.25))
            assert r[k] == v, (k, r[k], v)
        assert 0 < abs(r["accuracy"] - 0.25) <= 2.0 ** -19
    assert r["fscore"] == 0.0


CUBE_V = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], f32)
CUBE_F = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4],
                   [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]], np.int32)


@pytest.mark.gpu
def test_hip_cube_mesh_against_itself(parity):
    from splatt3r_amd.evaluate import eval_reconstruction
    mesh = (torch.from_numpy(CUBE_V).cuda(), torch.from_numpy(CUBE_F).cuda())
    r = eval_reconstruction(mesh, (CUBE_V, CUBE_F), threshold=0.05, samples=20000, seed=4)
    assert r["precision"] == 1.0 and r["recall"] == 1.0 and r["fscore"] == 1.0
    assert r["n_rec"] == 20000 and r["n_gt"] == 20000
    w = _oracle_scores(R.sample_mesh(CUBE_V, CUBE_F, 20000, 4)["points"],
                       R.sample_mesh(CUBE_V, CUBE_F, 20000, 5)["points"], 0.05, fast=True)
    for k, v in w.items():
        parity(f"cube.{k}", err=abs(r[k] - v), tol=0.0)
        assert r[k] == v, (k, r[k], v)
    assert 0 < r["accuracy"] < 0.02


@pytest.mark.gpu
def test_hip_frontend_eval_geometry_returns_none_like_save_mesh():
    """None before the first keyframe and when the session keeps no map (viz
    off), as save_mesh; the scoring path itself is the plane-map test below."""
    from splatt3r_amd.slam import Frontend
    from test_map_reanchor import _model_and_frames
    dev, model, frames = _model_and_frames()
    gt = np.zeros((4, 3), f32)
    fe = Frontend(model, device=dev, spatial_stride=4, render=False, viz=True, max_gaussians=20000)
    try:
        assert fe.eval_geometry(gt, 0.1) is None
    finally:
        fe.close()
    off = Frontend(model, device=dev, spatial_stride=4, render=False, viz=False)
    try:
        off.step(0, frames[0])
        assert len(off.keyframes) >= 1 and off.eval_geometry(gt, 0.1) is None
    finally:
        off.close()


@pytest.mark.gpu
def test_hip_eval_geometry_of_a_plane_map():
    """eval_geometry on a map that does give a mesh (test_tsdf_mesh's plane
    z = 2 + 0.05 x seen from three poses): the surface lies within a voxel of
    the plane; ground truth in a frame that is a known similarity of the
    map's, with the keyframe trajectory in that frame, gives that similarity
    back and the same scores times its scale."""
    import types
    import lietorch
    from splatt3r_amd.slam import Frontend
    from test_tsdf_mesh import _plane_map
    gm = _plane_map()
    H, W, voxel = 48, 64, 0.08
    fe = Frontend.__new__(Frontend)
    fe.gmap, fe.device, fe.main_stream, fe.map_follow_poses = gm, gm.device, None, False
    fe.K = torch.tensor([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]])
    fe.drain = lambda: None
    centres = [(0.0, 0.0, 0.0), (0.4, 0.0, 0.0), (0.0, -0.3, 0.0)]
    fe.keyframes = [types.SimpleNamespace(
        T_WC=lietorch.Sim3(torch.tensor([[*c, 0.0, 0.0, 0.0, 1.0, 1.0]], device="cuda")),
        frame_id=i, uimg=None, img=torch.zeros(1, 3, H, W, device="cuda"))
        for i, c in enumerate(centres)]
    g = np.arange(-130, 131) / 100.0
    y, x = np.meshgrid(g, g, indexing="ij")
    plane = np.stack([x, y, 2.0 + 0.05 * x], -1).reshape(-1, 3)
    kw = dict(threshold=2 * voxel, samples=20000)
    r = fe.eval_geometry(plane.astype(f32), voxel, **kw)
    print("plane map:", r)
    assert r is not None and r["n_rec"] == 20000 and r["n_gt"] == len(plane)
    assert 0 < r["accuracy"] < voxel and r["precision"] > 0.9
    s, Rm, t = known()
    stamps = [1.0, 2.0, 3.0]
    traj = (stamps, np.asarray(centres) @ Rm.T * s + t)
    r2 = fe.eval_geometry((plane @ Rm.T * s + t).astype(f32), voxel, traj_gt=traj,
                          timestamps=stamps, threshold=2 * voxel * s, samples=20000)
    print("moved:", r2)
    tr = r2["trajectory"]
    assert tr["n"] == 3 and tr["rmse"] < 1e-5 and abs(tr["scale"] - s) < 1e-5
    assert np.abs(tr["R"] - Rm).max() < 1e-5
    assert abs(r2["accuracy"] / (s * r["accuracy"]) - 1) < 0.05
    assert abs(r2["precision"] - r["precision"]) < 0.02
