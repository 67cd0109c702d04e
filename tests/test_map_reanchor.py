"""Map re-anchor (include/s3a.h, csrc/map_reanchor.hip,
SharedGaussians.reanchor, Frontend(map_follow_poses=True)) against the numpy
float64 restatement tests/map_reanchor_ref64.py.

Tolerance (the house rule): 4 x the error of the same composition done in
float32 on the CPU over the 1,000-row case below, rounded up to one digit,
one figure per metric -- a mean's error relative to |M| |mu - t_o| + |t_n|, a
covariance row's error relative to its largest output entry.  It is computed
here (`tolerance()`), never taken from the kernel's own result; DESIGN 6o
records the values.
"""
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_reanchor_ref64 as R
from conftest import REPO

I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
SENTINEL = 1234.5


# ------------------------------------------------------------------ cases ---
def _unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _poses(rng, n, tmax=100.0, unit_scale=False):
    """[n, 8] float32: |t| up to tmax, random unit quaternions, scales
    log-uniform over 0.25..4."""
    d = rng.normal(size=(n, 3))
    t = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, tmax, size=(n, 1))
    s = np.ones((n, 1)) if unit_scale else np.exp(rng.uniform(np.log(0.25), np.log(4.0), (n, 1)))
    return np.concatenate([t, _unit_quats(rng, n), s], 1).astype(np.float32)


def _covs(rng, n):
    """Covariances R diag(lambda) R^T with eigenvalue ratios up to 1e8."""
    top = np.exp(rng.uniform(np.log(1e-4), np.log(1.0), size=(n, 1)))
    lam = top * np.concatenate([np.ones((n, 1)), 10.0 ** rng.uniform(-8, 0, size=(n, 2))], 1)
    p = np.zeros((n, 8))
    p[:, 3:7] = _unit_quats(rng, n)
    p[:, 7] = 1
    Q = np.stack([R.rotation(r) for r in p.astype(np.float32)])
    return R.full_to_triu(np.einsum("nik,nk,njk->nij", Q, lam, Q)).astype(np.float32)


# what happens to keyframe k, by k % 10 (k = 0 moves, so n_kf = 1 moves)
KINDS = ("move", "move", "same", "unset", "nan", "move", "s0", "sneg", "q0", "move")


def _tables(rng, n_kf, unit_scale=False):
    anchor = _poses(rng, n_kf, unit_scale=unit_scale)
    poses = _poses(rng, n_kf, unit_scale=unit_scale)
    for k in range(n_kf):
        kind = KINDS[k % len(KINDS)]
        if kind == "same":
            poses[k] = anchor[k]
        elif kind == "unset":
            anchor[k] = 0
        elif kind == "nan":
            poses[k, k % 8] = np.nan
        elif kind == "s0":
            poses[k, 7] = 0
        elif kind == "sneg":
            poses[k, 7] = -1
        elif kind == "q0":
            poses[k, 3:7] = 0
    return anchor, poses


def _run_labels(n, n_kf, cuts):
    """Labels in runs: a new keyframe (cycling) after each cut."""
    lab = np.zeros(n, np.int32)
    k = 0
    for a, b in zip([0] + list(cuts), list(cuts) + [n]):
        lab[a:b] = k % n_kf
        k += 1
    return lab


def make_case(n, n_kf, seed=0, cap=1001, labels=None, unit_scale=False):
    rng = np.random.default_rng(seed)
    anchor, poses = _tables(rng, n_kf, unit_scale)
    if labels is None:
        # run boundaries at rows 255, 256 and 257, then every 97 rows
        cuts = [c for c in (255, 256, 257) if c < n] + list(range(300, n, 97))
        labels = _run_labels(n, n_kf, cuts)
    kf = np.zeros(cap, np.int32)          # past the count: label 0, which moves
    kf[:n] = labels
    ko = np.clip(kf, 0, n_kf - 1)
    means = (anchor[ko, :3] + rng.normal(size=(cap, 3)) * 5).astype(np.float32)
    cov = _covs(rng, cap)
    if n > 3:
        cov[3] = 0                        # one zero covariance
    colors = rng.uniform(size=(cap, 3)).astype(np.float32)
    opac = rng.uniform(size=cap).astype(np.float32)
    for a in (means, cov, colors, opac):
        a[n:] = SENTINEL
    return dict(n=n, cap=cap, n_kf=n_kf, means=means, cov=cov, colors=colors, opac=opac, kf=kf,
                anchor=anchor, poses=poses)


def _ref(c, **kw):
    return R.reanchor(c["means"], c["cov"], c["kf"], c["n"], c["anchor"], c["poses"], **kw)


@functools.lru_cache(maxsize=None)
def base_case():
    """1,000 rows over 7 keyframes (3 move, 1 equal, 1 unset, 2 held)."""
    c = make_case(1000, 7, seed=1)
    return c, _ref(c)


def _round_up_one_digit(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-12) * 10 ** e


@functools.lru_cache(maxsize=None)
def tolerance():
    """(mean, covariance): 4 x the float32 composition's error on the base
    case, rounded up to one digit."""
    c, ref = base_case()
    f32 = _ref(c, dtype=np.float32)
    em, ec = R.errors(f32["means"], f32["cov"], ref)
    assert 1e-8 < em < 1e-5 and 1e-8 < ec < 1e-5, (em, ec)
    return _round_up_one_digit(4 * em), _round_up_one_digit(4 * ec)


# ------------------------------------------------------ CPU: ref64 by hand ---
def test_ref64_by_hand():
    """180 degrees about z, scale 1 -> 2, dyadic everything: exact."""
    t_o, t_n = np.array([1.0, -2.0, 0.5]), np.array([-4.0, 8.0, 0.25])
    anchor = np.array([[*t_o, 0, 0, 0, 1, 1]], np.float32)
    poses = np.array([[*t_n, 0, 0, 1, 0, 2]], np.float32)
    mu = np.array([[3.0, 0.5, -1.5], [0.25, 4.0, 2.0]], np.float32)
    cov = np.array([[1.0, 0.5, 0.25, 2.0, -0.125, 4.0], [0.5, 0, 0, 0.5, 0, 0.5]], np.float32)
    kf = np.array([0, 0], np.int32)
    out = R.reanchor(mu, cov, kf, 2, anchor, poses)
    e = mu.astype(np.float64) - t_o
    want_mu = t_n + 2 * np.stack([-e[:, 0], -e[:, 1], e[:, 2]], 1)
    want_cov = 4 * cov.astype(np.float64) * np.array([1, 1, -1, 1, -1, 1.0])
    assert (out["means"] == want_mu).all()
    assert (out["cov"] == want_cov).all()
    assert out["moved"] == 2 and out["held"] == 0
    assert (out["anchor"] == poses).all()


def test_ref64_unset_held_and_out_of_range_labels():
    mu = np.arange(12, dtype=np.float32).reshape(4, 3)
    cov = np.tile(np.array([1, 0, 0, 1, 0, 1], np.float32), (4, 1))
    p = np.array([[1, 2, 3, 0, 0, 1, 0, 2]], np.float32)
    # an unset anchor adopts the pose and moves nothing
    out = R.reanchor(mu, cov, np.zeros(4, np.int32), 4, np.zeros((1, 8), np.float32), p)
    assert out["moved"] == 0 and out["held"] == 0 and (out["anchor"] == p).all()
    assert (out["means"] == mu).all() and (out["cov"] == cov).all()
    # NaN, s = 0, s < 0 and a zero quaternion are each held
    a = np.array([[0, 0, 0, 0, 0, 0, 1, 1]], np.float32)
    for col, val in ((1, np.nan), (7, 0.0), (7, -2.0), (None, None)):
        bad = p.copy()
        if col is None:
            bad[0, 3:7] = 0
        else:
            bad[0, col] = val
        out = R.reanchor(mu, cov, np.zeros(4, np.int32), 4, a, bad)
        assert out["held"] == 1 and out["moved"] == 0
        assert (out["anchor"] == a).all() and (out["means"] == mu).all()
    # labels -1 and n_kf are untouched; rows at and past the count too
    out = R.reanchor(mu, cov, np.array([-1, 1, 0, 0], np.int32), 3, a, p)
    assert out["mask"].tolist() == [False, False, True, False] and out["moved"] == 1
    assert (out["means"][[0, 1, 3]] == mu[[0, 1, 3]]).all()


def test_sensitivity(parity):
    """Dropping s^2 on the covariance, R_o^T, or the quaternion normalisation
    (input |q| off by 1e-3) moves the float64 result by far more than the
    tolerance."""
    c, ref = base_case()
    tm, tc = tolerance()
    off = dict(c)
    off["anchor"], off["poses"] = c["anchor"].copy(), c["poses"].copy()
    off["anchor"][:, 3:7] *= np.float32(1.001)
    off["poses"][:, 3:7] *= np.float32(0.999)
    ref_off = _ref(off)
    for name, case, want in (("no_s2", c, ref), ("no_RoT", c, ref), ("no_norm", off, ref_off)):
        v = _ref(case, variant=name)
        em, ec = R.errors(v["means"], v["cov"], want)
        parity(f"reanchor_sensitivity_{name}", err=max(em / tm, ec / tc), tol=100.0,
               mean_factor=em / tm, cov_factor=ec / tc)
        assert max(em / tm, ec / tc) > 100, (name, em, ec)
    # the normalisation itself: the off-norm input gives the unit-norm result
    em, ec = R.errors(ref_off["means"], ref_off["cov"], ref)
    assert em < tm and ec < tc


# ------------------------------------------- CPU: the arithmetic, host build
@functools.lru_cache(maxsize=None)
def _host_exe():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    import atexit
    import tempfile
    d = tempfile.mkdtemp(prefix="map_reanchor_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "map_reanchor_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(REPO, "splatt3r-slam_amd", "csrc"),
                    "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "native", "map_reanchor_host.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _host_run(c):
    exe = _host_exe()
    if exe is None:
        pytest.skip("hipcc not available")
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        for a in (c["means"], c["cov"], c["kf"], c["anchor"], c["poses"]):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.run([exe, fin, fout, str(c["n"]), str(c["cap"]), str(c["n_kf"])], check=True,
                   timeout=60)
    raw = open(fout, "rb").read()
    cap, n_kf = c["cap"], c["n_kf"]
    o = 0
    means = np.frombuffer(raw, np.float32, cap * 3, o).reshape(cap, 3); o += cap * 12
    cov = np.frombuffer(raw, np.float32, cap * 6, o).reshape(cap, 6); o += cap * 24
    anchor = np.frombuffer(raw, np.float32, n_kf * 8, o).reshape(n_kf, 8); o += n_kf * 32
    moved, held = np.frombuffer(raw, np.int64, 2, o)
    return dict(means=means, cov=cov, anchor=anchor, moved=int(moved), held=int(held))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                          np.ascontiguousarray(b).view(np.uint32))


def _check(c, ref, got, parity=None, key=None):
    """Everything a result must satisfy against the float64 reference."""
    tm, tc = tolerance()
    em, ec = R.errors(got["means"], got["cov"], ref)
    if parity is not None:
        parity(key + "_mean", err=em, tol=tm)
        parity(key + "_cov", err=ec, tol=tc)
    assert em <= tm and ec <= tc, (em, tm, ec, tc)
    still = ~ref["mask"]
    assert _same_bits(got["means"][still], c["means"][still])
    assert _same_bits(got["cov"][still], c["cov"][still])
    assert got["moved"] == ref["moved"] and got["held"] == ref["held"]
    assert _same_bits(got["anchor"], ref["anchor"])


def test_host_math_matches_ref64(parity):
    c, ref = base_case()
    assert ref["moved"] > 500 and ref["held"] == 2 and (~ref["mask"][:1000]).sum() > 100
    _check(c, ref, _host_run(c), parity, "reanchor_host")


# -------------------------------------------------------------------- GPU ---
def _gpu_map(c, max_keyframes=64):
    import torch
    from splatt3r_amd.gaussian_map import SharedGaussians
    gm = SharedGaussians(max_gaussians=c["cap"], device="cuda", max_keyframes=max_keyframes)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gm.means.copy_(t(c["means"]))
    gm.cov_triu.copy_(t(c["cov"]))
    gm.colors.copy_(t(c["colors"]))
    gm.opacities.copy_(t(c["opac"]))
    gm.kf_id.copy_(t(c["kf"]))
    gm._n.fill_(c["n"])
    gm._anchor_rows(c["n_kf"])[:c["n_kf"]] = t(c["anchor"])
    return gm


def _gpu_run(c, gm=None, poses=None, max_keyframes=64):
    """reanchor on the device -> host arrays; asserts on the device that
    colours, opacities, kf_id and the count kept their bits."""
    import torch
    gm = gm or _gpu_map(c, max_keyframes)
    before = [f.clone() for f in (gm.colors, gm.opacities, gm.kf_id, gm._n)]
    rows_before = gm.anchors.shape[0]
    poses = c["poses"] if poses is None else poses
    moved, held = gm.reanchor(torch.from_numpy(poses).cuda(), count=True)
    for a, b in zip(before, (gm.colors, gm.opacities, gm.kf_id, gm._n)):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    n_kf = len(poses)
    assert gm.anchors.shape[0] >= max(rows_before, n_kf)
    assert not gm.anchors[n_kf:].any()       # rows no keyframe names stay unset
    return dict(means=gm.means.cpu().numpy(), cov=gm.cov_triu.cpu().numpy(),
                anchor=gm.anchors[:n_kf].cpu().numpy(), moved=moved, held=held, gm=gm)


def _check_gpu_untouched(c, ref, got):
    """torch.equal on all five fields of every row that must not move."""
    import torch
    gm = got["gm"]
    still = torch.from_numpy(~ref["mask"]).cuda()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for f, src in ((gm.means, c["means"]), (gm.cov_triu, c["cov"]), (gm.colors, c["colors"]),
                   (gm.opacities, c["opac"]), (gm.kf_id, c["kf"])):
        assert torch.equal(f[still], t(src)[still])


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf", [1, 3, 64, 65, 300])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_hip_reanchor_matches_ref64(n, n_kf, parity):
    """Row counts around the workgroup size, keyframe counts around it and
    past one workgroup of k_reanchor_delta; capacity 1001 with sentinel rows
    (labelled 0, which moves) at and past the count; runs cut at rows 255,
    256, 257; every kind of keyframe (KINDS)."""
    c = make_case(n, n_kf, seed=100 * n_kf + n)
    ref = _ref(c)
    got = _gpu_run(c)
    _check(c, ref, got, parity, f"reanchor_n{n}_kf{n_kf}")
    _check_gpu_untouched(c, ref, got)
    assert (got["means"][n:] == SENTINEL).all() and (got["cov"][n:] == SENTINEL).all()
    if n >= 255:
        assert ref["moved"] > 0


@pytest.mark.gpu
def test_hip_reanchor_label_layouts(parity):
    """A wave with alternating moved and unmoved labels (0 moves, 2 is
    equal), moved labels alternating between two keyframes (0, 1: the wave
    does not share one delta), and labels -1, n_kf, INT32_MAX, INT32_MIN."""
    n, n_kf = 1000, 7
    lab = _run_labels(n, n_kf, list(range(300, n, 97)))
    lab[0:64] = np.where(np.arange(64) % 2 == 0, 0, 2)
    lab[64:128] = np.where(np.arange(64) % 2 == 0, 0, 1)
    lab[128:192] = np.resize(np.array([-1, n_kf, I32_MAX, I32_MIN, 0], np.int64),
                             64).astype(np.int32)
    c = make_case(n, n_kf, seed=7, labels=lab)
    ref = _ref(c)
    assert ref["mask"][0:64].sum() == 32 and ref["mask"][64:128].all()
    assert ref["mask"][128:192].sum() == 12
    got = _gpu_run(c)
    _check(c, ref, got, parity, "reanchor_layouts")
    _check_gpu_untouched(c, ref, got)


@pytest.mark.gpu
def test_hip_reanchor_is_pure():
    """A moved row is a function of its own inputs and the two pose rows:
    alone, inside the 1,000-row call, in a second run, on a non-default
    stream and through the staged path it has the same bits; a second call
    with the same poses leaves every byte of the map and the table equal."""
    import torch
    from splatt3r_amd import _lib
    c, ref = base_case()
    got = _gpu_run(c)
    _check(c, ref, got)
    again = _gpu_run(c)
    assert _same_bits(again["means"], got["means"]) and _same_bits(again["cov"], got["cov"])
    # alone: each of a few moved rows as a one-row map
    for i in np.flatnonzero(ref["mask"])[[0, 1, -1]]:
        one = dict(c, n=1, cap=1, **{k: c[k][i:i + 1] for k in ("means", "cov", "colors", "opac",
                                                                "kf")})
        g1 = _gpu_run(one)
        assert g1["moved"] == 1
        assert _same_bits(g1["means"][0], got["means"][i])
        assert _same_bits(g1["cov"][0], got["cov"][i])
    # the same poses again: nothing moves, nothing is written
    gm = got["gm"]
    second = _gpu_run(c, gm=gm)
    assert (second["moved"], second["held"]) == (0, ref["held"])
    for k in ("means", "cov", "anchor"):
        assert _same_bits(second[k], got[k])
    # a non-default stream
    st = torch.cuda.Stream()
    gm_s = _gpu_map(c)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        on_stream = _gpu_run(c, gm=gm_s)
    st.synchronize()
    # the staged path
    _lib.lib().s3a_set_path(1)
    try:
        staged = _gpu_run(c)
        staged_small = _gpu_run(make_case(257, 3, seed=5, cap=300))
    finally:
        _lib.lib().s3a_set_path(0)
    direct_small = _gpu_run(make_case(257, 3, seed=5, cap=300))
    for other, want in ((on_stream, got), (staged, got), (staged_small, direct_small)):
        for k in ("means", "cov", "anchor"):
            assert _same_bits(other[k], want[k])
        assert (other["moved"], other["held"]) == (want["moved"], want["held"])


@pytest.mark.gpu
def test_hip_reanchor_rejects_bad_arguments():
    import ctypes
    import torch
    from splatt3r_amd import _lib
    c, _ = base_case()
    gm = _gpu_map(c)
    lib = _lib.lib()
    ws = torch.empty(7 * 16, dtype=torch.float64, device="cuda")
    poses = torch.from_numpy(c["poses"]).cuda()
    args = lambda n_kf, nbytes: (ctypes.byref(gm._c), gm.anchors.data_ptr(), poses.data_ptr(),
                                 n_kf, None, None, ws.data_ptr(), nbytes, None)
    assert lib.s3a_reanchor_workspace_bytes(7) == 7 * 128
    assert lib.s3a_reanchor_workspace_bytes(0) == 0
    assert lib.s3a_map_reanchor(*args(0, 7 * 128)) == 1
    assert b"n_kf" in lib.s3_last_error()
    assert lib.s3a_map_reanchor(*args(7, 7 * 128 - 1)) == 1
    assert b"workspace" in lib.s3_last_error()
    torch.cuda.synchronize()
    assert _same_bits(gm.means.cpu().numpy(), c["means"])


@pytest.mark.gpu
def test_hip_reanchor_chain_of_50(parity):
    """50 successive re-anchors through random valid poses with s = 1 against
    ref64 going straight from the first poses to the last.  With s = 1 every
    pass preserves norms, so per-pass errors add at most linearly: the bound
    is 50 x the single-pass tolerance."""
    import torch
    rng = np.random.default_rng(11)
    n, n_kf = 1000, 7
    c = make_case(n, n_kf, seed=12, unit_scale=True)
    c["anchor"] = _poses(rng, n_kf, unit_scale=True)      # every keyframe set and valid
    chain = [_poses(rng, n_kf, unit_scale=True) for _ in range(50)]
    c["poses"] = chain[-1]
    ref = _ref(c)
    assert ref["moved"] == n
    gm = _gpu_map(c)
    first = None
    for p in chain:
        gm.reanchor(torch.from_numpy(p).cuda())
        if first is None:
            first = (gm.means.cpu().numpy(), gm.cov_triu.cpu().numpy())
    tm, tc = tolerance()
    step = R.reanchor(c["means"], c["cov"], c["kf"], n, c["anchor"], chain[0])
    em1, ec1 = R.errors(*first, step)
    em, ec = R.errors(gm.means.cpu().numpy(), gm.cov_triu.cpu().numpy(), ref)
    parity("reanchor_chain50_mean", err=em, tol=50 * tm, one_pass=em1, growth=em / em1)
    parity("reanchor_chain50_cov", err=ec, tol=50 * tc, one_pass=ec1, growth=ec / ec1)
    assert em <= 50 * tm and ec <= 50 * tc, (em, ec)
    assert _same_bits(gm.anchors[:n_kf].cpu().numpy(), chain[-1])


@pytest.mark.gpu
def test_hip_reanchor_commutes_with_gaussians_to_world(parity):
    """Four synthetic 24 x 32 predicted views placed under poses A (map A,
    one set_anchor per view) and under poses B (map B): reanchor(B) on map A
    agrees with map B.  Baseline: the float64 re-anchor of map A against map
    B, the distance between two float32 pipelines; bound: that plus the
    kernel tolerance."""
    import torch
    import lietorch
    from splatt3r_amd.gaussian_map import SharedGaussians
    from splatt3r_amd.splatt3r_utils import _sim3_to_4x4, world_records
    rng = np.random.default_rng(21)
    H, W, V = 24, 32, 4
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    views = []
    for _ in range(V):
        means = np.concatenate([rng.uniform(-1, 1, (H, W, 2)), rng.uniform(0.5, 4, (H, W, 1))], -1)
        views.append((dict(means=t(means), scales=t(rng.uniform(0.005, 0.1, (H, W, 3))),
                           rotations=t(_unit_quats(rng, H * W).reshape(H, W, 4)),
                           sh=t(rng.normal(size=(H, W, 3, 1)) * 0.3),
                           opacities=t(rng.uniform(0.05, 1, (H, W)))),
                      t(rng.normal(size=(3, H, W)))))
    PA, PB = _poses(rng, V, tmax=10.0), _poses(rng, V, tmax=10.0)
    assert (np.abs(PA[:, 7] - 1) > 1e-3).all() and (np.abs(PB[:, 7] - 1) > 1e-3).all()

    def build(P):
        gm = SharedGaussians(max_gaussians=4096, device=dev)
        for k, (view, img) in enumerate(views):
            T = lietorch.Sim3(t(P[k:k + 1]))
            rec, cnt = world_records(view, img, _sim3_to_4x4(T)[0].to(dev))
            gm.set_anchor(k, T)
            gm.append_records(rec, cnt, k, 0.3)
        return gm

    A, B = build(PA), build(PB)
    n = A.n_gaussians
    assert n == B.n_gaussians and 1000 < n < V * H * W
    host = lambda gm: dict(means=gm.means[:n].cpu().numpy(), cov=gm.cov_triu[:n].cpu().numpy(),
                           kf=gm.kf_id[:n].cpu().numpy())
    a, b = host(A), host(B)
    assert _same_bits(A.anchors[:V].cpu().numpy(), PA)
    ref = R.reanchor(a["means"], a["cov"], a["kf"], n, PA, PB)
    assert ref["moved"] == n
    base_m, base_c = R.errors(b["means"], b["cov"], ref)
    moved, held = A.reanchor(lietorch.Sim3(t(PB)), count=True)
    assert (moved, held) == (n, 0)
    got = host(A)
    em, ec = R.errors(got["means"], got["cov"], ref, b["means"], b["cov"])
    tm, tc = tolerance()
    parity("reanchor_commute_mean", err=em, tol=base_m + tm, baseline=base_m)
    parity("reanchor_commute_cov", err=ec, tol=base_c + tc, baseline=base_c)
    assert em <= base_m + tm and ec <= base_c + tc, (em, base_m, ec, base_c)
    assert torch.equal(A.colors[:n], B.colors[:n]) and torch.equal(A.opacities[:n], B.opacities[:n])
    assert torch.equal(A.kf_id[:n], B.kf_id[:n])
    assert _same_bits(A.anchors[:V].cpu().numpy(), PB)


# --------------------------------------------------------------- Frontend ---
FRONTEND_FRAMES = 6


@functools.lru_cache(maxsize=None)
def _model_and_frames():
    import torch
    from splatt3r_amd.splatt3r_utils import load_splatt3r
    from splatt3r_amd.synthetic import tum_like_sequence
    from splatt3r_amd.weights import FULL
    dev = torch.device("cuda", 0)
    model = load_splatt3r(None, device=dev, cfg=FULL, seed=1234, symmetric=True)
    return dev, model, tum_like_sequence(FRONTEND_FRAMES, 384, 512, seed=3, step_px=2.0,
                                         device=dev)


def _run_frontend(follow):
    """Step until there are >= 2 keyframes and a tracked (non-keyframe)
    append; returns the frontend and the (label, keyframes) of each tracked
    append."""
    from splatt3r_amd.slam import Frontend
    dev, model, frames = _model_and_frames()
    fe = Frontend(model, device=dev, spatial_stride=4, render=False, viz=True,
                  max_gaussians=20000, map_follow_poses=follow)
    fe.map_opacity_threshold = 0.1
    # this slow pan never travels main.py's 0.12 between keyframes: let every
    # tracked frame append, so that non-keyframe appends occur
    fe.min_translation, fe.min_frame_gap = 0.0, 1
    tracked = []
    for i in range(len(frames)):
        fe.step(i, frames[i])
        if fe.last_append_idx == i and i not in fe.new_kf_frames:
            n = fe.gmap.n_gaussians
            tracked.append((int(fe.gmap.kf_id[n - 1]), len(fe.keyframes)))
        if len(fe.keyframes) >= 2 and tracked:
            break
    assert len(fe.keyframes) >= 2 and tracked, (len(fe.keyframes), tracked)
    return fe, tracked


def _perturbed(fe, k):
    import torch
    p = fe.keyframes[k].T_WC.data.reshape(1, 8).clone()
    p[0, :3] += torch.tensor([0.05, -0.02, 0.03], device=p.device)
    q = p[0, 3:7] + torch.tensor([0.02, -0.01, 0.03, 0.0], device=p.device)
    p[0, 3:7] = q / q.norm()
    p[0, 7] *= 1.03
    return p


def _snapshot(gm):
    n = gm.n_gaussians
    return dict(n=n, means=gm.means.cpu().numpy(), cov=gm.cov_triu.cpu().numpy(),
                colors=gm.colors.cpu().numpy(), opac=gm.opacities.cpu().numpy(),
                kf=gm.kf_id.cpu().numpy())


@pytest.mark.gpu
def test_frontend_map_follows_keyframe_poses(parity):
    fe, tracked = _run_frontend(True)
    try:
        # a tracked append carries the label of the keyframe it was tracked against
        assert all(label == n_kf - 1 for label, n_kf in tracked), tracked
        gm = fe.gmap
        assert fe.sync_map() == (0, 0)        # every label sits under its installed pose
        snap = _snapshot(gm)
        n_kf = len(fe.keyframes)
        anchor = gm.anchors[:n_kf].cpu().numpy()
        assert _same_bits(anchor, fe.keyframes.get_poses().data.reshape(-1, 8).cpu().numpy())
        fe.keyframes.set_poses([1], _perturbed(fe, 1))
        poses = fe.keyframes.get_poses().data.reshape(-1, 8).cpu().numpy()
        moved, held = fe.sync_map()
        ref = R.reanchor(snap["means"], snap["cov"], snap["kf"], snap["n"], anchor, poses)
        assert held == 0 and moved == ref["moved"] == int((snap["kf"][:snap["n"]] == 1).sum()) > 0
        after = _snapshot(gm)
        got = dict(means=after["means"], cov=after["cov"], moved=moved, held=held,
                   anchor=gm.anchors[:n_kf].cpu().numpy())
        _check(snap, ref, got, parity, "reanchor_frontend")
        for k in ("colors", "opac", "kf"):
            assert _same_bits(after[k], snap[k])
        assert after["n"] == snap["n"]
        assert fe.sync_map() == (0, 0)
    finally:
        fe.close()


@pytest.mark.gpu
def test_frontend_map_follows_a_single_thread_backend(parity):
    """With a backend that solves inside the step (no worker thread, poses
    written without apply_pending) the map still ends under the solved poses.
    A shadow map receives the same appends and is never re-anchored; its rows,
    re-anchored in float64 from the poses they were placed under straight to
    the final ones, are the reference.  The followed map went through at most
    one pass per step, each within the single-pass tolerance of the exact
    value, and the solves move the poses by little, so the errors add at most
    linearly: the bound is (number of steps) x the tolerance."""
    import torch
    from splatt3r_amd.backend import Backend
    from splatt3r_amd.frame import Keyframes
    from splatt3r_amd.gaussian_map import SharedGaussians
    from splatt3r_amd.slam import Frontend
    from splatt3r_amd.synthetic import tum_like_sequence
    dev, model, _ = _model_and_frames()
    steps = 10
    frames = tum_like_sequence(steps, 384, 512, seed=3, step_px=4.0, device=dev)
    be = Backend(model, Keyframes(), device=dev)
    fe = Frontend(model, device=dev, spatial_stride=4, render=False, viz=True,
                  max_gaussians=20000, backend=be, map_follow_poses=True)
    fe.map_opacity_threshold = 0.1
    gm = fe.gmap
    shadow = SharedGaussians(max_gaussians=20000, device=dev)
    placed = {}
    append_records, set_anchor = gm.append_records, gm.set_anchor

    def spy_append(records, count, kf_idx, opacity_threshold=0.05):
        shadow.append_records(records, count, kf_idx, opacity_threshold)
        return append_records(records, count, kf_idx, opacity_threshold)

    def spy_anchor(kf_idx, T_WC=None):
        if T_WC is not None:
            placed[kf_idx] = T_WC.data.reshape(8).cpu().numpy().copy()
        return set_anchor(kf_idx, T_WC)

    gm.append_records, gm.set_anchor = spy_append, spy_anchor
    try:
        for i in range(steps):
            fe.step(i, frames[i])
        n_kf = len(fe.keyframes)
        assert n_kf >= 3 and sorted(placed) == list(range(n_kf))
        fe.sync_map()
        assert fe.sync_map() == (0, 0)
        poses = fe.keyframes.get_poses().data.reshape(-1, 8).cpu().numpy()
        assert _same_bits(gm.anchors[:n_kf].cpu().numpy(), poses)
        anchor = np.stack([placed[k] for k in range(n_kf)])
        changed = [k for k in range(n_kf) if not _same_bits(anchor[k], poses[k])]
        assert changed, "the backend moved no keyframe: the test shows nothing"
        s, f = _snapshot(shadow), _snapshot(gm)
        assert s["n"] == f["n"] > 0
        for k in ("colors", "opac", "kf"):
            assert _same_bits(s[k], f[k])
        ref = R.reanchor(s["means"], s["cov"], s["kf"], s["n"], anchor, poses)
        assert ref["moved"] == int(np.isin(s["kf"][:s["n"]], changed).sum()) > 0
        em, ec = R.errors(f["means"], f["cov"], ref)
        tm, tc = tolerance()
        parity("reanchor_backend_mean", err=em, tol=steps * tm, keyframes_moved=len(changed))
        parity("reanchor_backend_cov", err=ec, tol=steps * tc)
        assert em <= steps * tm and ec <= steps * tc, (em, ec)
        still = ~ref["mask"]
        assert _same_bits(f["means"][still], s["means"][still])
        assert _same_bits(f["cov"][still], s["cov"][still])
    finally:
        fe.close()


@pytest.mark.gpu
def test_frontend_map_ignores_poses_by_default():
    fe, tracked = _run_frontend(False)
    try:
        # the reference's label: len(keyframes) at the time of the append
        assert all(label == n_kf for label, n_kf in tracked), tracked
        snap = _snapshot(fe.gmap)
        fe.keyframes.set_poses([1], _perturbed(fe, 1))
        assert fe.sync_map() is None
        after = _snapshot(fe.gmap)
        assert after["n"] == snap["n"]
        for k in ("means", "cov", "colors", "opac", "kf"):
            assert _same_bits(after[k], snap[k])
        assert not fe.gmap.anchors.any()
    finally:
        fe.close()
