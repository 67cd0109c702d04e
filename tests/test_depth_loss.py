"""Depth loss and depth-metric sums: the arithmetic
(csrc/depth_loss_math.hpp), the HIP kernels (csrc/depth_loss.hip,
include/s3z.h), splatt3r_amd.depth, and the host-side pieces that feed them
(ingest.resize_depth, TUMDataset.read_depth, write_synthetic_tum(depth=True)).

Reference: tests/depth_loss_ref64.py -- numpy float64, one IEEE operation per
operation of the definition, sums added exactly.  Tolerances:

  rmap, grad_depth, grad_alpha, D1..D3, N   exact, bit for bit: every value is
      a fixed sequence of double operations rounded once to float32 (or a
      count), and neither side contracts.
  every other sum   n 2^-52 relative, n = H W: all addends are >= 0 and are
      the same doubles on both sides, so only the order of at most 2 n
      additions differs, each within 2^-53 of the running sum.
  LOGSQ   additionally n 2^-48 max(1, max |log z|)^2 absolute: log is not
      correctly rounded, and libm's, the device's and numpy's may differ by
      an ulp or two in each of the two logs of a pixel.

One table of cases (depth_loss_ref64.cases()) is run twice: by the host
program tests/native/depth_loss_host.cpp, which runs the same header on the
CPU, and by the kernels.
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import depth_loss_ref64 as R
from conftest import REPO

f32, f64 = np.float32, np.float64
bits = lambda x: np.ascontiguousarray(np.asarray(x, f32)).view(np.int32)


@functools.lru_cache(maxsize=None)
def want(name):
    """(sums, rmap, grad_depth, grad_alpha) of a case, computed once."""
    c = R.cases()[name]
    sums, rmap = R.forward(*R.case_args(c))
    gd, ga = R.backward(c["D"], c["A"], c["z"], c["coef"], c["w"], c["s"], c["alpha_min"])
    return sums, rmap, gd, ga


def _compare(name, got_sums, got_maps, label, parity):
    """got_maps: (rmap, grad_depth, grad_alpha).  The split of the module docstring."""
    c = R.cases()[name]
    sums, *maps = want(name)
    B, H, W = c["D"].shape
    n = H * W
    bad = sum(int((bits(g).reshape(-1) != bits(w).reshape(-1)).sum())
              for g, w in zip(got_maps, maps))
    parity(f"{label}.{name}.maps", err=float(bad), tol=0.0)
    for g, w, what in zip(got_maps, maps, ("rmap", "grad_depth", "grad_alpha")):
        assert np.array_equal(bits(g).reshape(-1), bits(w).reshape(-1)), (label, name, what)
    got_sums = np.asarray(got_sums, f64).reshape(B, len(R.NAMES))
    valid = R.pixels(*R.case_args(c))[0]
    worst = 0.0
    for b in range(B):
        zv = c["z"][b][valid[b]].astype(f64)
        logmax = float(np.abs(np.log(zv)).max()) if zv.size else 0.0
        for k, i in R.IDX.items():
            g, w = got_sums[b, i], sums[b, i]
            if k in R.COUNTS:
                assert g == w, (label, name, b, k, g, w)
                continue
            tol = n * 2.0 ** -52 * abs(w)
            if k == "LOGSQ":
                tol += n * 2.0 ** -48 * max(1.0, logmax) ** 2
            err = abs(g - w)
            print(f"{label}.{name}[{b}].{k}: got {g!r} want {w!r} err {err:.3e} tol {tol:.3e}")
            worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else np.inf))
            assert err <= tol, (label, name, b, k, g, w, err, tol)
    parity(f"{label}.{name}.sums", err=worst, tol=1.0)


# ---------------------------------------------------- CPU: the reference --
def test_inputs_cover_the_cases():
    c = R.cases()
    tw, th = R.tile()
    assert (tw, th) == (64, 8)
    for H, W in ((1, 1), (1, tw + 1), (th + 1, 1), (th - 1, tw - 1), (th, tw), (th + 1, tw + 1),
                 (2 * th + 3, tw + 5)):
        assert c[f"plain_{H}x{W}"]["D"].shape == (1, H, W)
        assert c[f"dirty_{H}x{W}"]["D"].shape == (2, H, W)
    big = c[f"dirty_{2 * th + 3}x{tw + 5}"]
    z, A, D, w = big["z"], big["A"], big["D"], big["w"]
    assert np.isnan(z).any() and np.isposinf(z).any() and (z == 0).any() and (z < 0).any()
    assert (A < 0.5).any() and (A == 0.5).any() and (A > 0.5).any() and big["alpha_min"] == 0.5
    assert ((A == 0) & (D == 0)).any()
    assert (w == 0).any() and ((w > 0) & (w != 1)).any()
    assert big["s"] is not None and c[f"plain_{th}x{tw}"]["s"] is None
    valid = R.pixels(*R.case_args(big))[0]
    assert valid[(A == 0.5) & np.isfinite(z) & (z > 0) & (w > 0) & np.isfinite(D)].all()
    assert not valid[A < 0.5].any() and 0.5 < valid.mean() < 0.9
    # pairs that straddle a tile boundary with one end invalid, in x and in y, and a corner
    assert (valid[:, :, tw - 1] != valid[:, :, tw]).any()
    assert (valid[:, th - 1, :] != valid[:, th, :]).any()
    assert (valid[:, 2 * th - 1, :] != valid[:, 2 * th, :]).any()
    corner = valid[:, th - 1:th + 1, tw - 1:tw + 1].reshape(2, 4)
    assert (~corner).any() and corner.any()
    # a wholly invalid image in a batch of three
    b3 = c["batch_one_invalid"]
    v3 = R.pixels(*R.case_args(b3))[0]
    assert b3["D"].shape[0] == 3 and not v3[1].any() and v3[0].any() and v3[2].any()
    assert want("batch_one_invalid")[0][1].tolist() == [0.0] * len(R.NAMES)
    # r = 0 exactly and r_p = r_q exactly
    for name in ("sign_zero", "sign_zero_scaled"):
        r = R.pixels(*R.case_args(c[name]))[4][0]
        H, W = r.shape
        assert (r[H // 2:, :W - 3] == 0).all() and (r[:H // 2, :W - 3] == 0.25).all()
        assert (r[:, W - 3:] != 0).all()
    # the kink-free case: no |r| and no |r_p - r_q| below 1e-3
    k = c["kink_free"]
    valid, w, _, _, r = R.pixels(*R.case_args(k))
    assert (np.abs(r[valid]) >= 1e-3).all() and not valid[1, 3:6, 10:20].any()
    for axis in (1, 2):
        both, _, d = R._pairs(valid, w, r, axis)
        assert both.sum() > 1000 and (np.abs(d[both]) >= 1e-3).all()


def test_reference_cases_worked_by_hand():
    a = lambda *v: np.array(v, f32)
    # 1 x 2: r = (1, -2), weights (1, 3), one pair of weight 2
    D, A, z, w = (a(*v).reshape(1, 1, 2) for v in ((2, 3), (1, 1), (1, 5), (1, 3)))
    sums, rmap = R.forward(D, A, z, w)
    assert rmap.reshape(-1).tolist() == [1.0, -2.0]
    got = dict(zip(R.NAMES, sums[0]))
    assert got == dict(W=4.0, ABS=7.0, SQ=13.0, ABSREL=1.0 + 6.0 / 5.0, SQREL=1.0 + 12.0 / 5.0,
                       LOGSQ=got["LOGSQ"], GRAD=6.0, WG=2.0, D1=0.0, D2=0.0, D3=1.0, N=2.0,
                       QZ=47.0, QQ=31.0)
    assert got["LOGSQ"] == pytest.approx(np.log(2.0) ** 2 + 3 * np.log(0.6) ** 2, rel=1e-14)
    gd, ga = R.backward(D, A, z, a(1, 1, 1).reshape(1, 3), w)
    # dL/dr = 1 (1 + 2) + 2 sign(3) = 5 and 3 (-1 - 4) + 2 sign(-3) = -17
    assert gd.reshape(-1).tolist() == [5.0, -17.0] and ga.reshape(-1).tolist() == [-10.0, 51.0]
    # 2 x 1, scale 2, the lower pixel below alpha_min: no pair
    D, A, z = (a(*v).reshape(1, 2, 1) for v in ((1, 1), (1, 0.25), (1, 1)))
    sums, rmap = R.forward(D, A, z, None, a(2))
    got = dict(zip(R.NAMES, sums[0]))
    assert rmap.reshape(-1).tolist() == [1.0, 0.0]
    assert [got[k] for k in ("W", "ABS", "SQ", "GRAD", "WG", "N", "QZ", "QQ", "D1", "D3")] == \
        [1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    assert got["LOGSQ"] == np.log(2.0) ** 2
    gd, ga = R.backward(D, A, z, a(1, 0, 1).reshape(1, 3), None, a(2))
    assert gd.reshape(-1).tolist() == [2.0, 0.0] and ga.reshape(-1).tolist() == [-2.0, 0.0]
    # sign(0) = 0: r = 0 everywhere gives no gradient, whatever the coefficients
    D = A = z = np.ones((1, 3, 3), f32)
    gd, ga = R.backward(D, A, z, a(1, 1, 1).reshape(1, 3))
    assert not gd.any() and not ga.any()


def test_reference_gradients_match_float64_autograd():
    """ref64's gradients (before their rounding to float32) against torch
    float64 autograd of the same expression on the CPU, on the kink-free case;
    both sides are double, so rtol 1e-12."""
    c = R.cases()["kink_free"]
    valid = torch.from_numpy(R.pixels(*R.case_args(c))[0])
    t64 = lambda x: torch.from_numpy(x.astype(f64))
    D, A = t64(c["D"]).requires_grad_(True), t64(c["A"]).requires_grad_(True)
    z, w, s, coef = t64(c["z"]), t64(c["w"]), t64(c["s"])[:, None, None], t64(c["coef"])
    safe = torch.where(valid, z, torch.ones_like(z))
    r = torch.where(valid, s * (D / A) - safe, torch.zeros_like(z))
    wv = torch.where(valid, w, torch.zeros_like(w))
    ABS, SQ = (wv * r.abs()).sum((1, 2)), (wv * r * r).sum((1, 2))
    GRAD = 0
    for a_, b_ in (((slice(None), slice(None), slice(None, -1)), (slice(None), slice(None), slice(1, None))),
                   ((slice(None), slice(None, -1)), (slice(None), slice(1, None)))):
        both = valid[a_] & valid[b_]
        GRAD = GRAD + (both * 0.5 * (w[a_] + w[b_]) * (r[b_] - r[a_]).abs()).sum((1, 2))
    (coef[:, 0] * ABS + coef[:, 1] * SQ + coef[:, 2] * GRAD).sum().backward()
    gd, ga = R.backward64(c["D"], c["A"], c["z"], c["coef"], c["w"], c["s"], c["alpha_min"])
    for got, ref, what in ((gd, D.grad.numpy(), "depth"), (ga, A.grad.numpy(), "alpha")):
        assert np.abs(ref[valid.numpy()]).min() > 0
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, err_msg=what)


# ------------------------------------------- CPU: the arithmetic, host build
@functools.lru_cache(maxsize=None)
def _host_exe():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    import atexit
    import tempfile
    d = tempfile.mkdtemp(prefix="depth_loss_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "depth_loss_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(REPO, "splatt3r-slam_amd", "csrc"),
                    "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "native", "depth_loss_host.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_host_program_vs_ref64(name, parity):
    exe = _host_exe()
    if exe is None:
        pytest.skip("hipcc not available")
    c = R.cases()[name]
    B, H, W = c["D"].shape
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        for k in ("D", "A", "z", "w", "s", "coef"):
            if c[k] is not None:
                f.write(c[k].tobytes())
    subprocess.run([exe, fin, fout, str(B), str(H), str(W), str(int(c["w"] is not None)),
                    str(int(c["s"] is not None)), repr(c["alpha_min"])], check=True, timeout=300)
    raw = open(fout, "rb").read()
    n = B * H * W
    sums = np.frombuffer(raw, f64, B * len(R.NAMES), 0)
    o = sums.nbytes
    maps = [np.frombuffer(raw, f32, n, o + 4 * n * k) for k in range(3)]
    assert o + 12 * n == len(raw)
    _compare(name, sums, maps, "host", parity)


# ------------------------------------------------------------ CPU: the ABI --
def test_abi_rejects_bad_arguments_before_any_device_work():
    """Status 1 (3 for the workspace) with a message; the pointers are never
    dereferenced (they are not device memory here)."""
    from splatt3r_amd import _abi, _lib
    lib = _lib.lib()
    C = _abi.constants
    assert C["S3Z_NSUMS"] == 14 and len(R.NAMES) == 14
    assert [C["S3Z_SUM_" + k] for k in R.NAMES] == list(range(14))
    sig = _abi.functions["s3z_forward"][1]
    assert len(sig) == 13 and sig[8] is ctypes.c_double and sig[5] is ctypes.c_int
    assert _abi.functions["s3z_backward"][1][9] is ctypes.c_double
    assert _abi.functions["s3z_workspace_bytes"][0] is ctypes.c_size_t

    def fwd(d=0x1000, a=0x2000, z=0x3000, w=0x4000, s=0x5000, B=1, H=4, W=4, am=0.5, rmap=0x6000,
            sums=0x7000, ws=0x8000):
        return lib.s3z_forward(d, a, z, w, s, B, H, W, am, rmap, sums, ws, None)

    def bwd(d=0x1000, a=0x2000, z=0x3000, w=0x4000, s=0x5000, coef=0x5100, B=1, H=4, W=4, am=0.5,
            gd=0x6000, ga=0x7000):
        return lib.s3z_backward(d, a, z, w, s, coef, B, H, W, am, gd, ga, None)
    for kw, msg in ((dict(d=None), b"must not be NULL"), (dict(a=None), b"must not be NULL"),
                    (dict(z=None), b"must not be NULL"), (dict(sums=None), b"sums"),
                    (dict(B=0), b"B = 0"), (dict(B=-1), b"B = -1"), (dict(H=0), b"image size"),
                    (dict(W=-3), b"image size"), (dict(W=1 << 20), b"image size"),
                    (dict(am=-0.1), b"alpha_min"), (dict(am=float("nan")), b"alpha_min"),
                    (dict(am=float("inf")), b"alpha_min"), (dict(d=0x1002), b"aligned"),
                    (dict(rmap=0x1000), b"rmap overlaps"), (dict(rmap=0x3020), b"rmap overlaps"),
                    (dict(sums=0x7004), b"sums")):
        assert fwd(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    assert fwd(ws=None) == 3 and b"workspace" in lib.s3_last_error()
    for kw, msg in ((dict(d=None), b"must not be NULL"), (dict(coef=None), b"must not be NULL"),
                    (dict(gd=None), b"must not be NULL"), (dict(ga=None), b"must not be NULL"),
                    (dict(B=0), b"B = 0"), (dict(H=0), b"image size"),
                    (dict(am=-1.0), b"alpha_min"), (dict(am=float("nan")), b"alpha_min"),
                    (dict(gd=0x2000), b"grad_depth overlaps"), (dict(ga=0x4010), b"grad_alpha overlaps"),
                    (dict(ga=0x6020), b"each other")):
        assert bwd(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    tw, th = R.tile()
    assert lib.s3z_workspace_bytes(0, 4, 4) == 0 and lib.s3z_workspace_bytes(1, 0, 4) == 0
    assert lib.s3z_workspace_bytes(2, th + 1, tw + 1) == 2 * 4 * 14 * 8


def test_python_validation_needs_no_gpu():
    from splatt3r_amd import depth as Dm
    assert Dm.NSUMS == 14 and (Dm.TILE_W, Dm.TILE_H) == R.tile()
    assert (Dm.SUM_W, Dm.SUM_GRAD, Dm.SUM_QQ) == (R.IDX["W"], R.IDX["GRAD"], R.IDX["QQ"])
    z = torch.ones(2, 5, 7)
    for fn in (Dm.depth_sums, Dm.depth_loss, Dm.depth_metrics, Dm.depth_residuals):
        with pytest.raises(TypeError, match="float32"):
            fn(z.double(), z, z)
        with pytest.raises(TypeError, match="float32"):
            fn(z, z, z.half())
        with pytest.raises(TypeError, match="tensor"):
            fn(z, z.numpy(), z)
        with pytest.raises(ValueError, match=r"\[B, H, W\]"):
            fn(z[0], z[0], z[0])
        with pytest.raises(ValueError, match="alpha"):
            fn(z, z[:, :4], z)
        with pytest.raises(ValueError, match="weight"):
            fn(z, z, z, z[:1])
        with pytest.raises(RuntimeError, match="one device"):
            fn(z, z, z.to("meta"))
        with pytest.raises(ValueError, match="alpha_min"):
            fn(z, z, z, alpha_min=-1.0)
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(z, z, z)
    with pytest.raises(ValueError, match="scale"):
        Dm.depth_sums(z, z, z, scale=torch.ones(3))
    with pytest.raises(ValueError, match="scale"):
        Dm.depth_loss(z, z, z, scale=0.0)
    with pytest.raises(ValueError, match="align"):
        Dm.depth_metrics(z, z, z, align="median")
    with pytest.raises(ValueError, match="coef"):
        Dm.depth_backward(z, z, z, torch.ones(2, 4))
    # arithmetic on sums is plain torch
    sums = torch.zeros(3, 14, dtype=torch.float64)
    sums[:, Dm.SUM_QZ] = torch.tensor([2.0, 3.0, 5.0])
    sums[:, Dm.SUM_QQ] = torch.tensor([1.0, 0.0, 4.0])
    assert Dm.least_squares_scale(sums).tolist() == [2.0, 1.0, 1.25]
    assert Dm.least_squares_scale(sums, per_view=False).tolist() == [2.0, 2.0, 2.0]
    assert Dm.least_squares_scale(sums[1:2], per_view=False).tolist() == [1.0]


def test_refine_depth_arguments_need_no_gpu():
    from splatt3r_amd.refine import DepthControl, PoseControl, refine_splats
    rows, imgs = torch.zeros(4, 14), torch.zeros(2, 3, 12, 16)
    T, K = torch.eye(4).repeat(2, 1, 1), torch.eye(3)
    ok = DepthControl(torch.ones(2, 12, 16))
    assert ok.weight == 0.1 and (ok.l1_weight, ok.l2_weight, ok.grad_weight) == (1.0, 0.0, 0.0)
    with pytest.raises(NotImplementedError, match="poses"):
        refine_splats(rows, imgs, T, K, 3, depth=ok, poses=PoseControl())
    for bad in (torch.ones(3, 12, 16), torch.ones(2, 12, 17), torch.ones(2, 16, 12)):
        with pytest.raises(ValueError, match=r"targets must be \[2, 12, 16\]"):
            refine_splats(rows, imgs, T, K, 3, depth=DepthControl(bad))
    with pytest.raises(TypeError, match="DepthControl"):
        refine_splats(rows, imgs, T, K, 3, depth=torch.ones(2, 12, 16))
    with pytest.raises(ValueError, match="weights"):
        DepthControl(torch.ones(2, 12, 16), torch.ones(2, 12, 15))
    with pytest.raises(ValueError, match=r"\[V, H, W\]"):
        DepthControl(torch.ones(12, 16))
    for kw in (dict(weight=-1.0), dict(alpha_min=float("nan")), dict(scale=0.0), dict(grad_weight=-2)):
        with pytest.raises(ValueError):
            DepthControl(torch.ones(2, 12, 16), **kw)
    # without depth the checks are what they were: the rows must be on the GPU
    with pytest.raises(RuntimeError, match="GPU only"):
        refine_splats(rows, imgs, T, K, 3)


# ------------------------------------------------------ CPU: depth ingest --
@pytest.mark.parametrize("hw", ((480, 640), (640, 480), (512, 512), (384, 512), (300, 1000)))
def test_resize_depth_is_the_image_geometry_sampled_nearest(hw):
    from splatt3r_amd.ingest import ingest_geometry, resize_depth
    in_h, in_w = hw
    ramp = (np.arange(in_h)[:, None] * 4096 + np.arange(in_w)[None, :]).astype(f32)
    ramp[::7, ::5] = 0.0
    (W, H), _, box, _ = ingest_geometry(in_h, in_w, 512)
    got = resize_depth(ramp, 512)
    assert got.dtype == f32 and got.shape == (box[3] - box[1], box[2] - box[0])
    assert got.shape[0] % 16 == 0 and got.shape[1] % 16 == 0
    # every output pixel is the source pixel under its centre: never a blend
    ys = np.floor((np.arange(box[1], box[3]) + 0.5) * in_h / H).astype(int)
    xs = np.floor((np.arange(box[0], box[2]) + 0.5) * in_w / W).astype(int)
    assert ys.max() < in_h and xs.max() < in_w
    assert np.array_equal(got, ramp[np.ix_(ys, xs)])
    assert (got == 0).any() and np.isin(got, ramp).all()
    if hw == (512, 512):
        # a size that needs no resize: the crop of the input itself
        assert np.array_equal(got, ramp[box[1]:box[3], box[0]:box[2]])
    # the same geometry as the colour path
    from splatt3r_amd.splatt3r_utils import resize_img
    img = np.zeros((in_h, in_w, 3), f32)
    assert tuple(resize_img(img, 512)["unnormalized_img"].shape[:2]) == got.shape
    with pytest.raises(ValueError):
        resize_depth(np.zeros((3, 4, 5)), 512)


def _listing(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read()
            for d, _, fs in os.walk(root) for f in fs}


def test_tum_read_depth_round_trip(tmp_path):
    from splatt3r_amd import dataio
    root = dataio.write_synthetic_tum(tmp_path / "tum" / "seq", 4, H=48, W=64, depth=True)
    ds = dataio.TUMDataset(root)
    assert len(ds) == 4 and ds.use_calibration is False
    plane = np.broadcast_to(2.0 + 0.25 * np.arange(64) / 64, (48, 64))
    for i in range(4):
        d = ds.read_depth(i)
        assert d.dtype == f32 and d.shape == (48, 64)
        assert (d[:, :8] == 0).all() and (d[:, 8:] > 0).all()           # 0 stays invalid
        assert np.abs(d[:, 8:] - plane[:, 8:]).max() <= 1.0 / 5000.0
    # an RGB frame with no depth stamp within 0.02 s has no partner
    lines = (root / "depth.txt").read_text().splitlines()
    (root / "depth.txt").write_text("\n".join(lines[:-1]) + "\n")
    ds = dataio.TUMDataset(root)
    assert ds.read_depth(3) is None and ds.read_depth(2) is not None
    # a sequence without depth.txt has none at all
    plain = dataio.TUMDataset(dataio.write_synthetic_tum(tmp_path / "tum" / "plain", 2, H=48, W=64))
    assert plain.read_depth(0) is None
    # undistorted reading: refused
    ds.use_calibration = True
    with pytest.raises(NotImplementedError, match="undistort"):
        ds.read_depth(0)
    ds.use_calibration = False
    assert ds.read_depth(0).shape == (48, 64)


def test_write_synthetic_tum_defaults_write_what_they_wrote(tmp_path):
    from splatt3r_amd import dataio
    a = _listing(dataio.write_synthetic_tum(tmp_path / "a", 3, H=48, W=64))
    b = _listing(dataio.write_synthetic_tum(tmp_path / "b", 3, H=48, W=64, depth=False))
    c = _listing(dataio.write_synthetic_tum(tmp_path / "c", 3, H=48, W=64, depth=True))
    assert a == b and "rgb.txt" in a and len(a) == 4
    assert all(k.startswith("rgb") for k in a)
    extra = sorted(set(c) - set(a))
    assert len(extra) == 4 and "depth.txt" in extra and all(k.startswith("depth") for k in extra)
    assert {k: c[k] for k in a} == a


# --------------------------------------------------------------------- GPU --
def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_case(name):
    c = R.cases()[name]
    return {k: _cuda(c[k]) for k in ("D", "A", "z", "w", "s", "coef")}, c["alpha_min"]


def _run(t, am, rmap=True):
    from splatt3r_amd import depth as Dm
    if rmap:
        sums, r = Dm.depth_residuals(t["D"], t["A"], t["z"], t["w"], t["s"], am)
    else:
        sums, r = Dm.depth_sums(t["D"], t["A"], t["z"], t["w"], t["s"], am), None
    gd, ga = Dm.depth_backward(t["D"], t["A"], t["z"], t["coef"], t["w"], t["s"], am)
    return sums, r, gd, ga


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.cases()))
def test_hip_vs_ref64(name, parity):
    t, am = _dev_case(name)
    before = {k: v.clone() for k, v in t.items() if v is not None}
    sums, r, gd, ga = _run(t, am)
    _compare(name, sums.cpu().numpy(), [x.cpu().numpy() for x in (r, gd, ga)], "hip", parity)
    for k, v in before.items():                      # inputs left as they were
        assert torch.equal(v.view(torch.int32), t[k].view(torch.int32)), k


@pytest.mark.gpu
def test_hip_determinism_and_batch_independence():
    tw, th = R.tile()
    ib = lambda x: x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)
    for name in (f"dirty_{2 * th + 3}x{tw + 5}", "batch_one_invalid", "kink_free"):
        t, am = _dev_case(name)
        one, two = _run(t, am), _run(t, am)
        for a, b in zip(one, two):
            assert torch.equal(ib(a), ib(b)), name
        # image by image: the same bits as in the batch
        for b in range(t["D"].shape[0]):
            sub = {k: (None if v is None else v[b:b + 1].contiguous()) for k, v in t.items()}
            for a, full in zip(_run(sub, am), one):
                assert torch.equal(ib(a), ib(full[b:b + 1])), (name, b)


@pytest.mark.gpu
def test_hip_optional_inputs_absent_equal_their_explicit_form():
    from splatt3r_amd import depth as Dm
    tw, th = R.tile()
    ib = lambda x: x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)
    t, am = _dev_case(f"plain_{th + 1}x{tw + 1}")
    assert t["w"] is None and t["s"] is None
    full = dict(t, w=torch.ones_like(t["D"]), s=torch.ones(t["D"].shape[0], device="cuda"))
    for a, b in zip(_run(t, am), _run(full, am)):
        assert torch.equal(ib(a), ib(b))
    # no residual map: the same sums
    assert torch.equal(ib(_run(t, am, rmap=False)[0]), ib(_run(t, am)[0]))
    # a number for the scale is that number for every image
    t2, am = _dev_case("batch_one_invalid_noscale")
    s = Dm.depth_sums(t2["D"], t2["A"], t2["z"], scale=0.75)
    s3 = Dm.depth_sums(t2["D"], t2["A"], t2["z"], scale=torch.full((3,), 0.75, device="cuda"))
    assert torch.equal(ib(s), ib(s3))


@pytest.mark.gpu
def test_hip_depth_loss_autograd(parity):
    """The gradients reaching depth and alpha are s3z_backward with the
    coefficients the loss implies: (l1 / W, l2 / W, grad / WG) / B per image."""
    from splatt3r_amd import depth as Dm
    t, am = _dev_case("batch_one_invalid")
    l1, l2, lg = 0.7, 0.2, 0.4
    D, A = t["D"].clone().requires_grad_(True), t["A"].clone().requires_grad_(True)
    loss = Dm.depth_loss(D, A, t["z"], t["w"], t["s"], l1, l2, lg, am)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and torch.isfinite(loss)
    loss.backward()
    sums = want("batch_one_invalid")[0]
    B = sums.shape[0]
    W, WG = sums[:, R.IDX["W"]], sums[:, R.IDX["WG"]]
    assert W[1] == 0 and WG[1] == 0                    # the invalid image: both terms are 0
    den = lambda v: np.where(v > 0, v, 1.0)
    per = (l1 * sums[:, R.IDX["ABS"]] + l2 * sums[:, R.IDX["SQ"]]) / den(W) \
        + lg * sums[:, R.IDX["GRAD"]] / den(WG)
    assert float(loss.detach()) == pytest.approx(per.mean(), rel=1e-6)
    dsums = Dm.depth_sums(t["D"], t["A"], t["z"], t["w"], t["s"], am)
    one = torch.ones_like(dsums[:, 0])
    Wd = torch.where(dsums[:, Dm.SUM_W] > 0, dsums[:, Dm.SUM_W], one)
    WGd = torch.where(dsums[:, Dm.SUM_WG] > 0, dsums[:, Dm.SUM_WG], one)
    coef = (torch.stack([l1 / Wd, l2 / Wd, lg / WGd], 1) / B).to(torch.float32)
    gd, ga = Dm.depth_backward(t["D"], t["A"], t["z"], coef, t["w"], t["s"], am)
    bad = int((D.grad.view(torch.int32) != gd.view(torch.int32)).sum()
              + (A.grad.view(torch.int32) != ga.view(torch.int32)).sum())
    parity("hip.depth_loss.autograd", err=float(bad), tol=0.0)
    assert bad == 0 and gd.abs().sum() > 0
    assert not D.grad[1].any() and not A.grad[1].any()
    # a wholly invalid batch: loss 0, zero gradients, no NaN
    D, A = t["D"][1:2].clone().requires_grad_(True), t["A"][1:2].clone().requires_grad_(True)
    loss = Dm.depth_loss(D, A, t["z"][1:2], None, None, l1, l2, lg, am)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not D.grad.any() and not A.grad.any()
    assert torch.isfinite(D.grad).all() and torch.isfinite(A.grad).all()
    # target and weight never get a gradient
    z = t["z"].clone().requires_grad_(True)
    Dm.depth_loss(t["D"].clone().requires_grad_(True), t["A"], z, t["w"]).backward()
    assert z.grad is None


@pytest.mark.gpu
def test_hip_depth_metrics_and_alignment(parity):
    from splatt3r_amd import depth as Dm
    c = R.cases()["batch_one_invalid_noscale"]
    D, A = _cuda(c["D"]), _cuda(c["A"])
    q = (c["D"].astype(f64) / c["A"].astype(f64))
    # targets = 2.5 q: scale 2.5, abs_rel ~ 0, d1 = 1
    m = Dm.depth_metrics(D, A, _cuda((2.5 * q).astype(f32)), align="scale")
    assert sorted(m) == sorted(Dm.METRIC_NAMES)
    assert all(v.shape == (3,) and v.dtype == torch.float64 and v.is_cuda for v in m.values())
    h = {k: v.cpu().numpy() for k, v in m.items()}
    parity("hip.metrics.scale", err=float(np.abs(h["scale"] - 2.5).max()), tol=1e-6)
    parity("hip.metrics.abs_rel", err=float(h["abs_rel"].max()), tol=1e-6)
    assert np.abs(h["scale"] - 2.5).max() <= 1e-6 and h["abs_rel"].max() <= 1e-6
    assert (h["d1"] == 1).all() and (h["d3"] == 1).all() and (h["valid"] == 1).all()
    assert h["rmse"].max() < 1e-5 and h["rmse_log"].max() < 1e-6
    # without alignment the same targets are 2.5 x off
    h0 = {k: v.cpu().numpy() for k, v in Dm.depth_metrics(D, A, _cuda((2.5 * q).astype(f32))).items()}
    assert (h0["scale"] == 1).all() and np.allclose(h0["abs_rel"], 0.6, atol=1e-6) and (h0["d3"] == 0).all()
    # global: the pooled sum QZ / sum QQ of two images whose scales differ
    z2 = np.stack([2.0 * q[0], 3.0 * q[2]]).astype(f32)
    D2, A2 = _cuda(c["D"][[0, 2]]), _cuda(c["A"][[0, 2]])
    sums = R.forward(c["D"][[0, 2]], c["A"][[0, 2]], z2)[0]
    pooled = sums[:, R.IDX["QZ"]].sum() / sums[:, R.IDX["QQ"]].sum()
    g = Dm.depth_metrics(D2, A2, _cuda(z2), align="global")
    per = Dm.depth_metrics(D2, A2, _cuda(z2), align="scale")
    gs, ps = g["scale"].cpu().numpy(), per["scale"].cpu().numpy()
    assert gs[0] == gs[1] and abs(gs[0] - pooled) <= 1e-6 and 2.0 < pooled < 3.0
    assert np.abs(ps - [2.0, 3.0]).max() <= 1e-6
    assert (g["abs_rel"].cpu().numpy() > 0.05).all()
    # against ref64 with that scale
    ref = R.forward(c["D"][[0, 2]], c["A"][[0, 2]], z2, None, np.full(2, gs[0], f32))[0]
    np.testing.assert_allclose(g["abs_rel"].cpu().numpy(), ref[:, R.IDX["ABSREL"]] / ref[:, R.IDX["W"]],
                               rtol=1e-12)
    # an image with nothing valid: NaN means, valid 0, no exception
    e = Dm.depth_metrics(D, A, _cuda(c["z"]), align="scale")
    eh = {k: v.cpu().numpy() for k, v in e.items()}
    assert np.isnan(eh["abs_rel"][1]) and np.isnan(eh["rmse"][1]) and eh["valid"][1] == 0
    assert eh["scale"][1] == 1 and np.isfinite(eh["abs_rel"][[0, 2]]).all()


@pytest.mark.gpu
def test_hip_bad_arguments_raise_before_any_launch():
    from splatt3r_amd import _lib
    from splatt3r_amd import depth as Dm
    lib = _lib.lib()
    t, am = _dev_case("batch_one_invalid")
    D, A, z = t["D"], t["A"], t["z"]
    with pytest.raises(RuntimeError, match="GPU only"):
        Dm.depth_sums(D.cpu(), A.cpu(), z.cpu())
    with pytest.raises(RuntimeError, match="one device"):
        Dm.depth_sums(D, A.cpu(), z)
    with pytest.raises(ValueError, match="alpha_min"):
        Dm.depth_loss(D, A, z, alpha_min=float("inf"))
    with pytest.raises(TypeError):
        Dm.depth_metrics(D, A, z.half())
    # through the ABI: status 1 and a message, nothing launched, nothing written
    B, H, W = D.shape
    sums = torch.full((B, 14), 7.0, device="cuda", dtype=torch.float64)
    rmap = torch.full_like(D, 7.0)
    ws = torch.empty(lib.s3z_workspace_bytes(B, H, W), device="cuda", dtype=torch.uint8)

    def call(am=0.5, B_=B, rm=rmap.data_ptr(), tgt=z.data_ptr()):
        return lib.s3z_forward(D.data_ptr(), A.data_ptr(), tgt, None, None, B_, H, W, am, rm,
                               sums.data_ptr(), ws.data_ptr(), _lib.stream(D.device))
    for kw, msg in ((dict(am=-1.0), b"alpha_min"), (dict(B_=0), b"B = 0"),
                    (dict(rm=D.data_ptr()), b"rmap overlaps"), (dict(tgt=None), b"must not be NULL")):
        assert call(**kw) == 1 and msg in lib.s3_last_error(), kw
    torch.cuda.synchronize()
    assert (sums == 7).all() and (rmap == 7).all()
    # and the library still works
    assert call() == 0
    torch.cuda.synchronize()
    assert not (sums == 7).any()
