"""Photometric loss and render-quality metrics (include/s3p.h,
splatt3r_amd/photometric.py) against a float64 autograd reference.

tests/photometric_ref64.py restates the definition in float64 PyTorch
(explicit reflect indexing, separable conv2d) and lets autograd differentiate
it; it shares no code with csrc/photometric.hip.  The CPU tests pin that
reference to scipy's gaussian_filter and check the host side; the GPU tests
hold the HIP kernels to the reference.

Cases (B, C, H, W): (1, 3, 11, 11) every pixel reflects on both sides;
(2, 3, 13, 29) odd sizes, B > 1; (1, 1, 75, 141) more than two 32 x 16 tiles
per axis with ragged last tiles; (1, 3, 384, 512) the product size (forward
only).  Inputs uniform in [0, 1]; `range` has values in [-0.5, 1.5] (nothing
is clamped); the `mask` cases have a rectangular hole and a fully masked-out
block of rows.

Metric: images (the S map) max|a - b|; scalars (the five sums, mse, l1, psnr,
both ssim normalisations) |a - b| / |ref|; gradients max|a - b| / max|ref|.

Floors and tolerances (the rule of tests/test_raster_grad.py).  floor = the
reference run in float32 against itself in float64, measured WITHOUT the
kernel, worst case over the cases (test_float32_floor prints them);
tol = 4 x floor rounded up to one significant digit.  uxx - ux^2 cancels in
float32 against C2 = 9e-4, which is why the S floor sits far above 1e-7.

  quantity    floor     worst case    tol
  S           2.6e-6    product       2e-05
  scalars     1.2e-7    odd_mask      5e-07    sums of (x-y)^2, |x-y|, m; mse, l1, psnr
  ssim        1.0e-5    odd           4e-05    sums of m S and of S over the crop; ssim
  grad_map    1.2e-6    odd_mask      5e-06    d sum(w S) / dpred, w random normal
  grad_loss   7.9e-7    border        4e-06    d photometric_loss / dpred
(floors rounded up to two digits.  The images are uniform noise, whose SSIM is
near zero: the sums of S cancel, hence the higher relative floor of `ssim`.)
"""
import functools

import numpy as np
import pytest
import torch

import photometric_ref64 as R64
from splatt3r_amd import photometric as PH
from splatt3r_amd import evaluate as EV

#            floor (measured)   tol = roundup_1sig(4 x floor)
FLOOR = {
    "S":         2.6e-6,
    "scalars":   1.2e-7,
    "ssim":      1.0e-5,
    "grad_map":  1.2e-6,
    "grad_loss": 7.9e-7,
}


def _roundup_1sig(x):
    e = np.floor(np.log10(x))
    return float(np.ceil(x / 10 ** e - 1e-9) * 10 ** e)


TOL = {k: _roundup_1sig(4.0 * v) for k, v in FLOOR.items()}

#         name        shape             mask   value range   backward
CASES = {
    "border":   ((1, 3, 11, 11),   False, (0.0, 1.0), True),
    "odd":      ((2, 3, 13, 29),   False, (0.0, 1.0), True),
    "odd_mask": ((2, 3, 13, 29),   True,  (0.0, 1.0), True),
    "range":    ((2, 3, 13, 29),   False, (-0.5, 1.5), True),
    "tiles":    ((1, 1, 75, 141),  False, (0.0, 1.0), True),
    "tiles_mask": ((1, 1, 75, 141), True, (0.0, 1.0), True),
    "product":  ((1, 3, 384, 512), False, (0.0, 1.0), False),
}
BWD = [n for n, c in CASES.items() if c[3]]
LOSS_W = dict(mse_weight=1.0, l1_weight=0.3, ssim_weight=0.5)
# scalar quantities: the error terms, and those made of S (random images have
# an SSIM near zero, sums of S cancel, so their relative floor is higher)
SCALARS = ("sum_sq", "sum_abs", "sum_m", "mse", "l1", "psnr")
SSIMS = ("sum_ms", "sum_crop", "ssim")
SUM_NAMES = ("sum_sq", "sum_abs", "sum_ms", "sum_m", "sum_crop")


def make_mask(B, H, W):
    """A rectangular hole and a fully masked-out block of rows (shifted per
    batch image); mask.sum() > 0."""
    m = torch.ones(B, H, W, dtype=torch.float32)
    for b in range(B):
        m[b, H // 4 + b:H // 2 + b, W // 5:(3 * W) // 5] = 0.0
        m[b, (4 * H) // 5 - b:H - b, :] = 0.0
    assert m.sum() > 0 and (m.sum((1, 2)) > 0).all()
    return m


def _grads(pred, target, mask, w, dtype, adjoint="Gt"):
    """Reference gradients by autograd: of sum(w S) and of the weighted loss."""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    x, y = p, target.to(dtype)
    if mask is not None:
        x, y = x * mask.to(dtype)[:, None], y * mask.to(dtype)[:, None]
    (R64.ssim_map(x, y, adjoint=adjoint) * w.to(dtype)).sum().backward()
    g_map = p.grad.detach().double()
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    R64.loss(p, target, mask, dtype=dtype, adjoint=adjoint, **LOSS_W).backward()
    return g_map, p.grad.detach().double()


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and the float64 reference of one case (computed once, shared by
    every test; treat as read-only)."""
    shape, masked, (lo, hi), bwd = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    pred = lo + (hi - lo) * torch.rand(shape, generator=g)
    target = lo + (hi - lo) * torch.rand(shape, generator=g)
    w = torch.randn(shape, generator=g)
    mask = make_mask(shape[0], shape[2], shape[3]) if masked else None
    with torch.no_grad():
        ref = {k: v.double() for k, v in R64.forward(pred, target, mask).items()}
    out = dict(name=name, pred=pred, target=target, mask=mask, w=w, ref=ref)
    if bwd:
        out["g_map"], out["g_loss"] = _grads(pred, target, mask, w, torch.float64)
    return out


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a.reshape(b.shape) - b).max() / (np.abs(b).max() + 1e-300))


def scalar_err(got, ref, names=SCALARS):
    """Worst |a - b| / |ref| over the quantities `names` present in `got`."""
    worst = 0.0
    for k in names:
        if k in got:
            a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
            worst = max(worst, float((np.abs(a - b) / np.abs(b)).max()))
    return worst


# --------------------------------------------------------------- CPU tests
def test_reference_filter_is_scipy_gaussian_filter():
    ndi = pytest.importorskip("scipy.ndimage")
    z = torch.rand(1, 1, 13, 29, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = ndi.gaussian_filter(z[0, 0].numpy(), sigma=1.5, truncate=3.5, mode="reflect")
    d = float(np.abs(R64.gaussian_filter(z)[0, 0].numpy() - want).max())
    print(f"reference filter vs scipy: {d:.3e}")
    assert d <= 1e-14


def test_reference_crop_mean_is_the_mean_of_the_full_map():
    for name in ("border", "odd", "tiles"):
        c = case(name)
        S = c["ref"]["S"]
        H, W = S.shape[-2:]
        crop = S[..., 5:H - 5, 5:W - 5]
        assert crop.shape[-2:] == (H - 10, W - 10)
        np.testing.assert_allclose(c["ref"]["ssim"].numpy(), crop.mean((1, 2, 3)).numpy(),
                                   rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", list(CASES))
def test_float32_floor(name, parity):
    """The rounding floor: the reference in float32 against itself in
    float64 (no kernel involved)."""
    c = case(name)
    with torch.no_grad():
        r32 = R64.forward(c["pred"], c["target"], c["mask"], dtype=torch.float32)
    errs = {"S": float((r32["S"].double() - c["ref"]["S"]).abs().max()),
            "scalars": scalar_err(r32, c["ref"]), "ssim": scalar_err(r32, c["ref"], SSIMS)}
    if "g_map" in c:
        gm, gl = _grads(c["pred"], c["target"], c["mask"], c["w"], torch.float32)
        errs["grad_map"] = rel_err(gm, c["g_map"])
        errs["grad_loss"] = rel_err(gl, c["g_loss"])
    for k, e in errs.items():
        print(f"floor32 {name} {k} {e:.3e}")
        parity(f"photo_ref32_{name}_{k}", err=e, tol=TOL[k])
        assert e <= TOL[k], (name, k, e)


def test_border_case_is_sensitive_to_the_adjoint_fold():
    """At 11 x 11 every pixel reflects: a backward without the border fold
    (the zero-extended correlation alone, the reference with the fold
    removed) misses the tolerance by more than 50 x."""
    c = case("border")
    gm, gl = _grads(c["pred"], c["target"], None, c["w"], torch.float64, adjoint="nofold")
    e = rel_err(gm, c["g_map"])
    print(f"sensitivity border grad_map: {e:.3e} = {e / TOL['grad_map']:.0f} x tol")
    assert e >= 50.0 * TOL["grad_map"]
    # the unmasked loss weights S inside the crop only, 5 pixels from every
    # border: nothing of it reaches a reflected position, the fold is idle
    assert rel_err(gl, c["g_loss"]) <= 1e-12


def test_argument_validation_needs_no_gpu():
    f = lambda *s: torch.zeros(*s)
    with pytest.raises(TypeError, match="float32"):
        PH.ssim(f(1, 3, 16, 16).double(), f(1, 3, 16, 16).double())
    with pytest.raises(TypeError, match="float32"):
        PH.image_metrics(f(1, 3, 16, 16), f(1, 3, 16, 16), f(1, 16, 16).bool())
    with pytest.raises(ValueError, match="1 or 3"):
        PH.image_metrics(f(1, 2, 16, 16), f(1, 2, 16, 16))
    with pytest.raises(ValueError, match="win_size"):
        PH.ssim(f(1, 3, 10, 16), f(1, 3, 10, 16))
    with pytest.raises(ValueError, match="win_size"):
        PH.ssim_map(f(1, 3, 16, 10), f(1, 3, 16, 10))
    with pytest.raises(ValueError, match="differ in shape"):
        PH.photometric_loss(f(1, 3, 16, 16), f(1, 3, 16, 17))
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        PH.compute_ssim(f(3, 16, 16), f(3, 16, 16))
    with pytest.raises(ValueError, match="mask must be"):
        PH.photometric_loss(f(2, 3, 16, 16), f(2, 3, 16, 16), f(2, 3, 16, 16))
    with pytest.raises(ValueError, match="need a mask"):
        PH.calculate_loss(f(1, 3, 16, 16), f(1, 3, 16, 16), None)
    # valid arguments on the host: the kernels run on the GPU only
    with pytest.raises(RuntimeError, match="GPU only"):
        PH.image_metrics(f(1, 3, 16, 16), f(1, 3, 16, 16))


def test_save_render_metrics_round_trips(tmp_path):
    rows = [dict(mse=0.125, psnr=9.030899869919434, ssim=0.5, l1=0.3),
            dict(mse=1e-7, psnr=70.0, ssim=0.9999998807907104, l1=1e-4),
            dict(mse=0.0, psnr=float("inf"), ssim=1.0, l1=0.0)]
    ts = [1305031453.359684, 1305031453.391690, 7]
    EV.save_render_metrics(tmp_path / "logs", "render_metrics.txt", ts, rows)
    lines = (tmp_path / "logs" / "render_metrics.txt").read_text().splitlines()
    assert len(lines) == 4 and lines[-1].startswith("# mean ")
    assert lines[0] == "1305031453.359684 0.125 9.030899869919434 0.5"
    got_ts, got_rows, means = EV.load_render_metrics(tmp_path / "logs" / "render_metrics.txt")
    assert got_ts == [str(t) for t in ts]
    for a, b in zip(got_rows, rows):
        assert a == {k: b[k] for k in EV.METRIC_NAMES}
    assert means["mse"] == float(np.mean([r["mse"] for r in rows]))
    assert means["psnr"] == float("inf") and means["ssim"] == float(np.mean([r["ssim"] for r in rows]))


# --------------------------------------------------------------- GPU tests
def _cuda(t):
    return None if t is None else t.cuda()


@functools.lru_cache(maxsize=None)
def gpu_run(name):
    """Every forward output (and, for the backward cases, both gradients) of
    one case from the HIP kernels."""
    c = case(name)
    pred, target, mask = _cuda(c["pred"]), _cuda(c["target"]), _cuda(c["mask"])
    sums, S, _ = PH._run_forward(pred, target, mask, True, True, False)
    out = dict(S=S.cpu().double())
    out.update({k: sums[:, i].cpu() for i, k in enumerate(SUM_NAMES)})
    out.update({k: v.cpu().double() for k, v in PH.image_metrics(pred, target, mask).items()})
    out["ssim_fn"] = PH.ssim(pred, target, mask).cpu().double()
    out["S_full"] = PH.ssim(pred, target, mask, full=True).cpu().double()
    if c["mask"] is None:
        out["compute_ssim_map"] = PH.compute_ssim(target, pred, full=True).cpu().double()
        out["compute_ssim_mean"] = PH.compute_ssim(target, pred, full=False).cpu().double()
    if "g_map" in c:
        p = pred.clone().requires_grad_(True)
        (PH.ssim_map(p, target, mask) * c["w"].cuda()).sum().backward()
        out["g_map"] = p.grad.cpu()
        p = pred.clone().requires_grad_(True)
        PH.photometric_loss(p, target, mask, **LOSS_W).backward()
        out["g_loss"] = p.grad.cpu()
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_forward_vs_float64_reference(name, parity):
    got, ref = gpu_run(name), case(name)["ref"]
    d = float((got["S"] - ref["S"]).abs().max())
    e = scalar_err(got, ref)
    e2 = max(scalar_err(got, ref, SSIMS), scalar_err(dict(ssim=got["ssim_fn"]), ref, SSIMS))
    print(f"hip {name} S {d:.3e} scalars {e:.3e} ssim {e2:.3e}")
    parity(f"photo_hip_{name}_S", max_abs=d, tol=TOL["S"])
    parity(f"photo_hip_{name}_scalars", max_rel=e, tol=TOL["scalars"])
    parity(f"photo_hip_{name}_ssim", max_rel=e2, tol=TOL["ssim"])
    assert all(k in got for k in SCALARS + SSIMS)
    assert d <= TOL["S"], (name, d)
    assert e <= TOL["scalars"] and e2 <= TOL["ssim"], (name, e, e2)
    assert torch.equal(got["S_full"], got["S"])
    if "compute_ssim_map" in got:
        assert torch.equal(got["compute_ssim_map"], got["S"])
        assert torch.equal(got["compute_ssim_mean"], got["ssim_fn"])


@pytest.mark.gpu
def test_hip_masked_ssim_is_the_reference_normalisation():
    """sum over channels of m S, over mask.sum(): 3 x the per-channel mean."""
    got, c = gpu_run("odd_mask"), case("odd_mask")
    m = c["mask"].double()[:, None]
    want = (c["ref"]["S"] * m).sum((1, 2, 3)) / c["mask"].double().sum((1, 2))
    assert float(((got["ssim"] - want).abs() / want.abs()).max()) <= TOL["ssim"]
    want_mse = (((c["pred"] - c["target"]).double() ** 2) * m).sum((1, 2, 3)) / m.sum((1, 2, 3))
    assert float(((got["mse"] - want_mse).abs() / want_mse).max()) <= TOL["scalars"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", BWD)
def test_hip_backward_vs_float64_reference(name, parity):
    got, c = gpu_run(name), case(name)
    errs = {"grad_map": rel_err(got["g_map"], c["g_map"]),
            "grad_loss": rel_err(got["g_loss"], c["g_loss"])}
    for k, e in errs.items():
        print(f"hip {name} {k} {e:.3e}")
        parity(f"photo_hip_{name}_{k}", max_rel=e, tol=TOL[k])
    for k, e in errs.items():
        assert e <= TOL[k], (name, k, e)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["odd_mask", "tiles_mask"])
def test_hip_masked_out_pixels_get_exactly_zero_gradient(name):
    got, c = gpu_run(name), case(name)
    dead = (c["mask"] == 0)[:, None].expand_as(c["pred"])
    assert dead.sum() > 0
    for k in ("g_map", "g_loss"):
        assert torch.all(got[k][dead] == 0.0), k
        assert torch.any(got[k][~dead] != 0.0), k


@pytest.mark.gpu
def test_hip_identical_images():
    c = case("odd")
    p = c["pred"].cuda()
    m = PH.image_metrics(p, p.clone())
    assert torch.all(m["mse"] == 0.0) and torch.all(m["l1"] == 0.0)
    assert torch.all(torch.isinf(m["psnr"]) & (m["psnr"] > 0))
    S = PH.ssim(p, p.clone(), full=True)
    assert float((S - 1.0).abs().max()) <= TOL["S"]
    assert float((m["ssim"] - 1.0).abs().max()) <= TOL["S"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["odd_mask", "tiles", "product"])
def test_hip_two_runs_are_bit_identical(name):
    c = case(name)
    pred, target, mask = _cuda(c["pred"]), _cuda(c["target"]), _cuda(c["mask"])

    def run():
        sums, S, derivs = PH._run_forward(pred, target, mask, True, True, True)
        p = pred.clone().requires_grad_(True)
        (PH.ssim_map(p, target, mask) * c["w"].cuda()).sum().backward()
        g1 = p.grad
        p = pred.clone().requires_grad_(True)
        PH.photometric_loss(p, target, mask, **LOSS_W).backward()
        return sums, S, derivs, g1, p.grad

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_hip_three_channels_equal_three_single_channel_calls():
    c = case("odd_mask")
    pred, target, mask, w = (_cuda(c[k]) for k in ("pred", "target", "mask", "w"))

    def run(p, t, ww):
        p = p.detach().clone().requires_grad_(True)
        S = PH.ssim_map(p, t.contiguous(), mask)
        (S * ww).sum().backward()
        return S.detach(), p.grad

    S3, g3 = run(pred, target, w)
    for ch in range(3):
        S1, g1 = run(pred[:, ch:ch + 1], target[:, ch:ch + 1], w[:, ch:ch + 1])
        assert torch.equal(S1, S3[:, ch:ch + 1])
        assert torch.equal(g1, g3[:, ch:ch + 1])


def _render_small_scene(sc, grad):
    """small_scene of tests/test_raster.py through the differentiable
    rasterizer (as its _gpu_render); every input requires grad."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from splatt3r_amd.synthetic import identity_camera_settings
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(grad)
    rs, scale = identity_camera_settings(sc["K"], sc["H"], sc["W"], "cuda")
    kw = dict(means3D=to(sc["means"] * scale), opacities=to(sc["opacities"]),
              cov3D_precomp=to(sc["cov6"] * scale * scale), shs=to(sc["shs"]))
    kw["means2D"] = torch.zeros_like(kw["means3D"], requires_grad=grad)
    img, _ = GaussianRasterizer(rs)(**kw)
    return img, kw


@pytest.mark.gpu
def test_hip_loss_backward_through_the_rasterizer():
    """photometric_loss(render).backward() gives the Gaussians, bit for bit,
    the gradients of the rasterizer's backward fed with the dL/dpred that
    photometric_loss returns for the detached render.  The image is 16 x 32,
    two rasterizer tiles: the rasterizer's backward adds a Gaussian's per-tile
    gradients with float atomics, and two addends are the most whose order
    cannot change the sum."""
    from test_raster import small_scene
    sc = small_scene(300, 3, H=16, W=32, fx=40.0)
    target = torch.rand(1, 3, 16, 32, generator=torch.Generator().manual_seed(4)).cuda()
    img, kw = _render_small_scene(sc, True)
    PH.photometric_loss(img[None], target, **LOSS_W).backward()
    d = img.detach()[None].clone().requires_grad_(True)
    PH.photometric_loss(d, target, **LOSS_W).backward()
    assert float(d.grad.abs().max()) > 0
    img2, kw2 = _render_small_scene(sc, True)
    assert torch.equal(img2, img)
    (img2 * d.grad[0]).sum().backward()
    for k in kw:
        assert kw[k].grad is not None and torch.equal(kw[k].grad, kw2[k].grad), k
    assert float(kw["means3D"].grad.abs().max()) > 0


@pytest.mark.gpu
def test_hip_calculate_loss_is_the_batch_normalisation():
    c = case("odd_mask")
    pred, target, mask = _cuda(c["pred"]), _cuda(c["target"]), _cuda(c["mask"])
    ref = c["ref"]
    p = pred.clone().requires_grad_(True)
    loss, mse, ssim_val = PH.calculate_loss(target, p, mask, calculate_ssim=True,
                                            mse_loss_weight=0.7)
    want_mse = float(ref["sum_sq"].sum() / ref["sum_m"].sum())
    want_ssim = float(ref["sum_ms"].sum() / ref["sum_m"].sum())
    assert abs(float(mse) - want_mse) <= TOL["scalars"] * want_mse
    assert abs(float(ssim_val) - want_ssim) <= TOL["ssim"] * abs(want_ssim)
    assert abs(float(loss) - 0.7 * want_mse) <= TOL["scalars"] * want_mse
    loss.backward()
    m = c["mask"].double()[:, None]
    want_g = 0.7 * 2.0 * m * (c["pred"] - c["target"]).double() / ref["sum_m"].sum()
    assert rel_err(p.grad.cpu(), want_g) <= TOL["grad_loss"]
    # five-dimensional [B, V, ...] inputs, no mask average
    out = PH.calculate_loss(target[:, None], pred[:, None], mask[:, None], apply_mask=False,
                            average_over_mask=False)
    want = float(((c["pred"] - c["target"]).double() ** 2).mean())
    assert len(out) == 2 and abs(float(out[1]) - want) <= TOL["scalars"] * want


def _synthetic_view(h, w, g):
    """Gaussian head outputs of one view, in front of the camera (as
    tests/test_raster_depth.py makes them)."""
    u = lambda *sh: torch.rand(*sh, generator=g, device="cuda")
    z = 1.0 + 2.0 * u(1, h, w, 1)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"),
                            indexing="ij")
    x = ((xs + 0.5) / w - 0.5)[None, ..., None] * z * 1.2
    y = ((ys + 0.5) / h - 0.5)[None, ..., None] * z * 0.9
    q = torch.nn.functional.normalize(torch.randn(1, h, w, 4, generator=g, device="cuda"), dim=-1)
    return dict(means=torch.cat([x, y, z], -1), scales=0.01 + 0.04 * u(1, h, w, 3), rotations=q,
                sh=u(1, h, w, 3, 1) - 0.5, opacities=0.1 + 0.8 * u(1, h, w, 1))


@pytest.mark.gpu
def test_hip_eval_keyframe_renders():
    """Keyframes built as tests/test_slam.py builds frames (tum_like_sequence
    through create_frame); their Gaussian predictions are seeded synthetic
    head outputs, so no network runs.  The rows are image_metrics of the same
    renders; a keyframe without predictions is counted as skipped."""
    import types
    from splatt3r_amd.frame import create_frame
    from splatt3r_amd.splatt3r_utils import splatt3r_render
    from splatt3r_amd.synthetic import tum_like_sequence
    dev = torch.device("cuda", 0)
    h, w = 48, 64
    model = types.SimpleNamespace(decoder=types.SimpleNamespace(
        background_color=torch.tensor([0.1, 0.2, 0.3], device=dev)))
    frames = tum_like_sequence(3, h, w, seed=3, step_px=2.0, device=dev)
    kfs = [create_frame(i, frames[i], device=dev) for i in range(3)]
    g = torch.Generator(device="cuda").manual_seed(5)
    for kf in kfs[:2]:
        kf.gaussian_pred, kf.gaussian_pred_cross = _synthetic_view(h, w, g), _synthetic_view(h, w, g)
    res = EV.eval_keyframe_renders(model, kfs)
    assert res["skipped"] == 1 and [r["frame_id"] for r in res["rows"]] == [0, 1]
    renders = torch.cat([splatt3r_render(model, kf, kf)[0] for kf in kfs[:2]])
    targets = torch.cat([kf.img * 0.5 + 0.5 for kf in kfs[:2]])
    want = PH.image_metrics(renders.contiguous(), targets.contiguous())
    for k in ("mse", "psnr", "ssim", "l1"):
        np.testing.assert_array_equal([r[k] for r in res["rows"]], want[k].cpu().numpy())
        assert res["means"][k] == float(np.mean(want[k].cpu().tolist()))
    rows, means = EV.eval_renders(renders, targets)
    assert [{k: r[k] for k in means} for r in res["rows"]] == rows and means == res["means"]
    assert np.isfinite([r["mse"] for r in rows]).all() and rows[0] != rows[1]
    # a keyframe that carries uimg is scored against it
    kfs[0].uimg = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(6))
    res2 = EV.eval_keyframe_renders(model, kfs[:1])
    want2 = PH.image_metrics(renders[:1].contiguous(),
                             kfs[0].uimg.to(dev).permute(2, 0, 1)[None].contiguous())
    assert res2["rows"][0]["mse"] == float(want2["mse"][0]) != rows[0]["mse"]
