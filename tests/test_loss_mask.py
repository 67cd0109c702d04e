"""Co-visibility loss mask (include/s3c.h, splatt3r_amd/loss_mask.py) against
the reference's utils/loss_mask.py, whose inputs and outputs are committed in
tests/golden/loss_mask.npz (tools/gen_loss_mask_golden.py).

A boolean decision cannot be compared to a tolerance: a pixel whose projection
lies within float32 rounding of the frustum's edge, or whose depth difference
lies within rounding of the isclose edge, may legitimately fall either way.
Such pixels form the ambiguity band, found from the float64 restatement's
margins (tests/loss_mask_ref64.py):

    ambiguous  <=>  for some context view  m_fr < eps_px  or  |m_md| < eps_d

The widths are not chosen: the fixture stores the largest difference between
the reference's own float32 u, v and m_md and the float64 restatement's over
all cases (the floor), and eps = 4 x floor rounded up to one significant digit
(the rule of test_raster_grad.py).  Measured floors: 2.2e-4 px and 1.6e-5
depth units, hence eps_px = 9e-4 and eps_d = 7e-5.  Outside the band every
pixel must agree exactly; the band itself may hold at most 1 % of the pixels
of any case.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from loss_mask_ref64 import COND_DEPTH, COND_FRUSTUM, COND_MATCH, ambiguous, loss_mask_ref

import splatt3r_amd.loss_mask as LM

INPUTS = ("depth_1", "K_1", "c2w_1", "depth_2", "K_2", "c2w_2")
HAND_BUILT = ("a", "b", "c")
MAX_AMBIGUOUS_SHARE = 0.01


def round_up_1sig(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


_CACHE = {}


def fixture():
    """The committed cases: name -> dict of the inputs (CPU tensors), the
    reference's mask / fr / nz / md, its condition bits, the float64
    restatement and the ambiguous pixels.  Built once, never modified."""
    if not _CACHE:
        z = np.load(os.path.join(GOLDEN, "loss_mask.npz"))
        eps_px = round_up_1sig(4 * float(z["floor_px"]))
        eps_d = round_up_1sig(4 * float(z["floor_d"]))
        cases = {}
        for name in z["names"].tolist():
            c = {k: torch.from_numpy(z[f"{name}.{k}"]) for k in INPUTS + ("mask", "fr", "nz", "md")}
            c["args"] = tuple(c[k] for k in INPUTS)
            c["conditions"] = (c["fr"].to(torch.uint8) * COND_FRUSTUM
                               + c["nz"].to(torch.uint8) * COND_DEPTH
                               + c["md"].to(torch.uint8) * COND_MATCH)
            c["ref64"] = loss_mask_ref(*c["args"])
            c["ambiguous"] = ambiguous(c["ref64"], eps_px, eps_d)
            cases[name] = c
        _CACHE.update(cases=cases, eps_px=eps_px, eps_d=eps_d, floor_px=float(z["floor_px"]),
                      floor_d=float(z["floor_d"]), probe_a=tuple(z["probe_a"].tolist()),
                      probe_b=tuple(z["probe_b"].tolist()))
    return _CACHE


CASE_NAMES = ("r0", "r1", "r2") + HAND_BUILT


def _cuda(c):
    return [t.cuda() for t in c["args"]]


# ----------------------------------------------------------------- CPU ------
def test_fixture_holds_the_issue_cases():
    f = fixture()
    assert tuple(f["cases"]) == CASE_NAMES
    shapes = [tuple(f["cases"][n]["depth_1"].shape) + (f["cases"][n]["depth_2"].shape[1],)
              for n in ("r0", "r1", "r2")]
    assert shapes == [(2, 2, 24, 40, 2), (1, 1, 37, 53, 3), (1, 3, 16, 16, 1)]
    for n in ("r0", "r1", "r2"):
        c = f["cases"][n]
        # every condition rejects pixels on its own
        assert 0.05 < float((~c["fr"]).float().mean()) < 0.95
        assert 0.03 < float((~c["nz"]).float().mean()) < 0.10
        assert int((c["fr"] & c["nz"] & ~c["md"]).sum()) > 50
        assert torch.equal(c["fr"] & c["nz"] & c["md"], c["mask"])
    x, y = f["probe_a"]
    assert bool(f["cases"]["a"]["mask"][0, 0, y, x])
    x, y = f["probe_b"]
    assert bool(f["cases"]["b"]["mask"][0, 0, y, x])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_float64_restatement_equals_the_reference_outside_the_band(name):
    c = fixture()["cases"][name]
    clear = ~c["ambiguous"]
    for key in ("mask", "fr", "nz", "md"):
        assert torch.equal(c["ref64"][key][clear], c[key][clear]), key
    assert torch.equal(c["ref64"]["conditions"][clear], c["conditions"][clear])


def test_ambiguity_band_is_at_most_one_percent_of_every_case():
    f = fixture()
    assert f["eps_px"] == round_up_1sig(4 * f["floor_px"]) >= 4 * f["floor_px"]
    assert f["eps_d"] == round_up_1sig(4 * f["floor_d"]) >= 4 * f["floor_d"]
    assert 0 < f["floor_px"] < 1e-2 and 0 < f["floor_d"] < 1e-3
    for name, c in f["cases"].items():
        share = float(c["ambiguous"].float().mean())
        print(f"{name}: ambiguous {int(c['ambiguous'].sum())} of {c['ambiguous'].numel()} "
              f"({share:.4%}), eps_px {f['eps_px']:g}, eps_d {f['eps_d']:g}")
        assert share <= MAX_AMBIGUOUS_SHARE, name
        if name in HAND_BUILT:
            assert not bool(c["ambiguous"].any()), name


def test_reference_rerun_equals_the_committed_fixture():
    ref_dir = os.environ.get("S3_REFERENCE_DIR", "/root/reference")
    if not os.path.isdir(os.path.join(ref_dir, "splatt3r_core", "utils")):
        pytest.skip("no reference tree")
    pytest.importorskip("einops")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import gen_loss_mask_golden as gen
        out = gen.build_cases()
    finally:
        sys.path.remove(os.path.join(REPO, "tools"))
    z = np.load(os.path.join(GOLDEN, "loss_mask.npz"))
    assert sorted(out) == sorted(z.files)
    for k in z.files:
        assert out[k].dtype == z[k].dtype and np.array_equal(out[k], z[k]), k


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return "mask"


def test_calculate_loss_mask_slices_and_stacks_the_batch(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(LM, "calculate_in_frustum_mask", rec)
    g = torch.Generator().manual_seed(0)
    view = lambda: dict(depthmap=torch.rand(2, 6, 5, generator=g),
                        camera_intrinsics=torch.rand(2, 4, 4, generator=g),
                        camera_pose=torch.rand(2, 4, 4, generator=g))
    batch = dict(target=[view()], context=[view(), view(), view()])
    assert LM.calculate_loss_mask(batch, as_float=True) == "mask"
    (args, kwargs), = rec.calls
    assert kwargs == dict(as_float=True)
    assert [tuple(a.shape) for a in args] == [(2, 1, 6, 5), (2, 1, 3, 3), (2, 1, 4, 4),
                                              (2, 3, 6, 5), (2, 3, 3, 3), (2, 3, 4, 4)]
    for j, v in enumerate(batch["context"]):
        assert torch.equal(args[3][:, j], v["depthmap"])
        assert torch.equal(args[4][:, j], v["camera_intrinsics"][:, :3, :3])
        assert torch.equal(args[5][:, j], v["camera_pose"])
    assert torch.equal(args[1][:, 0], batch["target"][0]["camera_intrinsics"][:, :3, :3])


def test_argument_errors_name_the_function_and_the_argument():
    c = fixture()["cases"]["r2"]
    a = list(c["args"])
    fn = "calculate_in_frustum_mask"

    def bad(i, t, exc, *words):
        b = list(a)
        b[i] = t
        with pytest.raises(exc) as e:
            LM.calculate_in_frustum_mask(*b)
        for w in (fn,) + words:
            assert w in str(e.value), (w, str(e.value))

    bad(0, a[0].double(), TypeError, "depth_1", "float32")
    bad(4, a[4].half(), TypeError, "intrinsics_2")
    bad(0, a[0][0], ValueError, "depth_1")
    bad(3, a[3][..., :-1], ValueError, "depth_2")
    bad(1, a[1][..., :2, :], ValueError, "intrinsics_1")
    bad(2, a[2][:, :1], ValueError, "c2w_1")
    bad(4, torch.zeros(1, 1, 4, 4), ValueError, "intrinsics_2")
    bad(5, a[5][..., :3, :], ValueError, "c2w_2")
    bad(5, None, TypeError, "c2w_2")
    # CPU tensors: what every kernel wrapper of the package raises
    with pytest.raises(RuntimeError, match="GPU only"):
        LM.calculate_in_frustum_mask(*a)


# ----------------------------------------------------------------- GPU ------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_hip_mask_and_conditions_equal_the_reference(name, parity):
    c = fixture()["cases"][name]
    mask, cond = LM.calculate_in_frustum_mask(*_cuda(c), return_conditions=True)
    assert mask.dtype == torch.bool and cond.dtype == torch.uint8
    assert mask.shape == c["mask"].shape == cond.shape
    mask, cond = mask.cpu(), cond.cpu()
    assert torch.equal(mask, cond == (COND_FRUSTUM | COND_DEPTH | COND_MATCH))
    amb = c["ambiguous"]
    differ = (mask != c["mask"]) | (cond != c["conditions"])
    parity(f"loss_mask.{name}", ambiguous=int(amb.sum()), differing_ambiguous=int((differ & amb).sum()),
           differing_unambiguous=int((differ & ~amb).sum()), pixels=amb.numel())
    assert torch.equal(mask[~amb], c["mask"][~amb])
    for bit, key in ((COND_FRUSTUM, "fr"), (COND_DEPTH, "nz"), (COND_MATCH, "md")):
        assert torch.equal((cond & bit != 0)[~amb], c[key][~amb]), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", HAND_BUILT)
def test_hip_hand_built_cases_match_exactly(name):
    f = fixture()
    c = f["cases"][name]
    mask, cond = LM.calculate_in_frustum_mask(*_cuda(c), return_conditions=True)
    assert torch.equal(mask.cpu(), c["mask"]) and torch.equal(cond.cpu(), c["conditions"])
    if name == "a":      # separate `any`: in view A's frustum, matching only in view B
        x, y = f["probe_a"]
        assert bool(mask[0, 0, y, x])
    if name == "b":      # no z > 0 test: a point behind the context camera passes
        x, y = f["probe_b"]
        assert bool(mask[0, 0, y, x]) and float(c["ref64"]["z"][0, 0, 0, y, x]) < 0


@pytest.mark.gpu
def test_hip_as_float_is_the_mask_and_runs_are_bit_identical():
    c = fixture()["cases"]["r0"]
    a = _cuda(c)
    mask, cond = LM.calculate_in_frustum_mask(*a, return_conditions=True)
    mask_f, cond_f = LM.calculate_in_frustum_mask(*a, as_float=True, return_conditions=True)
    assert mask_f.dtype == torch.float32 and torch.equal(mask_f, mask.float())
    assert torch.equal(cond, cond_f)
    assert torch.equal(LM.calculate_in_frustum_mask(*a), mask)
    # non-contiguous inputs are the same inputs
    wide = torch.zeros(*a[0].shape[:-1], a[0].shape[-1] + 3, device="cuda")
    wide[..., :-3] = a[0]
    assert torch.equal(LM.calculate_in_frustum_mask(wide[..., :-3], *a[1:]), mask)


@pytest.mark.gpu
def test_hip_batch_equals_the_per_image_calls():
    c = fixture()["cases"]["r0"]
    a = _cuda(c)
    mask, cond = LM.calculate_in_frustum_mask(*a, return_conditions=True)
    b, v1 = mask.shape[:2]
    for bb in range(b):
        for i in range(v1):
            one = [a[0][bb:bb + 1, i:i + 1], a[1][bb:bb + 1, i:i + 1], a[2][bb:bb + 1, i:i + 1],
                   a[3][bb:bb + 1], a[4][bb:bb + 1], a[5][bb:bb + 1]]
            m1, c1 = LM.calculate_in_frustum_mask(*one, return_conditions=True)
            assert torch.equal(m1[0, 0], mask[bb, i]) and torch.equal(c1[0, 0], cond[bb, i])


@pytest.mark.gpu
@pytest.mark.parametrize("value", (0.0, 1e30))
def test_hip_degenerate_depth_gives_an_all_false_mask(value):
    """depth_1 = 0: every pixel of a view unprojects to the camera centre and
    the depth condition is false.  depth_1 = 1e30: the chain runs at the edge
    of the float32 range; no context depth is within 0.1 of such a z.  The
    taps are bound-checked in floating point before they become indices
    (csrc/loss_mask.hip tap()); this test sees the result only."""
    c = fixture()["cases"]["r1"]
    a = _cuda(c)
    a[0] = torch.full_like(a[0], value)
    mask, cond = LM.calculate_in_frustum_mask(*a, return_conditions=True)
    assert not bool(mask.any())
    want_depth_bit = COND_DEPTH if value > 1e-6 else 0
    assert bool(((cond & COND_DEPTH) == want_depth_bit).all())
    if value > 1:
        assert not bool((cond & COND_MATCH).any())
    # the same with a pose that sends every point to NaN
    a[2] = torch.full_like(a[2], float("nan"))
    mask, cond = LM.calculate_in_frustum_mask(*a, return_conditions=True)
    assert not bool(mask.any()) and not bool((cond & (COND_FRUSTUM | COND_MATCH)).any())


@pytest.mark.gpu
def test_hip_image_metrics_over_the_kernel_mask_equal_the_reference_mask():
    import splatt3r_amd.photometric as PH
    c = fixture()["cases"]["r0"]
    mask_f = LM.calculate_in_frustum_mask(*_cuda(c), as_float=True)
    assert torch.equal(mask_f.cpu(), c["mask"].float()), "pick a case with no differing pixel"
    b, v1, h, w = mask_f.shape
    g = torch.Generator().manual_seed(11)
    pred = torch.rand(b * v1, 3, h, w, generator=g).cuda()
    target = torch.rand(b * v1, 3, h, w, generator=g).cuda()
    got = PH.image_metrics(pred, target, mask_f.flatten(0, 1))
    want = PH.image_metrics(pred, target, c["mask"].float().flatten(0, 1).cuda())
    for k in want:
        assert torch.equal(got[k], want[k]), k
        assert bool(torch.isfinite(got[k]).all()), k


def _synthetic_view(h, w, g):
    """Gaussian head outputs of one view, in front of the camera (as
    tests/test_photometric.py makes them)."""
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
def test_hip_eval_novel_view_renders():
    """Keyframes as test_photometric.test_hip_eval_keyframe_renders builds
    them (synthetic head outputs, no network), at three slightly different
    poses.  The rows are image_metrics of the same renders over the mask
    calculate_in_frustum_mask gives on the same rendered depths."""
    import types
    import lietorch
    import splatt3r_amd.evaluate as EV
    import splatt3r_amd.photometric as PH
    from splatt3r_amd.frame import create_frame
    from splatt3r_amd.splatt3r_utils import (_estimate_default_intrinsics, _sim3_to_4x4,
                                             splatt3r_render)
    from splatt3r_amd.synthetic import tum_like_sequence
    dev = torch.device("cuda", 0)
    h, w = 48, 64
    model = types.SimpleNamespace(decoder=types.SimpleNamespace(
        background_color=torch.tensor([0.1, 0.2, 0.3], device=dev)))
    frames = tum_like_sequence(3, h, w, seed=3, step_px=2.0, device=dev)
    kfs = [create_frame(i, frames[i], device=dev) for i in range(3)]
    g = torch.Generator(device="cuda").manual_seed(5)
    for i, kf in enumerate(kfs):
        kf.gaussian_pred, kf.gaussian_pred_cross = _synthetic_view(h, w, g), _synthetic_view(h, w, g)
        kf.T_WC = lietorch.Sim3(torch.tensor([[0.03 * i, -0.02 * i, 0.01 * i, 0, 0, 0, 1, 1 + 0.1 * i]],
                                             device=dev))
    res = EV.eval_novel_view_renders(model, kfs)
    assert res["skipped"] == 0 and res["empty"] == 0
    assert [(r["frame_id"], r["source_id"]) for r in res["rows"]] == [(1, 0), (2, 1)]

    K = _estimate_default_intrinsics(h, w, dev).reshape(1, 1, 3, 3)

    def depth_of(kf):
        _, d, a = splatt3r_render(model, kf, kf, return_depth=True)
        return torch.where(a >= 0.5, d / a, torch.zeros_like(d)).contiguous()

    for row, (i, j) in zip(res["rows"], ((1, 0), (2, 1))):
        render = splatt3r_render(model, kfs[j], kfs[j], target_T_WC=kfs[i].T_WC)[0].contiguous()
        mask = LM.calculate_in_frustum_mask(
            depth_of(kfs[i]), K, _sim3_to_4x4(kfs[i].T_WC).reshape(1, 1, 4, 4),
            depth_of(kfs[j]), K, _sim3_to_4x4(kfs[j].T_WC).reshape(1, 1, 4, 4), as_float=True)[0]
        want = PH.image_metrics(render, (kfs[i].img * 0.5 + 0.5).contiguous(), mask)
        for k in ("mse", "psnr", "ssim", "l1"):
            assert row[k] == float(want[k][0]), k
            assert np.isfinite(row[k])
        assert row["mask_fraction"] == float(mask.mean())
        assert 0.0 < row["mask_fraction"] < 1.0
    assert res["means"]["mse"] == float(np.mean([r["mse"] for r in res["rows"]]))

    res2 = EV.eval_novel_view_renders(model, kfs, gap=2)
    assert [(r["frame_id"], r["source_id"]) for r in res2["rows"]] == [(2, 0)]
    # a keyframe without predictions is skipped and counted
    kfs[0].gaussian_pred = kfs[0].gaussian_pred_cross = None
    res3 = EV.eval_novel_view_renders(model, kfs)
    assert res3["skipped"] == 1 and [r["frame_id"] for r in res3["rows"]] == [2]
    assert {k: res3["rows"][0][k] for k in want} == {k: res["rows"][1][k] for k in want}
