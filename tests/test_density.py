"""Adaptive density control of the map refinement: the arithmetic
(csrc/splat_density_math.hpp), the HIP kernels (csrc/splat_density.hip,
include/s3d.h s3d_accumulate / s3d_densify / s3d_reset_opacity) and the loop
(refine.DensityControl, refine_splats(density=), SharedGaussians.refine).

Reference: tests/splat_density_ref64.py -- numpy float64, Philox4x32-10 in
integer arithmetic; it takes nothing from the code under test.  1,000 rows in
the ranges of splat_opt_ref64.make_inputs, statistics chosen so that about a
fifth each are pruned, cloned and split (test_inputs_cover_the_cases holds
the reference to that, and to every prune cause on its own, a NaN and an Inf
row, a zero quaternion among the splits, denom == 0 rows with a non-zero
grad_accum, three rows exactly on avg == grad_threshold with denom 1, and at
most 1 % of rows within relative 1e-5 of a threshold; as seeded there are
none, so every row's decision is compared).

Exact: decisions, counts, n_out, origin, row order, kept and cloned rows and
their moments (bit for bit), zero moments of new rows, f_dc / logit / raw
quaternion of split children (the parent's bits).

Tolerances (the rule of test_splat_io.py / test_refine.py): the floor of a
quantity is the error of the same composition in float32 numpy on the CPU
against float64, the tolerance 4 x floor rounded up to one significant digit;
computed here on every run, printed, recorded through `parity`.  Metrics: a
child's means and log scales per row relative to the row's largest reference
entry of the group; grad_accum per entry, relative.  Measured:

  quantity         floor    tolerance  host build  MI355X (n = 1000)
  child.means      5.1e-7   3e-6       3.8e-7      3.8e-7  (n = 262,145: 1.2e-6)
  child.log_scale  5.6e-8   3e-7       5.6e-8      5.6e-8
  grad_accum       1.3e-7   6e-7       1.2e-7      1.3e-7  (three steps)
The host build and the kernels run the same source with the same rounding
(-ffp-contract=off) and agree.  The floors are those of the 1,000 rows; the
tiled 262,145 rows draw other normals (the row index is the counter).

Loop (test_hip_loop_with_density_control): test_refine's 2,048-Gaussian scene
plus 500 copies with logit -8, three 16 x 32 views, 20 steps, a pass every 5.
On the MI355X, grad_threshold 1e-2: the 500 pruned at the first pass, 11
clones and 5 splits over the four passes, 2,548 -> 2,064 rows, loss 1.293e-2
-> 8.68e-3 (without density control 2.77e-3: in this scene every Gaussian
covers a tenth of the image, and a clone or a split raises the loss by more
than five steps take off; see LOOP below and DESIGN.md 6l).  The children of
two passes that split were within 5.8e-8 (means) and 4.0e-8 (log scales).
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import splat_density_ref64 as D
from conftest import REPO

N = 1000
SIZES = (1, 255, 256, 257, 1000)
# k_density_scan takes 1,024 blocks of 256 rows a trip: the smallest n with two trips
N_TWO_TRIPS = 1024 * 256 + 1
P0 = D.PARAMS
bits = lambda x: np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


# ------------------------------------------------------------ shared data --
@functools.lru_cache(maxsize=None)
def inputs(n=N):
    base = D.make_inputs(N)
    if n <= N:
        return tuple(t[:n] for t in base[:3]) + (tuple(t[:n] for t in base[3]),)
    return D.tile_inputs(n, base)


def params(**kw):
    p = dict(P0)
    p.update(kw)
    return p


@functools.lru_cache(maxsize=None)
def ref(n=N, cap=None, pass_=P0["pass"], seed=P0["seed"]):
    rows, m, v, st = inputs(n)
    return D.densify(rows, m, v, st, params(**{"pass": pass_, "seed": seed}),
                     2 * n if cap is None else cap)


@functools.lru_cache(maxsize=None)
def budget_case():
    """(inputs, B, the ten growing rows): every row of the 1,000 that is not
    pruned, two that are, and statistics that leave the first ten growing
    rows growing, so that cap = B + 3 >= n binds."""
    rows, m, v, st = inputs()
    codes = ref()["codes"]
    sel = np.sort(np.concatenate([np.nonzero(codes != D.PRUNE)[0],
                                  np.nonzero(codes == D.PRUNE)[0][:2]]))
    st = tuple(np.array(t[sel]) for t in st)
    grow = np.nonzero(codes[sel] >= D.CLONE)[0]
    assert set(codes[sel][grow[:10]]) == {D.CLONE, D.SPLIT}
    st[1][grow[10:]] = 0
    return (rows[sel], m[sel], v[sel], st), len(sel) - 2, grow[:10]


ACC_STEPS = 3


@functools.lru_cache(maxsize=None)
def accum_inputs(n=N):
    """(d_means2D [steps, n, 3], radii [steps, n]) float32 / int32: magnitudes
    log-uniform over 1e-8..1e-1, a third of the rows culled per step, a NaN
    and an Inf in two visible rows."""
    rng = np.random.default_rng(5)
    d2 = np.exp(rng.uniform(np.log(1e-8), np.log(1e-1), (ACC_STEPS, n, 3)))
    d2 = (d2 * rng.choice([-1.0, 1.0], d2.shape)).astype(np.float32)
    radii = rng.integers(1, 200, (ACC_STEPS, n)).astype(np.int32)
    radii[rng.random(radii.shape) < 0.33] = 0
    radii[:, 3::50] = -4
    if n > 12:
        radii[:, 10:12] = 9
        d2[1, 10, 0] = np.nan
        d2[2, 11, 1] = -np.inf
    return d2, radii


def accum_ref(n, dtype=np.float64):
    d2, radii = accum_inputs(n)
    st = inputs(n)[3]
    for t in range(ACC_STEPS):
        st = D.accumulate(d2[t], radii[t], st, dtype)
    return st


@functools.lru_cache(maxsize=None)
def floors():
    """Errors of the float32 numpy composition against float64."""
    rows, m, v, st = inputs()
    r32 = D.densify(rows, m, v, st, P0, 2 * N, dtype=np.float32)
    fl = D.child_errors(r32["rows"], ref())
    fl["grad_accum"] = D.accum_error(accum_ref(N, np.float32)[0], accum_ref(N)[0])
    return fl


def tol(k):
    return D.tolerance(floors()[k])


def got_codes(origin, n):
    """The decision each input row got, read off origin (a denied row reads
    as kept)."""
    o = np.asarray(origin, np.int64)
    src = np.where(o >= 0, o, ~o)
    cnt = np.bincount(src, minlength=n)
    neg = np.bincount(src, weights=(o < 0).astype(np.float64), minlength=n)
    return np.where(cnt == 0, D.PRUNE, np.where(cnt == 1, D.KEEP,
                                                np.where(neg == 2, D.SPLIT, D.CLONE)))


def compare(got, want, src, label, parity):
    """One pass of the code under test against the float64 reference `want`
    of the inputs src = (rows, m, v)."""
    n = len(src[0])
    eff = np.where((want["codes"] >= D.CLONE) & ~want["granted"], D.KEEP, want["codes"])
    same = got_codes(got["origin"], n) == eff
    assert same[~want["near"]].all(), (label, np.nonzero(~same & ~want["near"])[0][:10])
    assert same.all(), (label, "a near-threshold row decided the other way")
    assert got["n_out"] == want["n_out"] and tuple(got["counts"]) == tuple(want["counts"]), \
        (label, got["n_out"], want["n_out"], got["counts"], want["counts"])
    assert np.array_equal(np.asarray(got["origin"], np.int64), want["origin"]), label
    c = want["child"]
    for k in ("rows", "m", "v"):                       # kept rows, clones: bit for bit
        assert np.array_equal(bits(got[k][~c]), bits(want[k][~c])), (label, k)
        assert got[k].shape == (want["n_out"], 14)
    assert not got["m"][c].any() and not got["v"][c].any(), label
    new = want["origin"] < 0
    assert not got["m"][new].any() and not got["v"][new].any(), label
    parent = np.asarray(src[0])[~want["origin"][c]]
    for cols in (slice(3, 7), slice(10, 14)):          # copied fields of children
        assert np.array_equal(bits(got["rows"][c][:, cols]), bits(parent[:, cols])), label
    bad = []
    for k, e in D.child_errors(got["rows"], want).items():
        parity(f"{label}.{k}", err=e, tol=tol(k), floor=floors()[k])
        print(f"{label}.{k}: err {e:.3e} floor {floors()[k]:.3e} tol {tol(k):.1e}")
        if not e <= tol(k):
            bad.append((k, e, tol(k)))
    assert not bad, (label, bad)


# ---------------------------------------------------- CPU: the reference --
def test_inputs_cover_the_cases():
    rows, m, v, st = inputs()
    r = ref()
    frac = lambda c: float((r["codes"] == c).mean())
    print("pruned, kept, cloned, split:", [frac(c) for c in range(4)], "near:", r["near"].sum())
    for c in (D.PRUNE, D.CLONE, D.SPLIT):
        assert 0.12 <= frac(c) <= 0.28, (c, frac(c))
    assert r["near"].mean() <= 0.01
    causes = D.prune_causes(rows, st, P0)
    for j in range(4):                                   # every cause on its own
        assert (causes[:, j] & (causes.sum(1) == 1)).any(), j
    assert r["codes"][D.NAN_ROW] == D.PRUNE and r["codes"][D.INF_ROW] == D.PRUNE
    assert r["codes"][D.ZERO_QUAT_ROW] == D.SPLIT and not rows[D.ZERO_QUAT_ROW, 10:14].any()
    orphan = (st[1] == 0) & (st[0] != 0) & (r["codes"] != D.PRUNE)
    assert orphan.sum() >= 10 and (r["codes"][orphan] == D.KEEP).all()
    on = list(D.ON_THRESHOLD_ROWS)
    assert (st[0][on] == np.float32(P0["grad_threshold"])).all() and (st[1][on] == 1).all()
    assert set(r["codes"][on]) == {D.CLONE, D.SPLIT} and not r["near"][on].any()
    assert r["n_out"] == N - r["counts"][0] + r["counts"][1] + r["counts"][2]
    assert r["counts"][3] == 0
    assert D.LOG_SPLIT == float(np.float32(0.4700036292457356))


def test_float32_floors_are_finite(parity):
    for k, v in floors().items():
        parity(f"floor.{k}", floor=v, tol=D.tolerance(v))
        print(f"floor {k}: {v:.3e} tol {D.tolerance(v):.1e}")
        assert np.isfinite(v) and v > 0, k


@pytest.mark.parametrize("ablate,key", [("R", "child.means"), ("s", "child.means"),
                                        ("k", "child.means"), ("log", "child.log_scale")])
def test_reference_is_sensitive_to(ablate, key):
    """A kernel that dropped this term would miss the tolerance by >= 50 x."""
    rows, m, v, st = inputs()
    e = D.child_errors(D.densify(rows, m, v, st, P0, 2 * N, ablate=(ablate,))["rows"], ref())
    print(f"sensitivity {ablate}: {e[key]:.3e} = {e[key] / tol(key):.0f} x tol")
    assert e[key] >= 50.0 * tol(key)


PHILOX_KAT = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
              ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
               "d16cfe09 94fdcceb 5001e420 24126ea1"))


def test_reference_philox_known_answers():
    for ctr, key, want in PHILOX_KAT:
        got = D.philox4x32_10(np.array(ctr), np.array(key))
        assert " ".join(f"{int(x):08x}" for x in got) == want


# ------------------------------------------- CPU: the arithmetic, host build
@functools.lru_cache(maxsize=None)
def _host_exe():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    import atexit
    import tempfile
    d = tempfile.mkdtemp(prefix="splat_density_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "splat_density_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(REPO, "splatt3r-slam_amd", "csrc"),
                    "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "native", "splat_density_host.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _exe():
    exe = _host_exe()
    if exe is None:
        pytest.skip("hipcc not available")
    return exe


def _host_densify(rows, m, v, st, p, cap):
    exe = _exe()
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    n = len(rows)
    with open(fin, "wb") as f:
        for a, dt in ((rows, np.float32), (m, np.float32), (v, np.float32), (st[0], np.float32),
                      (st[1], np.int32), (st[2], np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    subprocess.run([exe, "densify", fin, fout, str(n), str(cap)] +
                   [repr(float(p[k])) for k in ("grad_threshold", "split_scale", "min_opacity",
                                                "max_scale")] +
                   [str(p["max_screen_radius"]), str(p["seed"]), str(p["pass"])],
                   check=True, timeout=300)
    raw = open(fout, "rb").read()
    n_out = int(np.frombuffer(raw, np.int64, 1)[0])
    counts = np.frombuffer(raw, np.int32, 4, 8)
    origin = np.frombuffer(raw, np.int32, n_out, 24)
    body = np.frombuffer(raw, np.float32, 3 * n_out * 14, 24 + 4 * n_out).reshape(3, n_out, 14)
    return dict(rows=body[0], m=body[1], v=body[2], origin=origin, n_out=n_out,
                counts=tuple(int(c) for c in counts))


def test_host_philox_known_answers():
    exe = _exe()
    for ctr, key, want in PHILOX_KAT:
        r = subprocess.run([exe, "philox"] + [f"{x:x}" for x in ctr + key], check=True,
                           capture_output=True, text=True, timeout=60)
        assert r.stdout.strip() == want


def test_host_math_vs_float64(parity):
    rows, m, v, st = inputs()
    compare(_host_densify(rows, m, v, st, P0, 2 * N), ref(), (rows, m, v), "host", parity)
    # a binding budget: three extra rows only
    src, B, grow = budget_case()
    want = D.densify(*src, P0, B + 3)
    assert want["counts"] == (2, want["counts"][1], 3 - want["counts"][1], 7)
    compare(_host_densify(*src, P0, B + 3), want, src[:3], "host.budget", parity)


def test_host_accumulate_vs_float64(parity):
    exe = _exe()
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "acc_in.bin"), os.path.join(d, "acc_out.bin")
    d2, radii = accum_inputs(N)
    with open(fin, "wb") as f:
        for t in range(ACC_STEPS):
            f.write(d2[t].tobytes())
            f.write(radii[t].tobytes())
    subprocess.run([exe, "accumulate", fin, fout, str(N), str(ACC_STEPS)], check=True, timeout=60)
    raw = open(fout, "rb").read()
    ga = np.frombuffer(raw, np.float32, N)
    dn = np.frombuffer(raw, np.int32, N, 4 * N)
    mr = np.frombuffer(raw, np.int32, N, 8 * N)
    zero = (np.zeros(N, np.float32), np.zeros(N, np.int32), np.zeros(N, np.int32))
    want = zero
    for t in range(ACC_STEPS):
        want = D.accumulate(d2[t], radii[t], want)
    e = D.accum_error(ga, want[0])
    parity("host.grad_accum", err=e, tol=tol("grad_accum"), floor=floors()["grad_accum"])
    print(f"host.grad_accum: err {e:.3e} tol {tol('grad_accum'):.1e}")
    assert e <= tol("grad_accum")
    assert np.array_equal(dn, want[1]) and np.array_equal(mr, want[2])


# ------------------------------------------------------------ CPU: the ABI --
def _struct(**kw):
    from splatt3r_amd.refine import as_params
    return as_params(params(**kw))


def test_abi_rejects_bad_arguments_before_any_device_work():
    """Status 1 with a message; the pointers are never dereferenced (they are
    not device memory here)."""
    from splatt3r_amd import _lib
    from splatt3r_amd import refine  # noqa: F401  (registers the signatures)
    lib = _lib.lib()

    def densify(n=5, cap=8, rows=0x1000, m=0x2000, v=0x3000, ga=0x4000, dn=0x5000, mr=0x6000,
                hp=True, out=0x10000, om=0x20000, ov=0x30000, origin=0x40000, n_out=0x50000,
                counts=0x60000, ws=0x70000, ws_bytes=1 << 20):
        h = _struct()
        return lib.s3d_densify(rows, m, v, n, ga, dn, mr, ctypes.byref(h) if hp else None, cap,
                               out, om, ov, origin, n_out, counts, ws, ws_bytes, None)
    for kw, msg in ((dict(n=-1), b"n < 0"), (dict(n=5, cap=4), b"cap < n"),
                    (dict(n=1 << 31, cap=1 << 32), b"too large"), (dict(hp=False), b"null params"),
                    (dict(rows=None), b"null parameter"), (dict(v=None), b"null parameter"),
                    (dict(dn=None), b"null statistics"), (dict(out=None), b"null output"),
                    (dict(origin=None), b"null output"), (dict(n_out=None), b"null output"),
                    (dict(counts=None), b"null output"), (dict(ws=None), b"null workspace"),
                    (dict(rows=0x1004), b"8-byte"), (dict(out=0x1000 + 56), b"overlaps"),
                    (dict(om=0x10000 + 56), b"outputs overlap")):
        assert densify(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    assert densify(ws_bytes=8) == 3 and b"workspace" in lib.s3_last_error()
    h = _struct()
    assert lib.s3d_densify(None, None, None, 0, None, None, None, ctypes.byref(h), 0, None, None,
                           None, None, None, None, None, 0, None) == 0
    assert lib.s3_last_error() == b""
    assert lib.s3d_workspace_bytes(1000) >= 1000 + 2 * 5 * 4

    acc = lambda n=5, d2=16, radii=16, ga=16: lib.s3d_accumulate(d2, radii, n, ga, 16, 16, None)
    for kw, msg in ((dict(n=-1), b"n < 0"), (dict(d2=None), b"null"), (dict(ga=None), b"null")):
        assert acc(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    assert lib.s3d_accumulate(None, None, 0, None, None, None, None) == 0
    rst = lambda n=5, rows=16, cap=-4.6: lib.s3d_reset_opacity(rows, 16, 16, n, cap, None)
    for kw, msg in ((dict(n=-1), b"n < 0"), (dict(rows=None), b"null"),
                    (dict(cap=float("nan")), b"NaN")):
        assert rst(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    assert lib.s3d_reset_opacity(None, None, None, 0, -4.6, None) == 0
    assert lib.s3_last_error() == b""


def test_python_validation_needs_no_gpu():
    from splatt3r_amd import refine
    assert ctypes.sizeof(refine.S3dParams) == 40 and refine.S3dParams.seed.offset == 24
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    st = (z(4), z(4, dt=torch.int32), z(4, dt=torch.int32))
    with pytest.raises(TypeError):
        refine.densify_splats(z(4, 14, dt=torch.float64), z(4, 14), z(4, 14), st, P0, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        refine.densify_splats(z(4, 14), z(4, 14), z(4, 14), st, P0, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        refine.reset_opacity(z(4, 14), z(4, 14), z(4, 14))
    with pytest.raises(ValueError):
        refine.accumulate_stats(z(4, 2), z(4, dt=torch.int32), st)
    with pytest.raises(ValueError, match="unknown"):
        refine.as_params(dict(P0, bogus=1))
    with pytest.raises(ValueError):
        refine.as_params(dict(P0, seed=-1))
    for kw in (dict(interval=0), dict(start=-1), dict(start=5, stop=4), dict(grad_threshold=-1.0),
               dict(extent=0.0), dict(min_opacity=float("nan")), dict(max_screen_radius=-1),
               dict(capacity=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            refine.DensityControl(**kw)
    dc = refine.DensityControl(start=0, interval=5, stop=20, opacity_reset_interval=7)
    assert [t for t in range(1, 26) if dc.due(t)] == [5, 10, 15, 20]
    assert [t for t in range(1, 16) if dc.reset_due(t)] == [7, 14]
    T = torch.eye(4).repeat(3, 1, 1)
    with pytest.raises(ValueError, match="extent"):
        dc.begin(10, T, "cpu")                           # coincident cameras
    T[1, 0, 3], T[2, 0, 3] = 1.0, -1.0
    assert abs(refine.DensityControl.cameras_extent(T) - 1.1) < 1e-12
    dc.begin(10, T, "cpu")
    hp = dc.params(2)
    assert abs(hp.split_scale - 0.011) < 1e-8 and abs(hp.max_scale - 0.11) < 1e-7
    assert getattr(hp, "pass") == 2 and dc.origin.tolist() == list(range(10))
    with pytest.raises(ValueError, match="capacity"):
        refine.DensityControl(capacity=5).begin(10, T, "cpu")
    # origin composition: pass 1 keeps 0, clones 1, splits 2; pass 2 splits the copy of 1
    o1 = torch.tensor([0, 1, ~1, ~2, ~2], dtype=torch.int32)
    c1 = refine.compose_origin(torch.arange(3, dtype=torch.int32), o1)
    assert c1.tolist() == [0, 1, ~1, ~2, ~2]
    o2 = torch.tensor([0, 1, ~2, ~2, 4], dtype=torch.int32)
    assert refine.compose_origin(c1, o2).tolist() == [0, 1, ~1, ~1, ~2]


# --------------------------------------------------------------------- GPU --
def _cuda(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _gpu_densify(src, p, cap):
    """One s3d_densify call through refine.densify_splats, as numpy."""
    from splatt3r_amd.refine import densify_splats
    rows, m, v, st = src
    t = [_cuda(a, np.float32) for a in (rows, m, v)]
    stats = (_cuda(st[0], np.float32), _cuda(st[1], np.int32), _cuda(st[2], np.int32))
    keep = [x.clone() for x in t + list(stats)]
    r, mm, vv, origin, counts = densify_splats(*t, stats, p, cap)
    for a, b in zip(t + list(stats), keep):               # inputs are left as they were
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    return dict(rows=r.cpu().numpy(), m=mm.cpu().numpy(), v=vv.cpu().numpy(),
                origin=origin.cpu().numpy(), n_out=r.shape[0],
                counts=tuple(counts[k] for k in ("pruned", "cloned", "split", "denied")))


def _same(a, b):
    return (a["n_out"] == b["n_out"] and a["counts"] == b["counts"]
            and np.array_equal(a["origin"], b["origin"])
            and all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("rows", "m", "v")))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES + (N_TWO_TRIPS,))
def test_hip_densify_vs_float64(n, parity):
    src = inputs(n)
    compare(_gpu_densify(src, P0, 2 * n), ref(n), src[:3], f"hip.n{n}", parity)


@pytest.mark.gpu
def test_hip_densify_is_reproducible_and_rows_are_independent():
    src = inputs()
    a, b = _gpu_densify(src, P0, 2 * N), _gpu_densify(src, P0, 2 * N)
    assert _same(a, b)
    # rows [0, 257) alone give what they give inside the 1,000-row call
    head = _gpu_densify(inputs(257), P0, 2 * 257)
    k = head["n_out"]
    assert k == ref(257)["n_out"] and np.array_equal(head["origin"], a["origin"][:k])
    for f in ("rows", "m", "v"):
        assert np.array_equal(bits(head[f]), bits(a[f][:k])), f
    # another pass or seed changes the children and nothing else
    c = ref()["child"]
    for kw in ({"pass": P0["pass"] + 1}, {"seed": P0["seed"] ^ (1 << 40)}):
        o = _gpu_densify(src, params(**kw), 2 * N)
        assert o["n_out"] == a["n_out"] and o["counts"] == a["counts"]
        assert np.array_equal(o["origin"], a["origin"])
        for f in ("rows", "m", "v"):
            assert np.array_equal(bits(o[f][~c]), bits(a[f][~c])), (kw, f)
        assert np.array_equal(bits(o["rows"][c][:, 3:]), bits(a["rows"][c][:, 3:])), kw
        assert (o["rows"][c][:, :3] != a["rows"][c][:, :3]).any(1).all(), kw


@pytest.mark.gpu
def test_hip_densify_budget(parity):
    src, B, grow = budget_case()
    want = D.densify(*src, P0, B + 3)
    got = _gpu_densify(src, P0, B + 3)
    compare(got, want, src[:3], "hip.budget", parity)
    assert got["n_out"] == B + 3 and got["counts"][0] == 2 and got["counts"][3] == 7
    assert got["counts"][1] + got["counts"][2] == 3
    assert sorted(set(~got["origin"][got["origin"] < 0])) == sorted(grow[:3])
    # cap == n and no prunes: nothing grows
    keep = want["codes"] != D.PRUNE
    rows, m, v, st = src
    sub = (rows[keep], m[keep], v[keep], tuple(t[keep] for t in st))
    nk = int(keep.sum())
    got = _gpu_densify(sub, P0, nk)
    assert got["n_out"] == nk and got["counts"] == (0, 0, 0, 10)
    assert np.array_equal(got["origin"], np.arange(nk))
    for f, s_ in zip(("rows", "m", "v"), sub):
        assert np.array_equal(bits(got[f]), bits(s_)), f


@pytest.mark.gpu
def test_hip_densify_edges():
    src = inputs()
    got = _gpu_densify(src, params(min_opacity=2.0), 2 * N)        # all rows pruned
    assert got["n_out"] == 0 and got["counts"] == (N, 0, 0, 0) and got["rows"].shape == (0, 14)
    finite = np.isfinite(src[0]).all(1)
    sub = tuple(t[finite] for t in src[:3]) + (tuple(t[finite] for t in src[3]),)
    nf = int(finite.sum())
    off = params(min_opacity=0.0, max_scale=0.0, max_screen_radius=0, grad_threshold=1e30)
    got = _gpu_densify(sub, off, 2 * nf)                           # no row acted on
    assert got["n_out"] == nf and got["counts"] == (0, 0, 0, 0)
    assert np.array_equal(got["origin"], np.arange(nf))
    for f, s_ in zip(("rows", "m", "v"), sub):
        assert torch.equal(torch.from_numpy(got[f].copy()), torch.from_numpy(np.array(s_))), f
    from splatt3r_amd.refine import densify_splats, new_stats
    e = torch.zeros(0, 14, device="cuda")
    r, mm, vv, o, counts = densify_splats(e, e.clone(), e.clone(), new_stats(0, "cuda"), P0, 0)
    assert r.shape == (0, 14) and o.shape == (0,) and counts["pruned"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", (257, 1000))
def test_hip_accumulate(n, parity):
    from splatt3r_amd.refine import accumulate_stats
    d2, radii = accum_inputs(n)
    st0 = inputs(n)[3]
    stats = (_cuda(st0[0], np.float32), _cuda(st0[1], np.int32), _cuda(st0[2], np.int32))
    for t in range(ACC_STEPS):
        before = [x.clone() for x in stats]
        accumulate_stats(_cuda(d2[t]), _cuda(radii[t]), stats)
        frozen = _cuda((radii[t] <= 0) | ~np.isfinite(d2[t][:, :2]).all(1))
        assert bool(frozen.any()) and not bool(frozen.all())
        for a, b in zip(stats, before):
            assert torch.equal(a[frozen], b[frozen])
        assert bool((stats[1][~frozen] == before[1][~frozen] + 1).all())
    want = accum_ref(n)
    e = D.accum_error(stats[0].cpu().numpy(), want[0])
    parity(f"hip.n{n}.grad_accum", err=e, tol=tol("grad_accum"), floor=floors()["grad_accum"])
    print(f"hip.n{n}.grad_accum: err {e:.3e} tol {tol('grad_accum'):.1e}")
    assert e <= tol("grad_accum")
    assert np.array_equal(stats[1].cpu().numpy(), want[1])
    assert np.array_equal(stats[2].cpu().numpy(), want[2])


@pytest.mark.gpu
def test_hip_reset_opacity():
    import math
    from splatt3r_amd.refine import SplatAdam
    rows, m, v, _ = inputs()
    ok = np.isfinite(rows).all(1)
    p = _cuda(rows[ok], np.float32)
    opt = SplatAdam(p)
    opt.exp_avg, opt.exp_avg_sq = _cuda(m[ok], np.float32), _cuda(v[ok], np.float32)
    before = [t.clone() for t in (opt.rows14, opt.exp_avg, opt.exp_avg_sq)]
    opt.reset_opacity(0.01)
    cap = torch.tensor(math.log(0.01 / 0.99), dtype=torch.float64).float().cuda()
    assert torch.equal(opt.rows14[:, 6], torch.minimum(before[0][:, 6], cap))
    assert bool((before[0][:, 6] > cap).any()) and bool((before[0][:, 6] < cap).any())
    assert not bool(opt.exp_avg[:, 6].any()) and not bool(opt.exp_avg_sq[:, 6].any())
    rest = [c for c in range(14) if c != 6]
    for a, b in zip((opt.rows14, opt.exp_avg, opt.exp_avg_sq), before):
        assert torch.equal(a[:, rest], b[:, rest])
    want = D.reset_opacity(rows[ok], m[ok], v[ok], math.log(0.01 / 0.99))
    for a, b in zip((opt.rows14, opt.exp_avg, opt.exp_avg_sq), want):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b))


# ------------------------------------------------ GPU: the rendering loop --
# the scene's Gaussians are 0.005..0.04 wide (median 0.02) and, after five
# steps, their mean gradient norm has a median of 1.8e-4 and a 90 % quantile of
# 1.4e-3, a 99 % quantile of 5.8e-3 and a maximum of 2.1e-2.  Every Gaussian
# covers about a tenth of a 16 x 32 image, so each clone (twice the opacity
# where it sits) or split raises the loss by more than the five steps to the
# next pass take off.  Measured last losses, first 1.293e-2, without density
# control 2.77e-3: grad_threshold 1e-3 (a seventh of the rows grow per pass)
# 1.05e-1; 5e-3 (34 to 77 rows per pass) 5.04e-2; 1e-2 (4, 5, 6, 1 rows)
# 8.68e-3; 1.5e-2 (one row) 2.98e-3.  The loop test asks for a loss that still
# falls and runs at 1e-2, the map test, which does not, at 5e-3.
LOOP = dict(start=0, interval=5, stop=20, grad_threshold=1e-2, extent=1.0, percent_dense=0.02,
            max_world_scale=0.0, seed=9)
MAP = dict(LOOP, grad_threshold=5e-3)


def _loop_scene():
    """test_refine's scene, perturbed, plus 500 copies with logit -8."""
    from test_refine import H, W, _perturbed, _scene
    from splatt3r_amd.refine import render_splats
    true, T_WC, K = _scene()
    images = render_splats(true, T_WC, K, H, W)
    start = _perturbed(true)
    ghosts = start[:500].clone()
    ghosts[:, 6] = -8.0
    return torch.cat([start, ghosts]).contiguous(), images, T_WC, K


def _loop_run():
    from splatt3r_amd.refine import DensityControl, refine_splats
    start, images, T_WC, K = _loop_scene()
    passes = []

    def on_pass(k, inp, out):
        host = lambda t: t.cpu().numpy().copy()
        passes.append((k, [host(t) for t in inp[:6]], inp[6], inp[7],
                       [host(t) for t in out[:4]], out[4]))
    dc = DensityControl(on_pass=on_pass, **LOOP)
    rows, hist = refine_splats(start, images, T_WC, K, 20, density=dc)
    return rows, hist, dc, passes, start


@pytest.mark.gpu
def test_hip_loop_with_density_control(parity):
    rows_a, hist_a, dc, passes, start = _loop_run()
    rows_b, hist_b, dc_b, _, _ = _loop_run()
    assert torch.equal(rows_a, rows_b) and torch.equal(hist_a, hist_b)
    assert dc.log == dc_b.log and torch.equal(dc.origin, dc_b.origin)
    print("passes:", dc.log)
    assert [e["t"] for e in dc.log] == [5, 10, 15, 20] and len(passes) == 4
    n = start.shape[0]
    for e in dc.log:                                     # the bookkeeping of .log
        assert e["n"] == n
        n = n - e["pruned"] + e["cloned"] + e["split"]
        assert e["n_out"] == n
    assert rows_a.shape == (n, 14) and dc.origin.shape == (n,)
    assert sum(e["cloned"] for e in dc.log) > 0 and sum(e["split"] for e in dc.log) > 0
    # the 500 are gone after the first pass
    o0 = passes[0][4][3].astype(np.int64)
    assert not (np.where(o0 >= 0, o0, ~o0) >= 2048).any() and dc.log[0]["pruned"] >= 500
    src = torch.where(dc.origin >= 0, dc.origin, ~dc.origin)
    assert int(src.max()) < 2048 and bool((src[1:] >= src[:-1]).all())
    assert bool(torch.isfinite(rows_a).all())
    h = hist_a.cpu().numpy()
    print("losses:", h)
    # every pass's captured inputs through the float64 reference
    for k, inp, hp, cap, out, counts in passes:
        p = dict(grad_threshold=hp.grad_threshold, split_scale=hp.split_scale,
                 min_opacity=hp.min_opacity, max_scale=hp.max_scale,
                 max_screen_radius=hp.max_screen_radius, seed=hp.seed,
                 **{"pass": getattr(hp, "pass")})
        assert getattr(hp, "pass") == k
        want = D.densify(inp[0], inp[1], inp[2], tuple(inp[3:6]), p, cap)
        assert want["near"].mean() <= 0.01
        got = dict(rows=out[0], m=out[1], v=out[2], origin=out[3], n_out=len(out[0]),
                   counts=tuple(counts[c] for c in ("pruned", "cloned", "split", "denied")))
        compare(got, want, inp[:3], f"hip.loop.pass{k}", parity)
    assert h[-1] < h[0]


@pytest.mark.gpu
def test_hip_map_refine_with_density_control():
    from test_refine import H, W, _map_of, _map_rows, _scene
    from splatt3r_amd.refine import DensityControl, render_splats
    _, T_WC, K = _scene()
    t, start, _ = _map_rows()
    start[900:, 6] = 3.0                                 # outside every view: opaque, small
    start[900:, 7:10] = -6.0
    kf = ((torch.arange(1000, device="cuda") * 7) // 1000).to(torch.int32)
    images = render_splats(t, T_WC, K, H, W)
    gm = _map_of(start, kf)
    fields = lambda m, n: [x[:n].clone() for x in (m.means, m.cov_triu, m.colors, m.opacities)]
    before = fields(gm, 1000)
    dc = DensityControl(**MAP)
    hist = gm.refine(images, T_WC, K, 12, density=dc)
    assert dc.capacity == 2048 and hist.shape == (12,)
    n_final = dc.log[-1]["n_out"]
    print("map passes:", dc.log)
    assert len(dc.log) == 2 and n_final != 1000 and gm.n_gaussians == n_final
    src = torch.where(dc.origin >= 0, dc.origin, ~dc.origin).long()
    kf_new = gm.kf_id[:n_final]
    assert torch.equal(kf_new, kf[src]) and bool((kf_new[1:] >= kf_new[:-1]).all())
    after = fields(gm, n_final)
    where = torch.nonzero(dc.origin >= 900).flatten()    # the outside Gaussians, survived
    assert where.numel() == 100 and torch.equal(dc.origin[where].long(), torch.arange(900, 1000).cuda())
    for a, b in zip(after, before):
        assert torch.equal(a[where], b[900:])
    # density=None leaves the count as before
    gm2 = _map_of(start, kf)
    gm2.refine(images, T_WC, K, 3)
    assert gm2.n_gaussians == 1000 and torch.equal(gm2.kf_id[:1000], kf)
