"""3DGS splat .ply export / import: the file format on the host, the
per-Gaussian arithmetic (csrc/splat_math.hpp) and the HIP kernels
(csrc/splat_io.hip, include/s3w.h s3w_map_to_splats / s3w_map_from_splats).

Reference: float64 (numpy.linalg.eigvalsh of the float32 covariance,
quaternion -> rotation in float64; tests/splat_ref64.py).  Eigenvectors are
never compared; a row is judged by the covariance it reconstructs, by its
eigenvalues, and by its structure (unit quaternion, w >= 0, scales
non-increasing, finite).

Tolerances (the rule of test_raster_grad.py / test_loss_mask.py): the floor
of a quantity is the error of the float32 host restatement (torch.linalg.eigh
on CPU float32 + numpy float32 elementwise maps, splat_ref64.host32_rows /
host32_import) on the same inputs against the same float64 reference, and
the tolerance is 4 x floor rounded up to one significant digit.  The floors
are computed here on every run, printed, and recorded through the `parity`
fixture; nothing is derived from the kernel's output.  Measured floors (max
over the set, on the MI355X host; they move by ~10 % with the LAPACK build)
and what the code under test gave:

  quantity                          floor    tolerance  host build  MI355X
  random 1000  recon  (rel. Frob.)  7.0e-7   3e-6       6.2e-7      1.4e-6
  random 1000  eig    (/ lam_max)   7.0e-7   3e-6       6.2e-7      1.8e-6
  random 1000  | |q| - 1 |          1.1e-7   5e-7       1.5e-7      1.5e-7
  random 1000  colour (abs)         5.6e-8   3e-7       5.6e-8      5.6e-8
  random 1000  opacity (abs)        2.9e-8   2e-7       2.6e-8      3.6e-8
  hand-built   recon                6.6e-7   3e-6       6.8e-7      1.0e-6
  hand-built   eig                  6.8e-7   3e-6       6.8e-7      1.1e-6
  hand-built   | |q| - 1 |          6.7e-8   3e-7       1.3e-7      1.3e-7
  hand-built   colour (abs)         3.4e-8   2e-7       3.4e-8      3.4e-8
  hand-built   opacity (abs)        1.8e-8   8e-8       1.2e-8      2.1e-8
  import cov (rel. Frob.)           1.1e-6   5e-6       9.0e-7      1.4e-6
  import colour (abs)               6.0e-8   3e-7       6.0e-8      6.0e-8
  import opacity (abs)              6.0e-8   3e-7       6.0e-8      6.0e-8
  render, mean |image diff|         1.9e-7   8e-7       -           1.2e-7

The device's scale errors exceed the host build's because its logf is less
exact (1.2 ulp measured at log 0.05; one ulp at |scale| = 6.9 is 4.8e-7,
doubled in exp(2 scale)).

"host build" is splat_math.hpp compiled for the CPU
(tests/native/splat_rows_host.cpp): the same source the kernels call, so the
arithmetic is checked without a GPU too.
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import splat_ref64 as R
from conftest import REPO

SIZES = (1, 63, 64, 65, 257, 1000)
N = 1000
SENTINEL = np.int32(0x7FC0BEEF)          # a NaN bit pattern no kernel computes


# ------------------------------------------------------------ shared data --
@functools.lru_cache(maxsize=None)
def random_inputs():
    return R.random_gaussians(N, seed=1234)


@functools.lru_cache(maxsize=None)
def hand_inputs():
    return R.hand_built_inputs()[1]


def _floors(inp, rows32):
    e = R.export_errors(inp[1], rows32)
    a = R.attribute_errors(inp[2], inp[3], rows32)
    return {k: float(np.nanmax(v)) for k, v in {**e, **a}.items()}


@functools.lru_cache(maxsize=None)
def random_floors():
    inp = random_inputs()
    return _floors(inp, R.host32_rows(*inp))


@functools.lru_cache(maxsize=None)
def hand_floors():
    inp = hand_inputs()
    return _floors(inp, R.host32_rows(*inp))


@functools.lru_cache(maxsize=None)
def import_floors():
    inp = random_inputs()
    back = R.host32_import(R.host32_rows(*inp)[:, R.ROWS14])
    return R.import_errors(inp, back)


def check_rows(inp, rows, floors, label, parity, names=None):
    """Every export check of one set of rows against float64."""
    means, cov, colors, op = inp
    rows = np.asarray(rows)
    assert rows.shape == (len(means), 17) and rows.dtype == np.float32
    assert np.array_equal(rows[:, :3].view(np.int32), means.view(np.int32)), "means not bit-exact"
    assert R.structure_ok(rows), label
    errs = {**R.export_errors(cov, rows), **R.attribute_errors(colors, op, rows)}
    for k, v in errs.items():
        worst = float(np.nanmax(v)) if np.any(~np.isnan(v)) else 0.0
        tol = R.tolerance(floors[k])
        where = int(np.nanargmax(v)) if np.any(~np.isnan(v)) else -1
        parity(f"{label}.{k}", err=worst, tol=tol, floor=floors[k])
        print(f"{label}.{k}: err {worst:.3e} floor {floors[k]:.3e} tol {tol:.1e}"
              + (f" worst {names[where]}" if names and where >= 0 else ""))
        assert worst <= tol, (label, k, worst, tol, names[where] if names else where)
    # the zero matrix is checked by its stated outputs: the identity quaternion
    # exactly, and log(scale_min) to the slack of a float32 logf
    zero = ~np.any(cov != 0, axis=1)
    if zero.any():
        want = np.log(np.float64(np.float32(R.SCALE_MIN)))
        assert np.all(np.abs(rows[zero, 10:13].astype(np.float64) - want) <= _log_slack(want))
        assert np.all(rows[zero, 10:13] == rows[zero, 10:11])
        assert np.all(rows[zero, 13:17] == np.array([1, 0, 0, 0], np.float32))


def _log_slack(want):
    """Error allowed on a float32 logf result near `want`: 3 ulp, the bound the
    OpenCL specification sets for single-precision log, which the device math
    library is written to (measured here: 1.2 ulp at log 0.05)."""
    return 3.0 * float(np.spacing(np.float32(abs(want))))


def _assert_scale_floor(rows, scale_min):
    """No scale below log(scale_min) (to the slack of a float32 logf); some at
    it (the clamp is active) and some well above."""
    want = np.log(np.float64(np.float32(scale_min)))
    s = rows[:, 10:13].astype(np.float64)
    assert np.all(s >= want - _log_slack(want))
    assert np.any(np.abs(s - want) <= _log_slack(want)) and np.any(s > want + 0.1)


# -------------------------------------------------------------- CPU: file --
def _rows(n, seed=5):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 17)).astype(np.float32)


EXPECTED_HEADER = (
    "ply\nformat binary_little_endian 1.0\nelement vertex {n}\n"
    "property float x\nproperty float y\nproperty float z\n"
    "property float nx\nproperty float ny\nproperty float nz\n"
    "property float f_dc_0\nproperty float f_dc_1\nproperty float f_dc_2\n"
    "property float opacity\n"
    "property float scale_0\nproperty float scale_1\nproperty float scale_2\n"
    "property float rot_0\nproperty float rot_1\nproperty float rot_2\nproperty float rot_3\n"
    "end_header\n")


@pytest.mark.parametrize("n", [0, 1, 5])
def test_writer_header_and_body(tmp_path, n):
    from splatt3r_amd.evaluate import write_splat_ply
    rows = _rows(n)
    p = tmp_path / "m.ply"
    write_splat_ply(p, rows)
    raw = p.read_bytes()
    head = EXPECTED_HEADER.format(n=n).encode("ascii")
    assert raw[:len(head)] == head
    assert raw[len(head):] == rows.astype("<f4").tobytes()
    assert len(raw) == len(head) + 68 * n


@pytest.mark.parametrize("n", [0, 1, 5, 1000])
def test_reader_round_trips_bit_exactly(tmp_path, n):
    from splatt3r_amd.evaluate import SPLAT_PROPERTIES, read_splat_ply, write_splat_ply
    rows = _rows(n)
    if n:
        rows[0, 4] = np.float32("nan")           # bits, not values, are kept
        rows.view(np.int32)[-1, 7] = int(SENTINEL)
    write_splat_ply(tmp_path / "m.ply", rows)
    got = read_splat_ply(tmp_path / "m.ply")
    assert list(got) == list(SPLAT_PROPERTIES)
    for k, name in enumerate(SPLAT_PROPERTIES):
        assert got[name].dtype == np.float32 and got[name].shape == (n,)
        assert np.array_equal(got[name].view(np.int32), rows[:, k].view(np.int32)), name


def _hand_file(path, n=7, seed=9, fmt="binary_little_endian", drop=None, retype=None,
               cut=0, body=None):
    """A file as a trainer writes it: x y z, normals, f_dc, 45 f_rest, opacity,
    scales, rotations -- then shuffled, with a uchar extra in the middle."""
    rng = np.random.default_rng(seed)
    names = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
             + [f"f_rest_{i}" for i in range(45)]
             + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
    names = [names[i] for i in rng.permutation(len(names))]
    names.insert(11, "label")
    names = [k for k in names if k != drop]
    types = {k: ("uchar", "u1") if k == "label" else ("float", "<f4") for k in names}
    if retype:
        types[retype[0]] = retype[1]
    rec = np.zeros(n, dtype=[(k, types[k][1]) for k in names])
    vals = {}
    for k in names:
        v = rng.integers(0, 200, n) if types[k][1] == "u1" else rng.normal(size=n)
        rec[k] = v
        vals[k] = rec[k].copy()
    head = (f"ply\nformat {fmt} 1.0\ncomment hand-written\nelement vertex {n}\n"
            + "".join(f"property {types[k][0]} {k}\n" for k in names) + "end_header\n")
    data = rec.tobytes() if body is None else body
    with open(path, "wb") as f:
        f.write(head.encode("ascii") + data[:len(data) - cut])
    return vals


def test_reader_finds_properties_by_name(tmp_path):
    from splatt3r_amd.evaluate import SPLAT_REQUIRED, read_splat_ply
    vals = _hand_file(tmp_path / "t.ply")
    got = read_splat_ply(tmp_path / "t.ply")
    assert set(got) == set(vals) and len(got) == 9 + 45 + 8 + 1
    for k in SPLAT_REQUIRED + ("f_rest_0", "f_rest_44", "nx"):
        assert got[k].dtype == np.float32
        assert np.array_equal(got[k].view(np.int32), vals[k].view(np.int32)), k
    assert got["label"].dtype == np.uint8 and np.array_equal(got["label"], vals["label"])


@pytest.mark.parametrize("case", ["ascii", "big_endian", "missing", "non_float", "truncated"])
def test_reader_rejections(tmp_path, case):
    from splatt3r_amd.evaluate import read_splat_ply
    p = tmp_path / "bad.ply"
    if case == "ascii":
        _hand_file(p, fmt="ascii", body=b"0 " * (63 * 7))
    elif case == "big_endian":
        _hand_file(p, fmt="binary_big_endian")
    elif case == "missing":
        _hand_file(p, drop="rot_2")
    elif case == "non_float":
        _hand_file(p, retype=("scale_1", ("double", "<f8")))
    else:
        _hand_file(p, cut=1)
    with pytest.raises(ValueError):
        read_splat_ply(p)


def test_save_gaussian_splats_without_a_map(tmp_path):
    from splatt3r_amd.evaluate import save_gaussian_splats
    assert save_gaussian_splats(tmp_path / "out", "map.ply", None) is None
    assert not (tmp_path / "out" / "map.ply").exists()


def test_import_rejects_bad_counts_before_any_device_work():
    """n > cap and n < 0 return status 1 with a message; the pointers are
    never dereferenced (they are not device memory here)."""
    from splatt3r_amd import _lib
    from splatt3r_amd.gaussian_map import S3wMap
    lib = _lib.lib()
    m = S3wMap(16, 16, 16, 16, 16, 16, 100)
    assert lib.s3w_map_from_splats(ctypes.byref(m), 16, 101, 0, None) == 1
    assert b"capacity" in lib.s3_last_error()
    assert lib.s3w_map_from_splats(ctypes.byref(m), 16, -1, 0, None) == 1
    assert b"n < 0" in lib.s3_last_error()
    assert lib.s3w_map_to_splats(16, 16, 16, 16, None, -1, 1e-7, 16, None) == 1
    assert b"n_max < 0" in lib.s3_last_error()
    # a call that succeeds (nothing to do for n_max = 0) clears the message
    assert lib.s3w_map_to_splats(None, None, None, None, None, 0, 1e-7, None, None) == 0
    assert lib.s3_last_error() == b""


# ------------------------------------------- CPU: the arithmetic, host build
@functools.lru_cache(maxsize=None)
def _host_exe():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    import atexit
    import tempfile
    d = tempfile.mkdtemp(prefix="splat_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "splat_rows_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(REPO, "splatt3r-slam_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "splat_rows_host.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _host_run(mode, arr, *extra):
    exe = _host_exe()
    if exe is None:
        pytest.skip("hipcc not available")
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    np.ascontiguousarray(arr, np.float32).tofile(fin)
    subprocess.run([exe, mode, fin, fout, *extra], check=True, timeout=300)
    return np.fromfile(fout, np.float32)


def _host_rows(inp, scale_min=R.SCALE_MIN):
    rec = np.concatenate([inp[0], inp[1], inp[2], inp[3][:, None]], 1)
    return _host_run("export", rec, repr(float(scale_min))).reshape(-1, 17)


def test_host_math_random(parity):
    inp = random_inputs()
    check_rows(inp, _host_rows(inp), random_floors(), "host.random", parity)


def test_host_math_hand_built(parity):
    names = R.hand_built_inputs()[0]
    check_rows(hand_inputs(), _host_rows(hand_inputs()), hand_floors(), "host.hand", parity,
               names)


def test_host_math_import(parity):
    inp = random_inputs()
    out = _host_run("import", _host_rows(inp)[:, R.ROWS14]).reshape(-1, 13)
    got = (out[:, :3], out[:, 3:9], out[:, 9:12], out[:, 12])
    assert np.array_equal(got[0].view(np.int32), inp[0].view(np.int32))
    errs, floors = R.import_errors(inp, got), import_floors()
    for k in errs:
        parity(f"host.import.{k}", err=errs[k], tol=R.tolerance(floors[k]), floor=floors[k])
        print(f"host.import.{k}: err {errs[k]:.3e} floor {floors[k]:.3e}")
        assert errs[k] <= R.tolerance(floors[k]), k


def test_host_math_raw_quaternion_and_scale_min():
    """Import normalises the quaternion; export honours scale_min."""
    inp = random_inputs()
    rows = _host_rows(inp)[:64, R.ROWS14]
    scaled = rows.copy()
    scaled[:, 10:14] *= np.float32(3.0)
    a = _host_run("import", rows).reshape(-1, 13)
    b = _host_run("import", scaled).reshape(-1, 13)
    S = np.linalg.norm(R.full(a[:, 3:9].astype(np.float64)), axis=(1, 2))
    d = np.linalg.norm(R.full(b[:, 3:9].astype(np.float64) - a[:, 3:9]), axis=(1, 2))
    assert np.max(d / S) <= R.tolerance(import_floors()["cov"])
    big = _host_rows(tuple(x[:64] for x in inp), scale_min=0.05)
    _assert_scale_floor(big, 0.05)


# --------------------------------------------------------------------- GPU --
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_rows(inp, n=None, **kw):
    from splatt3r_amd.gaussian_map import splats_from_cov
    return splats_from_cov(*[_cuda(x[:n]) for x in inp], **kw).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_hip_export_random(n, parity):
    inp = tuple(x[:n] for x in random_inputs())
    check_rows(inp, _gpu_rows(inp), random_floors(), f"hip.random{n}", parity)


@pytest.mark.gpu
def test_hip_export_hand_built(parity):
    names = R.hand_built_inputs()[0]
    check_rows(hand_inputs(), _gpu_rows(hand_inputs()), hand_floors(), "hip.hand", parity, names)


@pytest.mark.gpu
def test_hip_export_is_reproducible_and_independent_of_n():
    inp = random_inputs()
    a, b = _gpu_rows(inp), _gpu_rows(inp)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    first = _gpu_rows(inp, 137)
    assert np.array_equal(first.view(np.int32), a[:137].view(np.int32))


@pytest.mark.gpu
def test_hip_export_writes_only_live_rows():
    """Buffer [n_max + 8, 17] of a sentinel; *n_dev = 700, n_max = 1000: rows
    >= 700 keep the sentinel, rows < 700 are the rows of a plain call."""
    from splatt3r_amd import _lib
    d = [_cuda(x) for x in random_inputs()]
    buf = torch.full((N + 8, 17), int(SENTINEL), dtype=torch.int32, device="cuda")
    n_dev = torch.tensor([700], dtype=torch.int64, device="cuda")
    _lib.call("s3w_map_to_splats", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
              d[3].data_ptr(), n_dev.data_ptr(), N, 1e-7, buf.data_ptr(), _lib.stream())
    got = buf.cpu().numpy()
    assert np.all(got[700:] == SENTINEL)
    assert np.array_equal(got[:700], _gpu_rows(random_inputs(), 700).view(np.int32))


@pytest.mark.gpu
def test_hip_export_scale_min():
    """scale_min reaches the kernel."""
    inp = random_inputs()
    big = _gpu_rows(inp, 65, scale_min=0.05)
    _assert_scale_floor(big, 0.05)


def _filled_map(cap, inp, kf=3):
    from splatt3r_amd.gaussian_map import SharedGaussians
    gm = SharedGaussians(max_gaussians=cap, device="cuda")
    gm.append(*[_cuda(x) for x in inp], kf_idx=kf, opacity_threshold=-1.0)
    return gm


def _map_fields(gm, n):
    return tuple(t[:n].cpu().numpy() for t in (gm.means, gm.cov_triu, gm.colors, gm.opacities))


@pytest.mark.gpu
def test_hip_save_load_round_trip(tmp_path, parity):
    from splatt3r_amd.evaluate import read_splat_ply, save_gaussian_splats
    from splatt3r_amd.gaussian_map import SharedGaussians
    inp = random_inputs()
    gm = _filled_map(2048, inp)
    assert gm.n_gaussians == N
    assert save_gaussian_splats(tmp_path / "out", "map.ply", gm) == N
    path = tmp_path / "out" / "map.ply"
    assert os.path.getsize(path) == len(EXPECTED_HEADER.format(n=N)) + 68 * N
    on_disk = read_splat_ply(path)
    rows = gm.to_splats().cpu().numpy()
    assert np.array_equal(on_disk["rot_2"].view(np.int32), rows[:, 15].view(np.int32))
    # an explicit n reads no count on the host: rows past the count stay zero
    more_rows = gm.to_splats(N + 24).cpu().numpy()
    assert np.array_equal(more_rows[:N].view(np.int32), rows.view(np.int32))
    assert more_rows.shape == (N + 24, 17) and not more_rows[N:].any()

    new = SharedGaussians(max_gaussians=2048, device="cuda")
    assert new.load_ply(path, kf_idx=7) == N
    assert new.n_gaussians == N
    assert torch.all(new.kf_id[:N] == 7) and torch.all(new.kf_id[N:] == 0)
    got = _map_fields(new, N)
    assert np.array_equal(got[0].view(np.int32), inp[0].view(np.int32))
    errs, floors = R.import_errors(inp, got), import_floors()
    for k in errs:
        parity(f"hip.import.{k}", err=errs[k], tol=R.tolerance(floors[k]), floor=floors[k])
        print(f"hip.import.{k}: err {errs[k]:.3e} floor {floors[k]:.3e}")
        assert errs[k] <= R.tolerance(floors[k]), k
    # a following append lands behind the loaded rows
    more = tuple(x[:50] for x in R.random_gaussians(64, seed=77))
    new.append(*[_cuda(x) for x in more], kf_idx=9, opacity_threshold=-1.0)
    assert new.n_gaussians == N + 50
    assert np.array_equal(new.means[N:N + 50].cpu().numpy(), more[0])
    assert torch.all(new.kf_id[N:N + 50] == 9) and torch.all(new.kf_id[:N] == 7)
    # loading replaces: a shorter file shrinks the map
    small = _filled_map(256, tuple(x[:65] for x in inp))
    small.save_ply(tmp_path / "small.ply")
    assert new.load_ply(tmp_path / "small.ply") == 65 and new.n_gaussians == 65
    assert torch.all(new.kf_id[:65] == -1)


@pytest.mark.gpu
def test_hip_load_over_capacity_leaves_the_map_untouched(tmp_path):
    inp = random_inputs()
    _filled_map(2048, inp).save_ply(tmp_path / "big.ply")
    gm = _filled_map(512, tuple(x[:100] for x in inp))
    before = _map_fields(gm, 100)
    with pytest.raises(ValueError):
        gm.load_ply(tmp_path / "big.ply")
    assert gm.n_gaussians == 100
    for a, b in zip(before, _map_fields(gm, 100)):
        assert np.array_equal(a, b)
    assert torch.all(gm.kf_id[:100] == 3)


@pytest.mark.gpu
def test_hip_empty_map(tmp_path):
    from splatt3r_amd.evaluate import save_gaussian_splats
    from splatt3r_amd.gaussian_map import SharedGaussians
    gm = SharedGaussians(max_gaussians=64, device="cuda")
    assert save_gaussian_splats(tmp_path, "none.ply", gm) is None
    assert gm.save_ply(tmp_path / "empty.ply") == 0
    full = _filled_map(64, tuple(x[:10] for x in random_inputs()))
    assert full.load_ply(tmp_path / "empty.ply") == 0 and full.n_gaussians == 0


@functools.lru_cache(maxsize=None)
def _render_scene():
    """2048 Gaussians in front of a 64 x 48 camera (45 degree vertical field of
    view): means inside the frustum at depth 2..6."""
    P = 2048
    _, cov, colors, op = R.random_gaussians(P, seed=4321)
    rng = np.random.default_rng(99)
    z = rng.uniform(2.0, 6.0, P)
    t = np.tan(np.radians(22.5))
    means = np.stack([rng.uniform(-1, 1, P) * z * t * 64 / 48, rng.uniform(-1, 1, P) * z * t, z],
                     1).astype(np.float32)
    return means, cov, colors, np.maximum(op, np.float32(0.06))


def _render(means, colors, op, cov=None, scales=None, rots=None):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from splatt3r_amd.gaussian_map import VIZ_BG, viz_camera
    Wm, Hm = 64, 48
    tx, ty, view_t, proj, campos, s, s2 = viz_camera(np.eye(4, dtype=np.float32), Wm, Hm, 45.0)
    st = GaussianRasterizationSettings(
        image_height=Hm, image_width=Wm, tanfovx=tx, tanfovy=ty,
        bg=torch.tensor(VIZ_BG, dtype=torch.float32, device="cuda"), scale_modifier=1.0,
        viewmatrix=view_t.cuda(), projmatrix=proj.cuda(), sh_degree=0, campos=campos.cuda(),
        prefiltered=False, debug=False)
    m = _cuda(means) * np.float32(s)
    kw = dict(cov3D_precomp=_cuda(cov) * np.float32(s2)) if cov is not None else \
        dict(scales=_cuda(scales) * np.float32(s), rotations=_cuda(rots))
    out = GaussianRasterizer(st)(means3D=m, means2D=torch.zeros_like(m),
                                 colors_precomp=_cuda(colors), opacities=_cuda(op)[:, None], **kw)
    return out[0].cpu().numpy().astype(np.float64)


@pytest.mark.gpu
def test_hip_rasterizer_agrees_on_exported_scales_and_rotations(parity):
    """Rendering the map's covariances and rendering the exported (scale,
    quaternion) pairs give the same image, to 4 x the floor: the mean absolute
    difference between rendering Sigma and rendering the float32 host
    restatement's (scale, quaternion).  The mean, not the max: a 1/255 alpha
    skip or a radius ceil may flip single pixels."""
    means, cov, colors, op = _render_scene()
    base = _render(means, colors, op, cov=cov)
    assert base.std() > 0.02                       # the scene is visible
    r32 = R.host32_rows(means, cov, colors, op)
    floor = float(np.abs(_render(means, colors, op, scales=np.exp(r32[:, 10:13]),
                                 rots=r32[:, 13:17]) - base).mean())
    rows = _gpu_rows((means, cov, colors, op))
    err = float(np.abs(_render(means, colors, op, scales=np.exp(rows[:, 10:13]),
                               rots=rows[:, 13:17]) - base).mean())
    tol = R.tolerance(floor)
    parity("hip.render.mean_abs", err=err, tol=tol, floor=floor)
    print(f"hip.render.mean_abs: err {err:.3e} floor {floor:.3e} tol {tol:.1e}")
    assert err <= tol
