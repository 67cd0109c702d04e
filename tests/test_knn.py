"""Exact k nearest neighbours on the uniform grid: the arithmetic
(csrc/nn_search_math.hpp search_k), the HIP kernels (csrc/nn_search.hip
k_nn_knn, include/s3k.h s3k_knn) and splatt3r_amd.nn's knn, knn_scale.

Reference: tests/knn_ref64.py -- numpy float64, every candidate sorted with
np.lexsort((index, d2)), no grid; it takes nothing from the code under test.
Every comparison (indices, distances, the two means) is exact, bit for bit:
the grid only decides which rows are looked at, the slots are a total order,
and the means are sums in slot order in double, one rounding per operation.

One table of cases (cases()) is run twice: by the host program
tests/native/knn_host.cpp, which runs the same header on the CPU with the grid
built serially, and by the kernels.  Sizes: one below, at and above the
64-lane wave, the 256-thread workgroup and the 2,048-item segment of the
sort; k = 1, 3, 4, 8, 16, 32 covers the four slot capacities (4, 8, 16, 32)
at and below their limit, and k > n - 1 the padding slots.
"""
import ctypes
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import knn_ref64 as R
import nn_search_ref64 as R1
from conftest import REPO

f32 = np.float32
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
OUTPUTS = ("idx", "dist", "mean", "mean_sq")
bits = lambda x: np.ascontiguousarray(np.asarray(x, f32)).view(np.int32)


# ------------------------------------------------------------ shared data --
def _lattice(k, spacing):
    g = np.arange(k, dtype=np.float64) * spacing
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(f32)


@functools.lru_cache(maxsize=None)
def cloud(n, seed=3):
    return np.random.default_rng(seed).uniform(0, 1, (n, 3)).astype(f32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(ref, q, grid (origin, cell, dims) or None: the default
    grid, max_dist, exclude_self, ks)."""
    rng = np.random.default_rng(17)
    out = {}

    def add(name, ref, q, ks, grid=None, max_dist=np.inf, exclude_self=False):
        out[name] = dict(ref=np.ascontiguousarray(ref, f32), q=np.ascontiguousarray(q, f32),
                         grid=grid, max_dist=max_dist, exclude_self=exclude_self, ks=ks)
    for n in SIZES:                                   # self-queries; k > n - 1 pads
        add(f"self_n{n}", cloud(n), cloud(n), (1, 3, 8, 32), exclude_self=True)
    far = np.array([[50, 50, 50], [-30, 0.2, 0.2]], f32)
    ref = cloud(700, 4)
    q = np.concatenate([rng.uniform(-0.3, 1.3, (300, 3)).astype(f32), ref[:40], far])
    add("separate", ref, q, (1, 4, 16))
    add("separate_max_dist", ref, q, (1, 4, 16), max_dist=0.2)
    # a 6^3 lattice, every point stored five times: more coincident rows than slots
    lat = _lattice(6, 0.25)
    five = np.tile(lat, (5, 1))
    centres = (_lattice(5, 0.25).astype(np.float64) + 0.125).astype(f32)
    g6 = ((0.0, 0.0, 0.0), 0.25, (6, 6, 6))
    add("ties", five, np.concatenate([lat, centres]), (3, 8), grid=g6)
    add("ties_self", five, five, (3, 8), grid=g6, exclude_self=True)
    # whatever the grid: one cloud under four grids
    pts = cloud(500, 6)
    qs = np.concatenate([rng.uniform(-0.5, 1.5, (200, 3)).astype(f32), far])
    add("grid_1_1_1", pts, qs, (3, 16), grid=((0.0, 0.0, 0.0), 0.3, (1, 1, 1)))
    add("grid_1_1_64", pts, qs, (3, 16), grid=((0.0, 0.0, 0.0), 1.0 / 64.0, (1, 1, 64)))
    add("grid_huge_cell", pts, qs, (3, 16), grid=((0.0, 0.0, 0.0), 10.0, (4, 4, 4)))
    add("grid_default", pts, qs, (3, 16))
    # cells 100 times smaller than the spacing of 27 points; k = 32 pads
    l3 = _lattice(3, 0.5)
    q3 = rng.uniform(-0.1, 1.1, (64, 3)).astype(f32)
    add("grid_tiny_cells", l3, q3, (1, 8, 32), grid=((0.0, 0.0, 0.0), 0.005, (201, 201, 201)))
    add("grid_tiny_cells_one", l3, q3, (1, 8, 32), grid=((0.0, 0.0, 0.0), 0.005, (1, 1, 1)))
    # two tight clusters 3 units apart: long ring walks and the linear rest
    cl = np.concatenate([rng.normal(0, 0.02, (300, 3)), rng.normal(0, 0.02, (300, 3)) + [3, 0, 0]])
    between = rng.uniform(0, 1, (100, 1)) * [3, 0, 0] + rng.normal(0, 0.3, (100, 3))
    add("clusters", cl, between, (3, 16), grid=((-0.1, -1.6, -1.6), 0.2, (16, 16, 16)))
    # non-finite rows in the reference and in the query
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3], f32)
    dirty = np.concatenate([cloud(300, 8)[:150], odd, cloud(300, 8)[150:]])
    add("non_finite", dirty, np.concatenate([cloud(60, 9), odd]), (4, 8))
    add("non_finite_self", dirty, dirty, (3, 32), exclude_self=True)
    # max_dist: exactly at it, one float above, zero with coincident rows
    two = np.array([[0.5, 0, 0], [4, 4, 4]], f32)
    above = np.array([[np.nextafter(f32(0.5), f32(1)), 0, 0], [4, 4, 4]], f32)
    zero = np.zeros((1, 3), f32)
    g5 = ((0.0, 0.0, 0.0), 0.3, (5, 5, 5))
    add("max_dist_at", two, zero, (1, 4), grid=g5, max_dist=0.5)
    add("max_dist_above", above, zero, (1, 4), grid=g5, max_dist=0.5)
    add("max_dist_below", two, zero, (1, 4), grid=g5, max_dist=float(np.nextafter(0.5, 0)))
    add("max_dist_zero", np.concatenate([two, two]), np.array([[0.5, 0, 0], [0.5, 0, 1e-30]], f32),
        (1, 4), grid=g5, max_dist=0.0)
    add("empty_ref", np.zeros((0, 3), f32), cloud(5), (1, 4))
    return out


@functools.lru_cache(maxsize=None)
def neighbours(name):
    c = cases()[name]
    return R.neighbours(c["q"], c["ref"], c["max_dist"], c["exclude_self"])


def want(name, k):
    return R.rows(*neighbours(name), k)


def _same(got, w, label, parity=None, names=OUTPUTS):
    """Every output named equals the reference bit for bit."""
    bad = 0
    for o in names:
        g = np.asarray(got[o]).reshape(w[o].shape)
        bad += int((g != w[o]).sum() if o == "idx" else (bits(g) != bits(w[o])).sum())
    if parity is not None:       # entries whose bits differ; exact: 0
        parity(label, err=float(bad), tol=0.0)
    for o in names:
        g = np.asarray(got[o]).reshape(w[o].shape)
        if o == "idx":
            rows = np.nonzero((g != w[o]).reshape(len(g), -1).any(1))[0]
            assert len(rows) == 0, (label, o, rows[:5], g[rows[:5]], w[o][rows[:5]])
        else:
            assert np.array_equal(bits(g), bits(w[o])), (label, o)


# ---------------------------------------------------- CPU: the reference --
def test_reference_cases_worked_by_hand():
    ref = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [1, 0, 0], [np.nan, 0, 0]], f32)
    got = R.knn(np.array([[0, 0, 0], [np.inf, 0, 0]], f32), ref, 4)
    assert got["idx"].tolist() == [[0, 1, 3, 2], [-1, -1, -1, -1]]       # the tie: 1 before 3
    assert got["dist"][0].tolist() == [0.0, 1.0, 1.0, 3.0] and np.isinf(got["dist"][1]).all()
    assert got["mean"][0] == f32(5.0 / 4) and got["mean_sq"][0] == f32(11.0 / 4)
    assert np.isinf(got["mean"][1]) and np.isinf(got["mean_sq"][1])
    own = R.knn(ref, ref, 2, exclude_self=True)
    assert own["idx"].tolist() == [[1, 3], [3, 0], [1, 3], [1, 0], [-1, -1]]
    part = R.knn(ref[:1], ref, 4, max_dist=1.0)                          # partly filled
    assert part["idx"].tolist() == [[0, 1, 3, -1]] and part["mean"][0] == f32(2.0 / 3)
    assert part["dist"][0, 3] == np.inf
    # the means are sums in slot order: a case where pairwise summing differs
    d = np.array([1e16, 1.0, 1.0, 1.0], np.float64)
    assert ((d[0] + d[1]) + d[2]) + d[3] != (d[0] + d[1]) + (d[2] + d[3])
    line = np.stack([np.sqrt(d), 0 * d, 0 * d], 1).astype(f32)
    got = R.knn(np.zeros((1, 3), f32), line, 4)
    x2 = line[:, 0].astype(np.float64) ** 2
    assert got["mean_sq"][0] == f32((((x2[1] + x2[2]) + x2[3]) + x2[0]) / 4)


def test_inputs_cover_the_cases():
    c = cases()
    t = want("ties", 3)
    assert (t["idx"][:216] == np.arange(216)[:, None] + [0, 216, 432]).all()   # lowest copies
    assert (t["dist"][:216] == 0).all()
    t8 = want("ties", 8)
    assert (t8["idx"][:216, :5] == np.arange(216)[:, None] + 216 * np.arange(5)).all()
    assert (want("ties_self", 3)["idx"][0] == [216, 432, 648]).all()
    md = want("separate_max_dist", 16)
    filled = (md["idx"] >= 0).sum(1)
    assert (filled == 0).any() and (filled == 16).any() and ((filled > 0) & (filled < 16)).sum() > 50
    assert np.isinf(md["mean"][filled == 0]).all() and np.isfinite(md["mean"][filled > 0]).all()
    assert (want("self_n2", 3)["idx"] == [[1, -1, -1], [0, -1, -1]]).all()
    assert (want("self_n1", 1)["idx"] == [[-1]]).all()
    assert (want("grid_tiny_cells", 32)["idx"][:, 27:] == -1).all()
    assert (want("grid_tiny_cells", 32)["idx"][:, :27] >= 0).all()
    assert want("max_dist_at", 1)["idx"].tolist() == [[0]]
    assert want("max_dist_above", 1)["idx"].tolist() == [[-1]]
    assert want("max_dist_below", 1)["idx"].tolist() == [[-1]]
    assert want("max_dist_zero", 4)["idx"].tolist() == [[0, 2, -1, -1], [-1, -1, -1, -1]]
    nf = want("non_finite_self", 3)["idx"]
    assert (nf[150:154] == -1).all() and (nf[:150] >= 0).all() and not np.isin(nf, [150, 151, 152, 153]).any()
    for name in ("grid_1_1_64", "grid_huge_cell", "grid_default"):             # one cloud
        assert c[name]["ref"] is not None and np.array_equal(c[name]["q"], c["grid_1_1_1"]["q"])


def test_k1_is_the_nearest_neighbour_reference():
    """k = 1 without exclude_self restates nn_search_ref64.nearest."""
    for name in ("separate", "separate_max_dist", "non_finite"):
        c = cases()[name]
        idx, dist = R1.nearest(c["q"], c["ref"], c["max_dist"])
        w = R.rows(*neighbours(name), 1)
        assert np.array_equal(w["idx"][:, 0], idx) and np.array_equal(bits(w["dist"][:, 0]), bits(dist))


# ------------------------------------------- CPU: the arithmetic, host build
@functools.lru_cache(maxsize=None)
def _host_exe():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    import atexit
    import tempfile
    d = tempfile.mkdtemp(prefix="knn_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "knn_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(REPO, "splatt3r-slam_amd", "csrc"),
                    "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "native", "knn_host.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _grid_of(c):
    if c["grid"] is not None:
        return c["grid"]
    from splatt3r_amd import nn
    return nn.default_grid(torch.from_numpy(c["ref"]))      # host arithmetic on a host tensor


def _host_knn(c, k):
    exe = _host_exe()
    if exe is None:
        pytest.skip("hipcc not available")
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    n, m = len(c["ref"]), len(c["q"])
    with open(fin, "wb") as f:
        f.write(c["ref"].tobytes())
        f.write(c["q"].tobytes())
    origin, cell, dims = _grid_of(c)
    subprocess.run([exe, fin, fout, str(n), str(m)] + [repr(float(v)) for v in origin] +
                   [repr(float(cell))] + [str(v) for v in dims] +
                   [repr(float(c["max_dist"])), str(k), str(int(c["exclude_self"]))],
                   check=True, timeout=300)
    raw = open(fout, "rb").read()
    o = 0

    def take(dt, count):
        nonlocal o
        a = np.frombuffer(raw, dt, count, o)
        o += a.nbytes
        return a
    got = dict(idx=take(np.int32, m * k).reshape(m, k), dist=take(f32, m * k).reshape(m, k),
               mean=take(f32, m), mean_sq=take(f32, m), cells=take(np.int64, m),
               rows=take(np.int64, m), rings=take(np.int32, m), linear=take(np.int32, m))
    assert o == len(raw)
    return got, dims


@pytest.mark.parametrize("name", sorted(cases()))
def test_host_search_k_vs_brute_force(name, parity):
    c = cases()[name]
    kept = int(np.isfinite(c["ref"]).all(1).sum())
    for k in c["ks"]:
        got, dims = _host_knn(c, k)
        _same(got, want(name, k), f"host.{name}.k{k}", parity)
        # bounded work: no cell and no row twice
        assert (got["cells"] <= dims[0] * dims[1] * dims[2]).all() and (got["rows"] <= kept).all()
        if name == "clusters":     # both the long ring walk and the linear rest are exercised
            assert got["linear"].sum() >= 10 and (got["linear"] == 0).sum() >= 10
            assert ((got["linear"] == 0) & (got["rings"] >= 3)).any()
        if name == "self_n2049" and k == 3:   # and the stop rule stops: most queries end early
            assert np.median(got["rows"]) < kept / 4, np.median(got["rows"])


def test_host_bits_do_not_depend_on_the_grid():
    names = ("grid_1_1_1", "grid_1_1_64", "grid_huge_cell", "grid_default")
    for k in (3, 16):
        outs = [_host_knn(cases()[n], k)[0] for n in names]
        for o in outs[1:]:
            for key in OUTPUTS:
                assert np.array_equal(o[key].view(np.int32), outs[0][key].view(np.int32)), (k, key)
    a, b = (_host_knn(cases()[n], 32)[0] for n in ("grid_tiny_cells", "grid_tiny_cells_one"))
    for key in OUTPUTS:
        assert np.array_equal(a[key].view(np.int32), b[key].view(np.int32)), key


# ------------------------------------------------------------ CPU: the ABI --
def test_abi_rejects_bad_arguments_before_any_device_work():
    """Status 1 with a message; the pointers are never dereferenced (they are
    not device memory here)."""
    from splatt3r_amd import _lib
    lib = _lib.lib()
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)

    def knn(n=5, m=3, k=3, ex=0, cell=0.5, dims=(4, 4, 4), grid=0x100000, gb=1 << 20, q=0x1000,
            md=1.0, idx=0x2000, dist=0x3000, mean=0x4000, msq=0x5000, ws=0x200000, wb=1 << 20):
        return lib.s3k_knn(grid, gb, n, org, cell, *dims, q, m, k, ex, md, idx, dist, mean, msq,
                           ws, wb, None)
    for kw, msg in ((dict(k=0), b"k must be"), (dict(k=33), b"k must be"), (dict(k=-1), b"k must be"),
                    (dict(idx=None, dist=None, mean=None, msq=None), b"every output is null"),
                    (dict(ex=1, m=6), b"exclude_self"), (dict(m=-1), b"m < 0"),
                    (dict(cell=0.0), b"cell"), (dict(md=-1.0), b"max_dist"),
                    (dict(md=float("nan")), b"max_dist"), (dict(dims=(1024, 1024, 129)), b"2^27"),
                    (dict(gb=64), b"grid workspace too small"), (dict(q=None), b"null q"),
                    (dict(wb=64), b"workspace too small"), (dict(ws=None), b"workspace too small"),
                    (dict(ws=0x100000), b"overlaps"), (dict(ws=0x200010), b"aligned"),
                    (dict(q=0x100100), b"overlaps the grid or"), (dict(idx=0x200100), b"overlaps"),
                    (dict(dist=0x1000), b"overlap each other"), (dict(msq=0x4000), b"each other"),
                    (dict(idx=0x2000, dist=0x2020), b"each other")):
        assert knn(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    # m = 0 does nothing, whatever the pointers; the argument checks still hold
    assert knn(m=0, q=None, ws=None, wb=0) == 0 and lib.s3_last_error() == b""
    assert knn(m=0, k=40) == 1 and b"k must be" in lib.s3_last_error()
    assert knn(m=0, ex=1) == 0
    assert lib.s3k_knn_workspace_bytes(0) == 0
    assert lib.s3k_knn_workspace_bytes(3000) == lib.s3k_query_workspace_bytes(3000) >= 48000
    top = (1 << 31) - 2048
    assert lib.s3k_knn_workspace_bytes(top) > 0 and lib.s3k_knn_workspace_bytes(top + 1) == 0


def test_python_validation_needs_no_gpu():
    from splatt3r_amd import _abi, nn
    assert nn.MAX_K == _abi.constants["S3K_MAX_K"] == 32
    assert nn.KNN_OUTPUTS == OUTPUTS
    sig = _abi.functions["s3k_knn"][1]
    assert len(sig) == 20 and sig[10] is ctypes.c_int32 and sig[12] is ctypes.c_double
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        nn.knn(z, z, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        nn.knn_scale(z)
    with pytest.raises(RuntimeError, match="GPU only"):
        nn.outlier_mask(z)
    with pytest.raises(TypeError):
        nn.outlier_mask(z.double())


# --------------------------------------------------------------------- GPU --
def _cuda(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _grid(c):
    from splatt3r_amd.nn import PointGrid
    g = c["grid"]
    kw = {} if g is None else dict(origin=g[0], cell=g[1], dims=g[2])
    return PointGrid(_cuda(c["ref"]), **kw)


def _host(out):
    return {o: t.cpu().numpy() for o, t in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cases()))
def test_hip_knn_vs_brute_force(name, parity):
    c = cases()[name]
    grid, q = _grid(c), _cuda(c["q"])
    for k in c["ks"]:
        got = grid.knn(q, k, c["max_dist"], c["exclude_self"], want=OUTPUTS)
        assert got["idx"].shape == (len(c["q"]), k) and got["mean"].shape == (len(c["q"]),)
        _same(_host(got), want(name, k), f"hip.{name}.k{k}", parity)
    assert np.array_equal(bits(grid.ref.cpu().numpy()), bits(c["ref"]))   # inputs left as they were


@pytest.mark.gpu
def test_hip_k1_equals_the_query(parity):
    """k = 1 without exclude_self is PointGrid.query bit for bit, max_dist included."""
    for name in ("separate", "separate_max_dist", "non_finite", "clusters", "ties"):
        c = cases()[name]
        grid, q = _grid(c), _cuda(c["q"])
        idx, dist = grid.query(q, c["max_dist"])
        got = grid.knn(q, 1, c["max_dist"])
        assert sorted(got) == ["dist", "idx"]
        assert torch.equal(got["idx"][:, 0], idx)
        assert torch.equal(got["dist"][:, 0].contiguous().view(torch.int32), dist.view(torch.int32))
        parity(f"hip.k1.{name}", err=float((got["idx"][:, 0] != idx).sum()), tol=0.0)


@pytest.mark.gpu
def test_hip_optional_outputs_and_determinism():
    from splatt3r_amd import nn
    c = cases()["separate_max_dist"]
    grid, q = _grid(c), _cuda(c["q"])
    for k in (4, 16):
        full = grid.knn(q, k, c["max_dist"], want=OUTPUTS)
        again = grid.knn(q, k, c["max_dist"], want=OUTPUTS)
        for o in OUTPUTS:
            assert torch.equal(full[o].view(torch.int32), again[o].view(torch.int32)), o
        for sub in (("mean",), ("mean_sq", "idx"), "dist"):
            part = grid.knn(q, k, c["max_dist"], want=sub)
            names = (sub,) if isinstance(sub, str) else sub
            assert tuple(part) == names
            for o in names:
                assert torch.equal(part[o].view(torch.int32), full[o].view(torch.int32)), (sub, o)
    # the module-level forms
    r = _cuda(c["ref"])
    one = nn.knn(q, r, 4, max_dist=c["max_dist"], want=OUTPUTS)
    _same(_host(one), want("separate_max_dist", 4), "hip.nn.knn")
    empty = grid.knn(q[:0], 3, want=OUTPUTS)
    assert empty["idx"].shape == (0, 3) and empty["mean"].shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (2, 257, 2049))
def test_hip_knn_scale(n, parity):
    """nn.knn_scale is mean_sq of the self-query (3DGS's distCUDA2, k = 3)."""
    from splatt3r_amd import nn
    got = nn.knn_scale(_cuda(cloud(n))).cpu().numpy()
    w = want(f"self_n{n}", 3)["mean_sq"]
    parity(f"hip.knn_scale.n{n}", err=float((bits(got) != bits(w)).sum()), tol=0.0)
    assert np.array_equal(bits(got), bits(w))
    got8 = nn.knn_scale(_cuda(cloud(n)), k=8, cell=0.2).cpu().numpy()
    assert np.array_equal(bits(got8), bits(want(f"self_n{n}", 8)["mean_sq"]))


@pytest.mark.gpu
def test_hip_bad_arguments_raise_before_any_launch():
    from splatt3r_amd import _lib
    from splatt3r_amd.nn import PointGrid
    lib = _lib.lib()
    ref = _cuda(cloud(100))
    g = PointGrid(ref)
    for kw in (dict(k=0), dict(k=33), dict(k=3, want=()), dict(k=3, want=("idx", "median")),
               dict(k=3, max_dist=-1.0)):
        with pytest.raises(ValueError):
            g.knn(ref, **kw)
    with pytest.raises(ValueError, match="exclude_self"):
        g.knn(_cuda(cloud(101)), 3, exclude_self=True)
    with pytest.raises(TypeError):
        g.knn(ref.half(), 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        g.knn(ref.cpu(), 3)
    # through the ABI: status 1 and a message, nothing launched
    org = (ctypes.c_double * 3)(*g.origin)
    ws = torch.empty(1 << 16, device="cuda", dtype=torch.uint8)
    idx = torch.full((100, 3), 7, device="cuda", dtype=torch.int32)

    def call(k=3, ex=0, m=100, idx_p=idx.data_ptr()):
        return lib.s3k_knn(g._grid.data_ptr(), g._grid.numel(), 100, org, g.cell, *g.dims,
                           ref.data_ptr(), m, k, ex, math.inf, idx_p, None, None, None,
                           ws.data_ptr(), ws.numel(), _lib.stream(ref.device))
    for kw, msg in ((dict(k=0), b"k must be"), (dict(k=33), b"k must be"),
                    (dict(idx_p=None), b"every output is null"), (dict(ex=1, m=101), b"exclude_self")):
        assert call(**kw) == 1 and msg in lib.s3_last_error(), kw
    assert (idx == 7).all()
    # and the library still works
    _same(_host(g.knn(ref, 3, exclude_self=True, want=OUTPUTS)), R.knn(cloud(100), cloud(100), 3,
                                                                     exclude_self=True), "after")
