"""Exact nearest neighbour on a uniform grid, distance statistics and
area-uniform mesh sampling: the arithmetic (csrc/nn_search_math.hpp), the HIP
kernels (csrc/nn_search.hip, include/s3k.h) and splatt3r_amd.nn.

Reference: tests/nn_search_ref64.py -- numpy float64, brute force, no grid; it
takes nothing from the code under test.  Every comparison of an index, a
distance, a sampled face or a sampled point is exact (bit for bit): the grid
only decides which rows are looked at, the stratified sampler is integer
arithmetic plus one rounding per coordinate.  The two sums of dist_stats are
compared to the exactly rounded sums (math.fsum) to m 2^-52 relative: each
of the m additions in double rounds once.

The host program tests/native/nn_search_host.cpp runs the same header on the
CPU, the grid build written out serially; the GPU tests run the kernels.
Sizes: one below, at and above the 64-lane wave, the 256-thread workgroup and
the 2,048-item segment of the scans and the sort, and 8,000.
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

import nn_search_ref64 as R
from conftest import REPO

f32 = np.float32
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8000)
bits = lambda x: np.ascontiguousarray(np.asarray(x, f32)).view(np.int32)


# ------------------------------------------------------------ shared data --
def _lattice(k, spacing):
    g = np.arange(k, dtype=np.float64) * spacing
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(f32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (ref, q, (origin, cell, dims), max_dist)."""
    rng = np.random.default_rng(11)
    out = {}
    far = np.array([[50, 50, 50], [-30, 0.2, 0.2]], f32)
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3], f32)
    for name, cell in (("lattice_0.1", 0.1), ("lattice_0.25", 0.25), ("lattice_third", 1.0 / 3.0)):
        lat = _lattice(6, cell)                          # points on cell faces
        ref = np.concatenate([lat, lat[[0, 7, 43, 100, 101, 180, 215]],   # seven duplicates
                              odd[:3] + lat[:3] * 0])
        centres = (_lattice(5, cell).astype(np.float64) + 0.5 * cell).astype(f32)
        rnd = rng.uniform(-0.2, 6 * cell + 0.2, (200, 3)).astype(f32)
        q = np.concatenate([lat, centres, rnd, far, odd])
        out[name] = (ref, q, ((0.0, 0.0, 0.0), cell, (6, 6, 6)), np.inf)
    pts = rng.uniform(0, 1, (2000, 3)).astype(f32)
    qs = np.concatenate([rng.uniform(-0.5, 1.5, (300, 3)).astype(f32), pts[:50], far])
    out["one_cell"] = (pts, qs, ((0.0, 0.0, 0.0), 10.0, (4, 4, 4)), np.inf)
    out["dims_1_1_1"] = (pts[:300], qs[:100], ((0.0, 0.0, 0.0), 0.3, (1, 1, 1)), np.inf)
    out["dims_1_1_64"] = (pts[:700], qs, ((0.0, 0.0, 0.0), 1.0 / 64.0, (1, 1, 64)), np.inf)
    # two tight clusters 3 units apart, queries between and around them
    cl = np.concatenate([rng.normal(0, 0.02, (300, 3)), rng.normal(0, 0.02, (300, 3)) + [3, 0, 0]])
    t = rng.uniform(0, 1, (200, 1))
    between = t * [3, 0, 0] + rng.normal(0, 0.3, (200, 3))
    near = cl[rng.integers(0, 600, 60)] + rng.normal(0, 0.05, (60, 3))
    out["clusters"] = (cl.astype(f32), np.concatenate([between, near]).astype(f32),
                       ((-0.1, -1.6, -1.6), 0.2, (16, 16, 16)), np.inf)
    # cells 100 times smaller than the point spacing
    out["tiny_cell"] = (_lattice(3, 0.5), rng.uniform(-0.1, 1.1, (64, 3)).astype(f32),
                        ((0.0, 0.0, 0.0), 0.005, (201, 201, 201)), np.inf)
    # a finite max_dist over the lattice and random queries
    out["max_dist"] = (out["lattice_0.25"][0], out["lattice_0.25"][1],
                       ((0.0, 0.0, 0.0), 0.25, (6, 6, 6)), 0.11)
    return out


@functools.lru_cache(maxsize=None)
def want(name):
    ref, q, _, max_dist = cases()[name]
    return R.nearest(q, ref, max_dist)


@functools.lru_cache(maxsize=None)
def cloud(n, seed=3):
    return np.random.default_rng(seed).uniform(0, 1, (n, 3)).astype(f32)


@functools.lru_cache(maxsize=None)
def want_sizes(n):
    return R.nearest(cloud(n, 4), cloud(n, 3))


def max_dist_cases():
    """(ref, q, max_dist, idx): a winner exactly at max_dist is kept, one a
    float above is not; max_dist 0 with a coincident point."""
    ref = np.array([[0.5, 0, 0], [4, 4, 4]], f32)
    above = np.nextafter(f32(0.5), f32(1))
    return ((ref, np.array([[0, 0, 0]], f32), 0.5, 0),
            (np.array([[above, 0, 0], [4, 4, 4]], f32), np.array([[0, 0, 0]], f32), 0.5, -1),
            (ref, np.array([[0.5, 0, 0], [0.5, 0, 1e-30]], f32), 0.0, None),
            (ref, np.array([[0, 0, 0]], f32), float(np.nextafter(0.5, 0)), -1))


@functools.lru_cache(maxsize=None)
def mesh(F, seed=21):
    """(verts [V, 3] float32 in [-8, 8], faces [F, 3] int32): random
    triangles; from 257 faces on also zero-area faces (a repeated index, three
    collinear vertices), one index out of range and one face a millionth of
    the largest in area."""
    rng = np.random.default_rng(seed + F)
    V = max(3, min(F + 2, 400))
    verts = rng.uniform(-8, 8, (V, 3)).astype(f32)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32)
    if F == 2:
        faces[1] = (faces[0, 0], faces[0, 0], faces[0, 1])          # zero area
    if F >= 257:
        faces[5] = (1, 1, 2)
        faces[6, 2] = V + 4                                          # out of range
        faces[7, 0] = -1
        verts[:3] = [[0, 0, 0], [1, 0, 0], [2, 0, 0]]                # collinear
        faces[8] = (0, 1, 2)
        area, _ = R.face_areas(verts, faces)
        big = int(area.argmax())
        a, b, c = (verts[i].astype(np.float64) for i in faces[big])
        verts = np.concatenate([verts, np.stack([a, a + (b - a) * 1e-3, a + (c - a) * 1e-3])
                                .astype(f32), np.array([[np.inf, 0, 0]], f32)])
        faces[9] = (V, V + 1, V + 2)                                 # 1e-6 of the largest
        faces[10] = (V + 3, 3, 4)                                    # a non-finite area
    return verts, faces


N_BAD = 3          # faces 6, 7 and 10 of the meshes of 257 faces and more
TINY_FACE = 9


SAMPLE_F = (1, 2, 257, 5000)
SAMPLE_S = (1, 64, 65, 10000)
SEED = 0x0123456789ABCDEF


@functools.lru_cache(maxsize=None)
def want_sample(F, S):
    return R.sample_mesh(*mesh(F), S, SEED)


# ---------------------------------------------------- CPU: the reference --
def test_oracle_cases_worked_by_hand():
    lat = _lattice(2, 1.0)
    idx, dist = R.nearest(np.array([[0.5, 0.5, 0.5]], f32), lat)
    assert idx[0] == 0 and dist[0] == f32(math.sqrt(0.75))          # an 8-way tie
    ref = np.array([[1, 1, 1], [2, 0, 0], [1, 1, 1]], f32)
    assert R.nearest(np.array([[1, 1, 0.9]], f32), ref)[0][0] == 0  # the lower duplicate
    ref = np.array([[np.nan, 0, 0], [5, 5, 5]], f32)
    idx, dist = R.nearest(np.array([[0, 0, 0], [np.nan, 0, 0]], f32), ref)
    assert idx.tolist() == [1, -1] and dist[0] == f32(math.sqrt(75.0)) and np.isinf(dist[1])
    assert R.dropped(ref) == 1
    idx, dist = R.nearest(np.zeros((2, 3), f32), np.zeros((0, 3), f32))
    assert idx.tolist() == [-1, -1] and np.isinf(dist).all()
    for ref, q, md, idx_want in max_dist_cases():
        got = R.nearest(q, ref, md)[0]
        assert got.tolist() == ([0, -1] if idx_want is None else [idx_want]), (md, got)


def test_inputs_cover_the_cases():
    c = cases()
    idx, dist = want("lattice_0.25")
    ref, q = c["lattice_0.25"][:2]
    assert (idx[:216] == [0, 1, 2, 3, 4, 5, 6] + list(range(7, 216))).all()  # duplicates lose
    assert (dist[:216] == 0).all()
    centre = slice(216, 216 + 125)
    assert (dist[centre] == f32(math.sqrt(3 * 0.125 ** 2))).all()           # exact 8-way ties
    x = np.arange(5)
    want_idx = (x[:, None, None] * 36 + x[None, :, None] * 6 + x[None, None, :]).reshape(-1)
    assert (idx[centre] == want_idx).all()                                   # the lowest corner
    assert (idx[-4:] == -1).all() and (idx[:-4] >= 0).all() and not (idx >= 216).any()
    md = want("max_dist")[0]
    assert (md[:216] >= 0).all() and (md[centre] == -1).all() and 0 < (md[341:541] >= 0).sum() < 200


# ------------------------------------------- CPU: the arithmetic, host build
@functools.lru_cache(maxsize=None)
def _host_exe():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    import atexit
    import tempfile
    d = tempfile.mkdtemp(prefix="nn_search_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "nn_search_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(REPO, "splatt3r-slam_amd", "csrc"),
                    "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "native", "nn_search_host.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _exe():
    exe = _host_exe()
    if exe is None:
        pytest.skip("hipcc not available")
    return exe


def _host_nn(ref, q, grid, max_dist):
    exe = _exe()
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "nn_in.bin"), os.path.join(d, "nn_out.bin")
    n, m = len(ref), len(q)
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(ref, f32).tobytes())
        f.write(np.ascontiguousarray(q, f32).tobytes())
    origin, cell, dims = grid
    subprocess.run([exe, "nn", fin, fout, str(n), str(m)] + [repr(float(v)) for v in origin] +
                   [repr(float(cell))] + [str(v) for v in dims] + [repr(float(max_dist))],
                   check=True, timeout=300)
    raw = open(fout, "rb").read()
    o = 0
    take = lambda dt, k: np.frombuffer(raw, dt, k, o)
    idx = take(np.int32, m); o += 4 * m
    dist = take(f32, m); o += 4 * m
    dropped = int(take(np.int64, 1)[0]); o += 8
    vc = take(np.int64, m); o += 8 * m
    vr = take(np.int64, m); o += 8 * m
    rings = take(np.int32, m); o += 4 * m
    linear = take(np.int32, m)
    return dict(idx=idx, dist=dist, dropped=dropped, cells=vc, rows=vr, rings=rings, linear=linear)


def _same(got_idx, got_dist, name_or_want, label, parity=None):
    w_idx, w_dist = want(name_or_want) if isinstance(name_or_want, str) else name_or_want
    bad = np.nonzero(np.asarray(got_idx) != w_idx)[0]
    if parity is not None:       # rows whose index or distance bits differ; exact: 0
        parity(label, err=float(len(bad) + (bits(got_dist) != bits(w_dist)).sum()), tol=0.0)
    assert len(bad) == 0, (label, bad[:10], np.asarray(got_idx)[bad[:10]], w_idx[bad[:10]])
    assert np.array_equal(bits(got_dist), bits(w_dist)), label


@pytest.mark.parametrize("name", sorted(cases()))
def test_host_search_vs_brute_force(name, parity):
    ref, q, grid, max_dist = cases()[name]
    got = _host_nn(ref, q, grid, max_dist)
    _same(got["idx"], got["dist"], name, f"host.{name}")
    parity(f"host.{name}", err=float((got["idx"] != want(name)[0]).sum()), tol=0.0)
    assert got["dropped"] == R.dropped(ref)
    cells = grid[2][0] * grid[2][1] * grid[2][2]
    kept = len(ref) - got["dropped"]
    # bounded work: no cell and no row twice
    assert (got["cells"] <= cells).all() and (got["rows"] <= kept).all(), name
    print(name, "rings max", got["rings"].max(), "linear", int(got["linear"].sum()), "of", len(q),
          "cells max", got["cells"].max())
    if name == "clusters":      # both the long ring walk and the linear rest are exercised
        assert got["linear"].sum() >= 20 and ((got["linear"] == 0) & (got["rings"] >= 3)).any()
        assert (got["linear"] == 0).sum() >= 20
    if name == "tiny_cell":
        assert got["linear"].sum() >= 32


@pytest.mark.parametrize("n", (1, 2, 65, 257, 2049))
def test_host_search_sizes_and_grid_independence(n, parity):
    ref, q = cloud(n, 3), cloud(n, 4)
    for grid in (((0.0, 0.0, 0.0), 0.25, (4, 4, 4)), ((-1.0, -2.0, 0.5), 0.07, (9, 31, 5)),
                 ((0.0, 0.0, 0.0), 1.0 / 3.0, (3, 3, 3))):
        got = _host_nn(ref, q, grid, np.inf)
        _same(got["idx"], got["dist"], want_sizes(n), f"host.n{n}.{grid[1]}", parity)
    got = _host_nn(np.zeros((0, 3), f32), q[:5], ((0.0, 0.0, 0.0), 1.0, (2, 2, 2)), np.inf)
    assert (got["idx"] == -1).all() and np.isinf(got["dist"]).all()


def test_host_max_dist_edges(parity):
    for ref, q, md, idx_want in max_dist_cases():
        got = _host_nn(ref, q, ((0.0, 0.0, 0.0), 0.3, (5, 5, 5)), md)
        _same(got["idx"], got["dist"], R.nearest(q, ref, md), f"host.max_dist{md}", parity)


def _host_sample(verts, faces, S, seed):
    exe = _exe()
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "s_in.bin"), os.path.join(d, "s_out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(verts, f32).tobytes())
        f.write(np.ascontiguousarray(faces, np.int32).tobytes())
    subprocess.run([exe, "sample", fin, fout, str(len(verts)), str(len(faces)), str(S), str(seed)],
                   check=True, timeout=300)
    raw = open(fout, "rb").read()
    bad, total = int(np.frombuffer(raw, np.int64, 1)[0]), int(np.frombuffer(raw, np.uint64, 1, 8)[0])
    if total == 0:
        return dict(bad=bad, total=0, points=None, face=None)
    return dict(bad=bad, total=total, points=np.frombuffer(raw, f32, 3 * S, 16).reshape(S, 3),
                face=np.frombuffer(raw, np.int32, S, 16 + 12 * S))


def _same_sample(got, w, label, parity=None):
    if parity is not None:       # samples whose face or point bits differ; exact: 0
        parity(label, err=float((np.asarray(got["face"]) != w["face"]).sum()
                                + (bits(got["points"]) != bits(w["points"])).any(1).sum()), tol=0.0)
    assert got["bad"] == w["bad"] and got["total"] == w["total"], (label, got["bad"], got["total"])
    assert np.array_equal(np.asarray(got["face"]), w["face"]), label
    assert np.array_equal(bits(got["points"]), bits(w["points"])), label


@pytest.mark.parametrize("F", SAMPLE_F)
def test_host_sampler_vs_float64(F, parity):
    for S in SAMPLE_S:
        _same_sample(_host_sample(*mesh(F), S, SEED), want_sample(F, S), f"host.F{F}.S{S}", parity)
    if F >= 257:
        w = want_sample(F, 10000)
        assert w["bad"] == N_BAD and (w["face"] == TINY_FACE).sum() <= 2
        big = float(w["w"].max())
        assert 0.5e-6 < float(w["w"][TINY_FACE]) / big < 2e-6 and big == 2.0 ** 32
    got = _host_sample(mesh(2)[0], np.array([[0, 0, 1], [2, 2, 2]], np.int32), 10, 1)
    assert got["total"] == 0 and got["bad"] == 0


@pytest.mark.parametrize("F", SAMPLE_F)
def test_sampler_counts_and_barycentrics(F, parity):
    verts, faces = mesh(F)
    worst, worst_lam = 0.0, -1.0
    for S in SAMPLE_S:
        w = want_sample(F, S)
        n_f = np.bincount(w["face"], minlength=F).astype(np.float64)
        expect = S * w["w"].astype(np.float64) / float(w["total"])
        worst = max(worst, float(np.abs(n_f - expect).max()))
        assert not n_f[w["w"] == 0].any()
        got = _host_sample(verts, faces, S, SEED)
        lam = R.barycentric(got["points"], verts, faces, got["face"])
        # the float32 rounding of the point: 2^-20, every sample
        off = float(max((-lam).max(), (lam - 1.0).max()))
        worst_lam = max(worst_lam, off)
        print(f"F {F} S {S}: barycentric coordinates leave [0, 1] by at most {off:.3e}")
        assert (lam >= -2.0 ** -20).all() and (lam <= 1 + 2.0 ** -20).all(), (F, S, off)
    parity(f"sampler.F{F}.barycentric", err=worst_lam, tol=2.0 ** -20)
    parity(f"sampler.F{F}.count_bound", err=worst, tol=2.0)
    print(f"F {F}: worst |n_f - S w_f / Q| = {worst:.3f}")
    assert worst <= 2.0


# ------------------------------------------------------------ CPU: the ABI --
def test_abi_rejects_bad_arguments_before_any_device_work():
    """Status 1 with a message; the pointers are never dereferenced (they are
    not device memory here)."""
    from splatt3r_amd import _lib
    from splatt3r_amd import nn  # noqa: F401  (registers the signatures)
    lib = _lib.lib()
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad_org = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)

    def build(n=5, origin=org, cell=0.5, dims=(4, 4, 4), ref=0x1000, grid=0x100000, gb=1 << 20,
              dropped=0x2000):
        return lib.s3k_grid_build(ref, n, origin, cell, *dims, grid, gb, dropped, None)
    for kw, msg in ((dict(n=-1), b"n < 0"), (dict(n=1 << 31), b"too large"),
                    (dict(origin=bad_org), b"origin"), (dict(origin=None), b"origin"),
                    (dict(cell=0.0), b"cell"), (dict(cell=-1.0), b"cell"),
                    (dict(cell=float("inf")), b"cell"), (dict(cell=float("nan")), b"cell"),
                    (dict(dims=(0, 4, 4)), b"dimension"), (dict(dims=(1024, 1024, 129)), b"2^27"),
                    (dict(dims=(1 << 30, 1 << 30, 4)), b"2^27"), (dict(dropped=None), b"counter"),
                    (dict(ref=None), b"null ref"), (dict(gb=64), b"too small"),
                    (dict(grid=None), b"too small"), (dict(grid=0x100010), b"aligned"),
                    (dict(ref=0x100000), b"overlaps")):
        assert build(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    assert lib.s3k_grid_workspace_bytes(5, 1024, 1024, 129) == 0
    assert lib.s3k_grid_workspace_bytes(5, 1024, 1024, 128) >= 4 * (1 << 27) + 5 * 16
    assert lib.s3k_grid_workspace_bytes(-1, 4, 4, 4) == 0
    top = (1 << 31) - 2048                               # the largest row count, as s3k.h says
    assert lib.s3k_grid_workspace_bytes(top, 4, 4, 4) > 0
    assert lib.s3k_grid_workspace_bytes(top + 1, 4, 4, 4) == 0
    assert lib.s3k_query_workspace_bytes(top) > 0 and lib.s3k_query_workspace_bytes(top + 1) == 0
    assert lib.s3k_sample_workspace_bytes(top) > 0 and lib.s3k_sample_workspace_bytes(top + 1) == 0

    def query(n=5, m=3, cell=0.5, dims=(4, 4, 4), grid=0x100000, gb=1 << 20, q=0x1000, md=1.0,
              idx=0x2000, dist=0x3000, ws=0x200000, wb=1 << 20):
        return lib.s3k_query(grid, gb, n, org, cell, *dims, q, m, md, idx, dist, ws, wb, None)
    for kw, msg in ((dict(m=-1), b"m < 0"), (dict(cell=0.0), b"cell"), (dict(md=-1.0), b"max_dist"),
                    (dict(md=float("nan")), b"max_dist"), (dict(dims=(1024, 1024, 129)), b"2^27"),
                    (dict(gb=64), b"grid workspace too small"), (dict(q=None), b"null"),
                    (dict(idx=None), b"null"), (dict(wb=64), b"workspace too small"),
                    (dict(ws=None), b"workspace too small"), (dict(ws=0x100000), b"overlaps"),
                    (dict(q=0x100100), b"overlaps the grid or"), (dict(idx=0x200100), b"overlaps"),
                    (dict(dist=0x1000), b"overlap each other"), (dict(idx=0x1020), b"each other")):
        assert query(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    assert query(m=0, q=None, idx=None, dist=None, ws=None, wb=0) == 0
    assert lib.s3_last_error() == b""
    assert lib.s3k_query_workspace_bytes(0) == 0 and lib.s3k_query_workspace_bytes(3000) >= 48000

    stats = lambda m=5, d=0x1000, thr=0.1, out=0x2000, ws=0x3000, wb=4096: \
        lib.s3k_dist_stats(d, m, thr, out, ws, wb, None)
    for kw, msg in ((dict(m=-1), b"m < 0"), (dict(thr=float("nan")), b"NaN"),
                    (dict(out=None), b"null output"), (dict(d=None), b"null dist"),
                    (dict(wb=8), b"too small")):
        assert stats(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    assert stats(m=(1 << 42)) == 1 and b"too large" in lib.s3_last_error()
    assert lib.s3k_dist_stats_workspace_bytes(2049) == 2 * 5 * 8
    assert lib.s3k_dist_stats_workspace_bytes(1 << 42) == 0

    def sample(V=4, F=2, S=3, verts=0x1000, faces=0x2000, pts=0x3000, face=0x4000, bad=0x5000,
               total=0x5008, ws=0x100000, wb=1 << 20):
        return lib.s3k_sample_mesh(verts, V, faces, F, S, 0, pts, face, bad, total, ws, wb, None)
    for kw, msg in ((dict(F=-1), b"negative"), (dict(S=-1), b"negative"),
                    (dict(F=1 << 31), b"too many faces"), (dict(bad=None), b"counter"),
                    # rejected before any device work: these never touch bad / total either
                    (dict(faces=None), b"null mesh"), (dict(pts=None), b"null output"),
                    (dict(wb=64), b"too small"), (dict(ws=0x100010), b"aligned")):
        assert sample(**kw) == 1 and msg in lib.s3_last_error(), (kw, lib.s3_last_error())
    assert lib.s3k_sample_workspace_bytes(0) == 0 and lib.s3k_sample_workspace_bytes(100) >= 1600
    assert query(m=0, q=None, idx=None, dist=None, ws=None, wb=0) == 0      # clears the message
    assert lib.s3_last_error() == b""


def test_python_validation_needs_no_gpu():
    from splatt3r_amd import nn
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    with pytest.raises(TypeError):
        nn.PointGrid(z(4, 3, dt=torch.float64))
    with pytest.raises(ValueError):
        nn.PointGrid(z(4, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        nn.PointGrid(z(4, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        nn.dist_stats(z(4), 0.1)
    with pytest.raises(TypeError):
        nn.dist_stats(z(4, dt=torch.float64), 0.1)
    with pytest.raises(ValueError):
        nn.dist_stats(z(4, 1), 0.1)
    with pytest.raises(ValueError):
        nn.dist_stats(z(4), float("nan"))
    with pytest.raises(TypeError):
        nn.sample_mesh(z(4, 3), z(2, 3, dt=torch.int64), 5)
    with pytest.raises(RuntimeError, match="GPU only"):
        nn.sample_mesh(z(4, 3), z(2, 3, dt=torch.int32), 5)
    # the default grid (host arithmetic on a host tensor)
    pts = torch.from_numpy(np.concatenate([cloud(1000), [[np.nan, 0, 0]]]).astype(f32))
    origin, cell, dims = nn.default_grid(pts)
    lo, hi = (cloud(1000).astype(np.float64).min(0), cloud(1000).astype(np.float64).max(0))
    assert origin == tuple(float(v) for v in lo)
    assert abs(cell - 2.0 * (float(np.prod(hi - lo)) / 1000) ** (1 / 3)) < 1e-12
    assert all(d == math.floor((h - l) / cell) + 1 for d, l, h in zip(dims, lo, hi))
    _, cell2, dims2 = nn.default_grid(pts, cell=1e-4, max_cells=1000)
    ratio = cell2 / 1e-4
    assert dims2[0] * dims2[1] * dims2[2] <= 1000 and ratio == 2.0 ** round(math.log2(ratio))
    assert nn.default_grid(torch.zeros(0, 3)) == ((0.0, 0.0, 0.0), 1.0, (1, 1, 1))
    assert nn.default_grid(torch.ones(5, 3))[2] == (1, 1, 1)
    # a near-FLT_MAX extent over a tiny cell: the cell doubles until the dims fit
    wide = torch.tensor([[-3e38, 0, 0], [3e38, 1, 1]], dtype=torch.float32)
    _, cell3, dims3 = nn.default_grid(wide, cell=1e-300, max_cells=4096)
    assert dims3[0] * dims3[1] * dims3[2] <= 4096 and dims3[0] > 1 and math.isfinite(cell3)
    with pytest.raises(ValueError):
        nn.default_grid(pts, cell=0.0)
    with pytest.raises(ValueError):
        nn.default_grid(pts, max_cells=(1 << 27) + 1)


# --------------------------------------------------------------------- GPU --
def _cuda(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _gpu_nn(ref, q, grid=None, max_dist=np.inf):
    from splatt3r_amd.nn import PointGrid
    kw = {} if grid is None else dict(origin=grid[0], cell=grid[1], dims=grid[2])
    g = PointGrid(_cuda(ref, f32), **kw)
    idx, dist = g.query(_cuda(q, f32), max_dist)
    return idx.cpu().numpy(), dist.cpu().numpy(), int(g.dropped)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_hip_nearest_sizes(n, parity):
    idx, dist, dropped = _gpu_nn(cloud(n, 3), cloud(n, 4))
    _same(idx, dist, want_sizes(n), f"hip.n{n}")
    parity(f"hip.n{n}", err=float((idx != want_sizes(n)[0]).sum()), tol=0.0)
    assert dropped == 0


@pytest.mark.gpu
def test_hip_nearest_empty_sets():
    idx, dist, dropped = _gpu_nn(np.zeros((0, 3), f32), cloud(5))
    assert (idx == -1).all() and np.isinf(dist).all() and dropped == 0
    idx, dist, _ = _gpu_nn(cloud(5), np.zeros((0, 3), f32))
    assert idx.shape == (0,) and dist.shape == (0,)
    idx, dist, dropped = _gpu_nn(np.full((3, 3), np.nan, f32), cloud(5))
    assert (idx == -1).all() and np.isinf(dist).all() and dropped == 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cases()))
def test_hip_nearest_adversarial(name, parity):
    ref, q, grid, max_dist = cases()[name]
    idx, dist, dropped = _gpu_nn(ref, q, grid, max_dist)
    _same(idx, dist, name, f"hip.{name}")
    parity(f"hip.{name}", err=float((idx != want(name)[0]).sum()), tol=0.0)
    assert dropped == R.dropped(ref)
    # the default grid gives the same
    idx, dist, _ = _gpu_nn(ref, q, None, max_dist)
    _same(idx, dist, name, f"hip.{name}.default_grid", parity)


@pytest.mark.gpu
def test_hip_max_dist_edges(parity):
    for ref, q, md, _ in max_dist_cases():
        for grid in (None, ((0.0, 0.0, 0.0), 0.3, (5, 5, 5))):
            idx, dist, _ = _gpu_nn(ref, q, grid, md)
            _same(idx, dist, R.nearest(q, ref, md), f"hip.max_dist{md}.{grid is None}", parity)


@pytest.mark.gpu
def test_hip_nearest_independence_and_reproducibility(parity):
    from splatt3r_amd.nn import PointGrid, nearest
    ref, q = cases()["lattice_third"][:2]
    ref = np.concatenate([ref, cloud(3000) * 2])
    q = np.concatenate([q, cloud(3000, 9) * 2.2 - 0.1])
    w = R.nearest(q, ref)
    r_d, q_d = _cuda(ref), _cuda(q)
    outs = []
    for kw in (dict(), dict(cell=0.05), dict(origin=(-3.0, 0.1, 0.7), cell=1.0 / 3.0,
                                             dims=(7, 5, 11))):
        g = PointGrid(r_d, **kw)
        a, b = g.query(q_d), g.query(q_d)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32),
                                                       b[1].view(torch.int32))
        _same(a[0].cpu().numpy(), a[1].cpu().numpy(), w, f"hip.grid{sorted(kw)}", parity)
        outs.append(a)
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(q))).cuda()
    idx_p, dist_p = nearest(q_d[perm].contiguous(), r_d)
    assert torch.equal(idx_p, outs[0][0][perm])
    assert torch.equal(dist_p.view(torch.int32), outs[0][1][perm].view(torch.int32))
    assert np.array_equal(bits(r_d.cpu().numpy()), bits(ref))     # inputs left as they were


@pytest.mark.gpu
def test_hip_query_modes_give_the_same_bits(parity):
    """Unsorted order and one wave per query (nn.set_query_mode, kept for the
    benchmark) change no bit: long ring walks, the linear rest, ties, max_dist."""
    from splatt3r_amd import nn
    try:
        for mode in ("unsorted", "wave", "sorted"):
            nn.set_query_mode(mode)
            for name in ("clusters", "lattice_0.25", "tiny_cell", "max_dist", "one_cell"):
                ref, q, grid, max_dist = cases()[name]
                idx, dist, _ = _gpu_nn(ref, q, grid, max_dist)
                _same(idx, dist, name, f"hip.{mode}.{name}", parity)
            idx, dist, _ = _gpu_nn(cloud(8000, 3), cloud(8000, 4))
            _same(idx, dist, want_sizes(8000), f"hip.{mode}.n8000", parity)
    finally:
        nn.set_query_mode("sorted")


@pytest.mark.gpu
@pytest.mark.parametrize("m", (0, 1, 2047, 2048, 2049, 50000))
def test_hip_dist_stats(m, parity):
    from splatt3r_amd.nn import dist_stats
    rng = np.random.default_rng(m)
    d = np.exp(rng.uniform(np.log(1e-4), np.log(10.0), m)).astype(f32)
    if m > 10:
        d[3], d[7], d[m - 1] = np.inf, np.nan, np.inf
        d[5] = f32(0.05)                                  # exactly on the threshold
    thr = float(f32(0.05))
    t = _cuda(d, f32)
    a, b = dist_stats(t, thr), dist_stats(t, thr)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    got, w = a.cpu().numpy(), R.stats(d, thr)
    assert got[0] == w[0] and got[3] == w[3] and got[4] == w[4], (got, w)
    for k in (1, 2):
        err = abs(got[k] - w[k]) / w[k] if w[k] else abs(got[k])
        parity(f"hip.stats.m{m}.{STAT[k]}", err=err, tol=max(m, 1) * 2.0 ** -52)
        print(f"m {m} {STAT[k]}: rel err {err:.3e} tol {max(m, 1) * 2.0 ** -52:.1e}")
        assert err <= max(m, 1) * 2.0 ** -52
    # and bit for bit the sums taken in the order s3k.h fixes
    assert np.array_equal(got.view(np.int64),
                          np.array(R.stats_in_order(d, thr), np.float64).view(np.int64)), got


def test_oracle_restatements_agree():
    """The prefiltered search is the brute-force one; the ordered sums are the
    exactly rounded ones to m 2^-52."""
    rng = np.random.default_rng(8)
    ref = np.concatenate([cloud(3000), cloud(3000)[:40], _lattice(6, 0.25)])
    q = np.concatenate([cloud(2000, 5), cloud(3000)[:100],
                        (_lattice(5, 0.25).astype(np.float64) + 0.125).astype(f32)])
    a, b = R.nearest(q, ref), R.nearest_prefiltered(q, ref)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    d = np.exp(rng.uniform(-9, 2, 5000)).astype(f32)
    d[[4, 99]] = np.inf, np.nan
    s, t = R.stats(d, 0.05), R.stats_in_order(d, 0.05)
    assert s[0] == t[0] == 4998 and s[3] == t[3] and s[4] == t[4]
    assert abs(s[1] - t[1]) <= 5000 * 2.0 ** -52 * s[1] and abs(s[2] - t[2]) <= 5000 * 2.0 ** -52 * s[2]


STAT = ("count", "sum", "sum_sq", "within", "max")


@pytest.mark.gpu
@pytest.mark.parametrize("F", SAMPLE_F)
def test_hip_sampler_vs_float64(F, parity):
    from splatt3r_amd.nn import sample_mesh
    verts, faces = mesh(F)
    v, f = _cuda(verts, f32), _cuda(faces, np.int32)
    for S in SAMPLE_S:
        pts, face, bad, total = sample_mesh(v, f, S, SEED, counters=True)
        got = dict(points=pts.cpu().numpy(), face=face.cpu().numpy(), bad=bad, total=total)
        _same_sample(got, want_sample(F, S), f"hip.F{F}.S{S}", parity)
        again = sample_mesh(v, f, S, SEED)
        assert torch.equal(again[0].view(torch.int32), pts.view(torch.int32))
        assert torch.equal(again[1], face)
    other = sample_mesh(v, f, 64, SEED + 1)[0]
    assert not torch.equal(other, sample_mesh(v, f, 64, SEED)[0])
    assert torch.equal(v.cpu(), torch.from_numpy(verts))


@pytest.mark.gpu
def test_hip_sampler_without_area_raises():
    from splatt3r_amd.nn import sample_mesh
    v = _cuda(mesh(2)[0], f32)
    with pytest.raises(ValueError, match="no area"):
        sample_mesh(v, _cuda(np.array([[0, 0, 1], [2, 2, 9]], np.int32)), 10)
    with pytest.raises(ValueError, match="no area"):
        sample_mesh(v, torch.zeros(0, 3, dtype=torch.int32, device="cuda"), 10)
    pts, face = sample_mesh(v, _cuda(np.array([[0, 1, 2]], np.int32)), 0)
    assert pts.shape == (0, 3) and face.shape == (0,)


@pytest.mark.gpu
def test_hip_bad_input_raises_and_sets_the_error():
    from splatt3r_amd import _lib
    from splatt3r_amd.nn import PointGrid, dist_stats, sample_mesh
    lib = _lib.lib()
    ref = _cuda(cloud(100), f32)
    with pytest.raises(TypeError):
        PointGrid(ref.double())
    with pytest.raises(ValueError):
        PointGrid(ref.reshape(-1))
    with pytest.raises(RuntimeError, match="GPU only"):
        PointGrid(ref.cpu())
    g = PointGrid(ref)
    with pytest.raises(TypeError):
        g.query(ref.half())
    with pytest.raises(ValueError):
        g.query(ref[:, :2])
    with pytest.raises(RuntimeError, match="GPU only"):
        g.query(ref.cpu())
    with pytest.raises(ValueError):
        g.query(ref, max_dist=-1.0)
    with pytest.raises(ValueError):
        PointGrid(ref, cell=0.0)
    # through the ABI: status 1 and a message
    for kw, msg in ((dict(cell=0.0), "cell"), (dict(cell=-2.0), "cell"),
                    (dict(cell=0.5, dims=(1024, 1024, 129)), "2^27")):
        kw.setdefault("dims", (2, 2, 2))
        with pytest.raises(RuntimeError, match=msg.replace("^", r"\^")):
            PointGrid(ref, origin=(0.0, 0.0, 0.0), **kw)
        assert msg.encode() in lib.s3_last_error()
    org = (ctypes.c_double * 3)(*g.origin)
    small = torch.empty(256, device="cuda", dtype=torch.uint8)
    drop = torch.zeros(1, device="cuda", dtype=torch.int64)
    assert lib.s3k_grid_build(ref.data_ptr(), 100, org, g.cell, *g.dims, small.data_ptr(), 256,
                              drop.data_ptr(), _lib.stream(ref.device)) == 1
    assert b"too small" in lib.s3_last_error()
    idx = torch.empty(100, device="cuda", dtype=torch.int32)
    dist = torch.empty(100, device="cuda", dtype=torch.float32)
    assert lib.s3k_query(g._grid.data_ptr(), g._grid.numel(), 100, org, g.cell, *g.dims,
                         ref.data_ptr(), 100, math.inf, idx.data_ptr(), dist.data_ptr(),
                         small.data_ptr(), 256, _lib.stream(ref.device)) == 1
    assert b"workspace too small" in lib.s3_last_error()
    with pytest.raises(TypeError):
        dist_stats(dist.double(), 0.1)
    with pytest.raises(TypeError):
        sample_mesh(ref, torch.zeros(2, 3, device="cuda", dtype=torch.int64), 4)
    # and the library still works
    _same(*[t.cpu().numpy() for t in g.query(ref)], R.nearest(cloud(100), cloud(100)), "after")
