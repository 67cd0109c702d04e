"""TSDF fusion and marching-tetrahedra extraction (include/s3f.h,
csrc/tsdf_mesh.hip, splatt3r_amd.mesh, SharedGaussians.extract_mesh,
Frontend.save_mesh) against the numpy float64 restatement
tests/tsdf_mesh_ref64.py.

Tolerances (derived, not measured).
  integrate   both sides round the state to float32 after every view and each
              update is a convex combination, so they differ by at most one
              float32 ulp per view: V * 2^-23, absolute on tsdf and colour
              (both within [-1, 1]), relative on weight.  A voxel is left out
              when one of its float64 decisions (z > 0, pixel rounding and
              with it in-image, sdf = -trunc) lies within 1e-9 of its
              boundary; at most 0.1 % of a case's voxel-view pairs may be
              (test_integrate_cases_stay_under_the_fragile_cap checks the
              reference alone, on the CPU).
  extraction  counts and faces exact; a vertex is computed in double and
              rounded once: one float32 ulp of the largest coordinate
              magnitude, 2^-23 on colours in [0, 1].
"""
import functools
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import tsdf_mesh_ref64 as R
from conftest import REPO

ULP = 2.0 ** -23
VOXEL = 0.05


def ulp32_of(x):
    """The float32 ulp at magnitude x."""
    return float(np.spacing(np.float32(abs(x))))


# ------------------------------------------------------- integrate: cases ---
DIMS = [(2, 2, 2), (5, 7, 9), (33, 17, 9), (64, 64, 3), (1, 5, 5)]
IMAGES = [(8, 6), (64, 48)]                      # (W, H)
VIEWS = [1, 3, 5]
SCALES = [0.5, 1.0, 2.3]
MATRIX = list(itertools.product(range(len(DIMS)), range(len(IMAGES)), VIEWS, SCALES))
EXTRAS = {
    "offcentre": dict(offcentre=True),
    "bad_depth": dict(bad_depth=True),
    "weight_zeros": dict(wzeros=True),
    "w_max_clamps": dict(V=5, w_max=3.0),
    "view_behind": dict(behind=True),
    "invalid_pose": dict(invalid=True),
    "no_color_no_wmap": dict(color=False, wmap=False),
}


def _look_at(rng, dist):
    """Camera-to-world rotation (columns: the camera's x, y, z axes in the
    world) and position of a camera `dist` from the origin looking at it."""
    z = rng.normal(size=3)
    z /= np.linalg.norm(z)
    up = rng.normal(size=3)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], 1), -z * dist


@functools.lru_cache(maxsize=None)
def make_case(dims=(5, 7, 9), img=(8, 6), V=3, s=1.0, seed=0, offcentre=False, bad_depth=False,
              wzeros=False, w_max=64.0, behind=False, invalid=False, color=True, wmap=True):
    """A volume with a random non-fresh state centred on the world origin, V
    cameras around it looking inwards, per-pixel random depths through the
    volume; the volume overfills the image, so some voxels project outside."""
    rng = np.random.default_rng(seed)
    W, H = img
    nx, ny, nz = dims
    half = VOXEL * max(dims) / 2
    origin = (-VOXEL * (np.array(dims) - 1) / 2 + rng.uniform(-0.01, 0.01, 3)).astype(np.float32)
    tsdf0 = rng.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    weight0 = (rng.uniform(0, 2, (nz, ny, nx)) * (rng.uniform(size=(nz, ny, nx)) > 0.3)).astype(
        np.float32)
    rgb0 = rng.uniform(0, 1, (3, nz, ny, nx)).astype(np.float32)
    dist = 1.2 + 2 * half
    Ks, Ts, depths = [], [], []
    for v in range(V):
        Rm, pos = _look_at(rng, dist)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = s * Rm, pos + rng.uniform(-0.05, 0.05, 3)
        if behind and v == 0:
            T[:3, :3] = -T[:3, :3] @ np.diag([1.0, -1.0, 1.0])     # looks away, still a rotation
        f = 0.35 * W * dist / half
        K = np.array([[f, 0, (W - 1) / 2 + (3.3 if offcentre else 0)],
                      [0, f * 1.1, (H - 1) / 2 - (2.7 if offcentre else 0)], [0, 0, 1]])
        depths.append((dist + rng.uniform(-1.5 * half, 1.5 * half, (H, W))) / s)
        Ks.append(K)
        Ts.append(T)
    K, T, depth = (np.array(a, np.float32) for a in (Ks, Ts, depths))
    if invalid:
        T[V // 2, 1, 2] = np.nan
        if V >= 3:
            T[0, :3, 0] = 0          # s = 0
        if V >= 5:
            K[4, 0, 0] = -1.0
    if bad_depth:
        bad = rng.uniform(size=depth.shape) < 0.2
        vals = np.resize(np.array([0, -1, np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
        depth[bad] = vals
    col = rng.uniform(0, 1, (V, 3, H, W)).astype(np.float32) if color else None
    wm = None
    if wmap:
        wm = rng.uniform(0.5, 2, (V, H, W)).astype(np.float32)
        if wzeros:
            z = rng.uniform(size=wm.shape)
            wm[z < 0.3] = 0
            wm[(z > 0.3) & (z < 0.33)] = np.nan
            wm[(z > 0.33) & (z < 0.36)] = -1
    c = dict(dims=dims, H=H, W=W, V=V, origin=origin, voxel=np.float32(VOXEL),
             trunc=np.float32(4 * VOXEL), w_max=np.float32(w_max), tsdf0=tsdf0, weight0=weight0,
             rgb0=rgb0, K=K, T=T, depth=depth, color=col, wmap=wm)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def matrix_case(di, ii, V, s):
    return make_case(DIMS[di], IMAGES[ii], V, s, seed=1000 * di + 100 * ii + 10 * V + int(s * 2))


def extra_case(name):
    kw = dict(dims=(33, 17, 9), img=(64, 48), V=5, s=2.3, seed=77 + sorted(EXTRAS).index(name))
    kw.update(EXTRAS[name])
    return make_case(**kw)


@functools.lru_cache(maxsize=None)
def _ref_cached(key):
    kind, arg = key
    c = matrix_case(*arg) if kind == "m" else extra_case(arg)
    return c, ref_integrate(c)


def ref_integrate(c, views=None):
    sl = slice(None) if views is None else views
    opt = lambda a: None if a is None else a[sl]
    return R.integrate(c["tsdf0"], c["weight0"], c["rgb0"], c["origin"], c["voxel"], c["trunc"],
                       c["w_max"], c["depth"][sl], c["K"][sl], c["T"][sl], opt(c["color"]),
                       opt(c["wmap"]))


def check_integrate(c, ref, got, parity=None, key=None):
    """got: dict tsdf, weight, rgb (numpy float32) against the reference."""
    V = c["V"]
    assert ref["fragile_pairs"] <= 1e-3 * ref["pairs"], (ref["fragile_pairs"], ref["pairs"])
    keep = ~ref["fragile"]
    tol = V * ULP
    ef = float(np.abs(got["tsdf"].astype(np.float64) - ref["tsdf"])[keep].max(initial=0))
    ec = float(np.abs(got["rgb"].astype(np.float64) - ref["rgb"])[:, keep].max(initial=0))
    wr = ref["weight"].astype(np.float64)
    ew = float((np.abs(got["weight"] - wr) / np.maximum(wr, 1e-30))[keep & (wr > 0)].max(initial=0))
    if parity is not None:
        parity(key + "_tsdf", err=ef, tol=tol)
        parity(key + "_rgb", err=ec, tol=tol)
        parity(key + "_weight", err=ew, tol=tol, left_out=float(ref["fragile"].sum()))
    assert ef <= tol and ec <= tol and ew <= tol, (ef, ec, ew, tol)
    assert (got["weight"][keep & (wr == 0)] == 0).all()
    # a voxel no view updates keeps its bits
    still = keep & ~ref["updated"]
    for name, src in (("tsdf", c["tsdf0"]), ("weight", c["weight0"])):
        assert np.array_equal(got[name][still].view(np.uint32), src[still].view(np.uint32)), name
    assert np.array_equal(got["rgb"][:, still].view(np.uint32), c["rgb0"][:, still].view(np.uint32))
    if c["color"] is None:
        assert np.array_equal(got["rgb"].view(np.uint32), c["rgb0"].view(np.uint32))


# ------------------------------------------------------ extraction: cases ---
def _grid(dims):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return i.astype(np.float64), j.astype(np.float64), k.astype(np.float64)


def _volume(dims, dist, seed=0, origin=(0.0, 0.0, 0.0), voxel=1.0):
    """A volume from a signed-distance array in voxels, truncated at 4."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    tsdf = np.clip(dist / 4.0, -1, 1).astype(np.float32)
    return dict(dims=dims, tsdf=tsdf, weight=np.ones_like(tsdf),
                rgb=rng.uniform(0, 1, (3, nz, ny, nx)).astype(np.float32),
                origin=np.array(origin, np.float32), voxel=np.float32(voxel), w_min=0.5)


def sphere_volume(dims=(20, 20, 20), c=(9.37, 9.61, 9.13), r=6.3, **kw):
    i, j, k = _grid(dims)
    return _volume(dims, np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - r, **kw)


def torus_volume(dims=(24, 24, 12), c=(11.4, 11.6, 5.45), major=7.3, minor=3.1):
    i, j, k = _grid(dims)
    ring = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2) - major
    return _volume(dims, np.sqrt(ring ** 2 + (k - c[2]) ** 2) - minor, seed=1)


def plane_volume(dims=(65, 33, 9)):
    i, j, k = _grid(dims)
    n = np.array([0.3, 0.5, 0.81])
    n /= np.linalg.norm(n)
    return _volume(dims, (i - 32.2) * n[0] + (j - 16.1) * n[1] + (k - 4.3) * n[2], seed=2,
                   origin=(-1.5, 0.25, 3.0), voxel=0.0371)


def hole_volume():
    v = sphere_volume(seed=3)
    v["weight"][8:12, 8:12, 2:6] = 0          # a block across the surface at low x
    return v


def outside_volume():
    v = sphere_volume(seed=4)
    v["tsdf"][:] = 1.0
    return v


MESH_CASES = {
    "sphere20": sphere_volume,
    "torus": torus_volume,
    "plane": plane_volume,
    "hole": hole_volume,
    "all_outside": outside_volume,
    # 125 lattice points: one workgroup of every kernel, counts below 256
    "small": lambda: sphere_volume((5, 5, 5), (2.1, 2.2, 1.9), 1.4, seed=5),
    # 274,625 lattice points = 1,073 workgroups: the scan of the workgroup
    # sums takes a second round of its 1,024 threads, and both counts exceed
    # what one workgroup scans
    "sphere65": lambda: sphere_volume((65, 65, 65), (31.37, 32.61, 30.13), 20.3, seed=6,
                                      origin=(2.0, -3.0, 0.5), voxel=0.013),
    "thin": lambda: sphere_volume((1, 5, 5), (0.0, 2.2, 1.9), 1.4, seed=7),
}


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    v = MESH_CASES[name]()
    return v, R.extract(v["tsdf"], v["weight"], v["rgb"], v["origin"], v["voxel"], v["w_min"])


def check_mesh(v, ref, verts, cols, faces, parity=None, key=None):
    assert (len(verts), len(faces)) == (len(ref["verts"]), len(ref["faces"]))
    if len(verts) == 0:
        return
    tol = ulp32_of(np.abs(ref["verts64"]).max())
    ev = float(np.abs(verts.astype(np.float64) - ref["verts64"]).max())
    ec = float(np.abs(cols.astype(np.float64) - ref["cols64"]).max())
    if parity is not None:
        parity(key + "_verts", err=ev, tol=tol, nv=len(verts), nt=len(faces))
        parity(key + "_cols", err=ec, tol=ULP)
    assert ev <= tol and ec <= ULP, (ev, tol, ec)
    assert np.array_equal(R.canonical_faces(faces), R.canonical_faces(ref["faces"]))


# ------------------------------------------------------ CPU: ref64 by hand ---
def test_ref64_integrate_by_hand():
    """2 x 2 x 2 voxels at x, y in {0, 1}, z in {1, 2}; one 2 x 2 view at the
    origin with fx = fy = 1, cx = cy = 0: voxel (x, y, z) lands on pixel
    (floor(x / z + 0.5), floor(y / z + 0.5)), dyadic everything."""
    K = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float32)
    T = np.eye(4, dtype=np.float32)[None]
    depth = np.array([[[1.5, 2.5], [0.0, 1.25]]], np.float32)       # [b, a]
    color = np.stack([depth[0] / 4, depth[0] / 8, depth[0] * 0], 0)[None].astype(np.float32)
    out = R.integrate(*R.fresh((2, 2, 2)), (0, 0, 1), 1.0, 1.0, 10.0, depth, K, T, color=color)
    want = np.array([[[0.5, 1.0], [1.0, 0.25]], [[-0.5, 0.5], [1.0, -0.75]]])   # [z, y, x]
    seen = np.array([[[1, 1], [0, 1]], [[1, 1], [0, 1]]], bool)
    assert (out["tsdf"] == want).all() and (out["weight"] == seen).all()
    assert (out["updated"] == seen).all()
    assert out["rgb"][0, 0, 0, 0] == 0.375 and out["rgb"][1, 1, 1, 1] == 1.25 / 8
    assert (out["rgb"][:, ~seen] == 0).all()
    # the same view again with weight 3 and the depth 0.25 further: the running mean
    out2 = R.integrate(out["tsdf"], out["weight"], out["rgb"], (0, 0, 1), 1.0, 1.0, 3.0,
                       depth + np.float32(0.25), K, T, wmap=np.full((1, 2, 2), 3, np.float32))
    assert out2["tsdf"][0, 0, 0] == (0.5 * 1 + 0.75 * 3) / 4
    assert out2["weight"][0, 0, 0] == 3.0            # min(1 + 3, w_max = 3)
    # the hole has d = 0.25 now: sdf = -0.75 on a fresh voxel
    assert out2["tsdf"][0, 1, 0] == -0.75 and out2["weight"][0, 1, 0] == 3.0
    assert (out2["rgb"] == out["rgb"]).all()          # no colour given
    # trunc 0.5: sdf = -0.75 is skipped, sdf = -0.5 is kept
    out3 = R.integrate(*R.fresh((2, 2, 2)), (0, 0, 1), 1.0, 0.5, 10.0, depth, K, T)
    assert out3["weight"][1, 1, 1] == 0 and out3["tsdf"][1, 1, 1] == 1
    assert out3["weight"][1, 0, 0] == 1 and out3["tsdf"][1, 0, 0] == -1
    # a similarity of scale 2 about the origin: camera units are half the world's
    T2 = T.copy()
    T2[0, :3, :3] *= 2
    out4 = R.integrate(*R.fresh((2, 2, 2)), (0, 0, 1), 1.0, 1.0, 10.0, depth / 2, K, T2)
    assert (out4["tsdf"] == want).all()


def test_ref64_mesh_by_hand():
    """One cell, corner 000 inside: all 6 Kuhn tetrahedra hold it, so 6
    triangles fan around it over the 7 edges the corner owns, every normal
    pointing away from it."""
    tsdf = np.full((2, 2, 2), 0.5, np.float32)
    tsdf[0, 0, 0] = -0.5
    w = np.ones_like(tsdf)
    rgb = np.zeros((3, 2, 2, 2), np.float32)
    rgb[0, 0, 0, 0] = 1.0
    m = R.extract(tsdf, w, rgb, (1, 2, 3), 2.0, 0.5)
    assert m["edge_ids"].tolist() == list(range(7))
    assert (m["verts64"] == np.array([1, 2, 3]) + 2.0 * 0.5 * R.DIRS).all()
    assert (m["cols64"] == [0.5, 0, 0]).all()
    assert len(m["faces"]) == 6
    a, b, c = (m["verts64"][m["faces"][:, k]] for k in range(3))
    assert (np.cross(b - a, c - a) @ np.ones(3) > 0).all()
    st = R.mesh_stats(m["verts64"], m["faces"])
    assert st["oriented"] and st["boundary_edges"] == 6
    # corner 111 outside, the rest inside: the mirror image
    m2 = R.extract(-tsdf[::-1, ::-1, ::-1], w, rgb, (0, 0, 0), 1.0, 0.5)
    a, b, c = (m2["verts64"][m2["faces"][:, k]] for k in range(3))
    assert len(m2["faces"]) == 6 and (np.cross(b - a, c - a) @ np.ones(3) > 0).all()
    # two inside corners along x: quads, still consistently oriented
    tsdf[0, 0, 1] = -0.25
    st = R.mesh_stats(*[R.extract(tsdf, w, rgb, (0, 0, 0), 1.0, 0.5)[k] for k in ("verts64", "faces")])
    assert st["oriented"] and st["nf"] == 8
    # weight below w_min on one corner: no valid cell, no mesh
    w[1, 1, 1] = 0.25
    assert len(R.extract(tsdf, w, rgb, (0, 0, 0), 1.0, 0.5)["faces"]) == 0


def test_sphere_and_torus_extraction(parity):
    v, m = mesh_case("sphere20")
    assert float(np.abs(v["tsdf"]).min()) > 0            # no exact zeros
    st = R.mesh_stats(m["verts64"], m["faces"])
    assert (st["nv"], st["nf"], st["ne"]) == (2232, 4460, 6690)
    assert st["closed"] and st["oriented"] and st["euler"] == 2
    vol, area = 4 / 3 * math.pi * 6.3 ** 3, 4 * math.pi * 6.3 ** 2
    # the restatement's own distance to the analytic values (an inscribed
    # polyhedron of a sampled distance field): 1.26 % and 0.65 % low
    parity("mesh_sphere20_volume", err=abs(st["volume"] - vol) / vol, tol=0.013)
    parity("mesh_sphere20_area", err=abs(st["area"] - area) / area, tol=0.007)
    assert 0 < vol - st["volume"] < 0.013 * vol and 0 < area - st["area"] < 0.007 * area
    _, mt = mesh_case("torus")
    st = R.mesh_stats(mt["verts64"], mt["faces"])
    assert st["closed"] and st["oriented"] and st["euler"] == 0 and st["volume"] > 0
    _, mh = mesh_case("hole")
    st = R.mesh_stats(mh["verts64"], mh["faces"])
    assert st["oriented"] and not st["closed"] and st["boundary_edges"] > 0
    _, mp = mesh_case("plane")
    st = R.mesh_stats(mp["verts64"], mp["faces"])
    assert st["oriented"] and st["boundary_edges"] > 0 and st["euler"] == 1
    assert len(mesh_case("all_outside")[1]["faces"]) == 0
    assert len(mesh_case("thin")[1]["faces"]) == 0
    small = mesh_case("small")[1]
    assert 0 < len(small["verts"]) < 256 and 0 < len(small["faces"]) < 256
    big = mesh_case("sphere65")[1]
    assert len(big["verts"]) > 1024 and len(big["faces"]) > 1024


def _float32_size_bound(ref):
    """How far volume and area can move when every vertex coordinate moves by
    at most one float32 ulp of the largest coordinate: |dV| <= area * |d|,
    |dA| <= (sum of perimeters) * |d|, |d| = sqrt(3) ulp."""
    d = math.sqrt(3) * ulp32_of(np.abs(ref["verts64"]).max())
    a, b, c = (ref["verts64"][ref["faces"][:, k]] for k in range(3))
    perim = (np.linalg.norm(b - a, axis=1) + np.linalg.norm(c - b, axis=1)
             + np.linalg.norm(a - c, axis=1)).sum()
    st = R.mesh_stats(ref["verts64"], ref["faces"])
    return st, st["area"] * d, perim * d


def check_mesh_properties(name, verts, faces, parity=None, key=None):
    """The case-table-free properties of a mesh of case `name`."""
    ref = mesh_case(name)[1]
    want, dv, da = _float32_size_bound(ref)
    st = R.mesh_stats(verts, faces)
    for k in ("nv", "ne", "nf", "euler", "closed", "oriented", "boundary_edges"):
        assert st[k] == want[k], (k, st[k], want[k])
    assert st["oriented"]
    if parity is not None:
        parity(key + "_volume", err=abs(st["volume"] - want["volume"]), tol=dv)
        parity(key + "_area", err=abs(st["area"] - want["area"]), tol=da)
    assert abs(st["volume"] - want["volume"]) <= dv and abs(st["area"] - want["area"]) <= da


# ------------------------------------------- CPU: the arithmetic, host build
@functools.lru_cache(maxsize=None)
def _host_exe():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    import atexit
    import tempfile
    d = tempfile.mkdtemp(prefix="tsdf_mesh_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "tsdf_mesh_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(REPO, "splatt3r-slam_amd", "csrc"),
                    "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "native", "tsdf_mesh_host.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _host_files():
    exe = _host_exe()
    if exe is None:
        pytest.skip("hipcc not available")
    d = os.path.dirname(exe)
    return exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")


def _host_integrate(c):
    exe, fin, fout = _host_files()
    nx, ny, nz = c["dims"]
    n = nx * ny * nz
    with open(fin, "wb") as f:
        f.write(np.array([*c["origin"], c["voxel"], c["trunc"], c["w_max"]], np.float32).tobytes())
        for a in (c["tsdf0"], c["weight0"], c["rgb0"], c["depth"], c["color"], c["wmap"], c["K"],
                  c["T"]):
            if a is not None:
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
    subprocess.run([exe, "integrate", fin, fout, str(nx), str(ny), str(nz), str(c["V"]),
                    str(c["H"]), str(c["W"]), str(int(c["color"] is not None)),
                    str(int(c["wmap"] is not None))], check=True, timeout=60)
    raw = np.fromfile(fout, np.float32)
    assert raw.size == 5 * n
    return dict(tsdf=raw[:n].reshape(nz, ny, nx), weight=raw[n:2 * n].reshape(nz, ny, nx),
                rgb=raw[2 * n:].reshape(3, nz, ny, nx))


def _host_mesh(v):
    exe, fin, fout = _host_files()
    nx, ny, nz = v["dims"]
    with open(fin, "wb") as f:
        f.write(np.array([*v["origin"], v["voxel"], v["w_min"]], np.float32).tobytes())
        for a in (v["tsdf"], v["weight"], v["rgb"]):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    subprocess.run([exe, "mesh", fin, fout, str(nx), str(ny), str(nz)], check=True, timeout=60)
    raw = open(fout, "rb").read()
    nv, nt = (int(x) for x in np.frombuffer(raw, np.int64, 2))
    o = 16
    verts = np.frombuffer(raw, np.float32, nv * 3, o).reshape(nv, 3)
    cols = np.frombuffer(raw, np.float32, nv * 3, o + nv * 12).reshape(nv, 3)
    faces = np.frombuffer(raw, np.int32, nt * 3, o + nv * 24).reshape(nt, 3)
    return verts, cols, faces


HOST_INTEGRATE = [("m", (1, 0, 3, 2.3)), ("m", (2, 1, 5, 0.5)), ("m", (4, 0, 1, 1.0)),
                  ("m", (0, 0, 3, 1.0))] + [("x", k) for k in sorted(EXTRAS)]


@pytest.mark.parametrize("key", HOST_INTEGRATE, ids=lambda k: str(k[1]).replace(" ", ""))
def test_host_integrate_matches_ref64(key, parity):
    c, ref = _ref_cached(key)
    check_integrate(c, ref, _host_integrate(c), parity, f"tsdf_host_{key[1]}")


@pytest.mark.parametrize("name", sorted(MESH_CASES))
def test_host_mesh_matches_ref64(name, parity):
    v, ref = mesh_case(name)
    verts, cols, faces = _host_mesh(v)
    check_mesh(v, ref, verts, cols, faces, parity, f"mesh_host_{name}")
    if len(faces):
        check_mesh_properties(name, verts, faces, parity, f"mesh_host_{name}")


def test_integrate_cases_stay_under_the_fragile_cap(parity):
    """Every GPU integrate case, reference alone: at most 0.1 % of the
    voxel-view pairs within 1e-9 of a decision boundary, and the cases do
    exercise every branch."""
    worst = 0.0
    seen_skip = seen_clamp = False
    for key in [("m", m) for m in MATRIX] + [("x", k) for k in sorted(EXTRAS)]:
        c, ref = _ref_cached(key)
        worst = max(worst, ref["fragile_pairs"] / ref["pairs"])
        assert ref["fragile_pairs"] <= 1e-3 * ref["pairs"], key
        if c["V"] > 1 or min(c["dims"]) > 1:
            seen_skip |= bool((~ref["updated"]).any()) and bool(ref["updated"].any())
        seen_clamp |= bool((ref["weight"] == c["w_max"]).any())
    parity("tsdf_fragile_share", err=worst, tol=1e-3)
    assert seen_skip and seen_clamp
    c, ref = _ref_cached(("x", "view_behind"))
    assert not ref_integrate(c, slice(0, 1))["updated"].any()
    c, ref = _ref_cached(("x", "invalid_pose"))
    for v in (0, 2, 4):
        assert not ref_integrate(c, slice(v, v + 1))["updated"].any()
    assert ref["updated"].any()


# ------------------------------------------------------------ CPU: mesh ply
def test_mesh_ply_round_trip(tmp_path):
    from splatt3r_amd.evaluate import read_mesh_ply, write_mesh_ply
    _, m = mesh_case("small")
    cols = np.clip(m["cols"], 0, 1)
    p = tmp_path / "m.ply"
    write_mesh_ply(p, m["verts"], cols, m["faces"])
    raw = p.read_bytes()
    head = raw[:raw.index(b"end_header\n")].decode()
    assert "format binary_little_endian 1.0" in head
    assert f"element vertex {len(m['verts'])}" in head and f"element face {len(m['faces'])}" in head
    assert "property list uchar int vertex_indices" in head
    assert len(raw) == len(head) + len("end_header\n") + 15 * len(m["verts"]) + 13 * len(m["faces"])
    v, c, f = read_mesh_ply(p)
    assert np.array_equal(v.view(np.uint32), m["verts"].view(np.uint32))
    assert np.array_equal(c, np.rint(cols * 255).astype(np.uint8))
    assert f.dtype == np.int32 and np.array_equal(f, m["faces"])
    # no triangles, and nothing at all
    for nv in (3, 0):
        write_mesh_ply(p, m["verts"][:nv], cols[:nv], np.zeros((0, 3), np.int32))
        v, c, f = read_mesh_ply(p)
        assert v.shape == (nv, 3) and c.shape == (nv, 3) and f.shape == (0, 3)
    # properties are found by name: another order and an extra one
    nv = 4
    rec = np.zeros(nv, dtype=[("red", "u1"), ("q", "<f8"), ("z", "<f4"), ("y", "<f4"),
                              ("x", "<f4"), ("blue", "u1"), ("green", "u1")])
    rec["x"], rec["y"], rec["z"], rec["green"] = [0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], 9
    frec = np.zeros(1, dtype=[("n", "u1"), ("v", "<u4", (3,))])
    frec["n"], frec["v"] = 3, [[0, 2, 3]]
    with open(p, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\ncomment x\nelement vertex 4\n"
                  "property uchar red\nproperty double q\nproperty float z\nproperty float y\n"
                  "property float x\nproperty uchar blue\nproperty uchar green\nelement face 1\n"
                  "property list uchar uint vertex_index\nend_header\n").encode())
        fh.write(rec.tobytes() + frec.tobytes())
    v, c, f = read_mesh_ply(p)
    assert v[:, 0].tolist() == [0, 1, 2, 3] and v[:, 2].tolist() == [8, 9, 10, 11]
    assert c[:, 1].tolist() == [9] * 4 and f.tolist() == [[0, 2, 3]]
    with pytest.raises(ValueError):
        write_mesh_ply(p, m["verts"][:3], cols[:3], np.array([[0, 1, 3]]))
    p.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        read_mesh_ply(p)


# ------------------------------------------------- CPU: the argument errors
def test_abi_rejects_bad_arguments_before_device_work():
    """Every check returns S3_ERR_INVALID without touching a pointer: called
    here with null and dummy pointers and no GPU."""
    from splatt3r_amd import _lib
    lib = _lib.lib()
    big = 1 << 20
    assert lib.s3f_integrate_workspace_bytes(0) == 0
    assert lib.s3f_integrate_workspace_bytes(3) == 3 * 20 * 8
    assert lib.s3f_mesh_workspace_bytes(big, big, big) == 0
    assert lib.s3f_mesh_workspace_bytes(0, 4, 4) == 0
    n = 8 * 8 * 8
    assert lib.s3f_mesh_workspace_bytes(8, 8, 8) == 2 * n + 4 * n + 8 * 2
    # 7 nx ny nz >= 2^31: (2^31 / 7 rounded up) voxels in a column
    edge = -(-2 ** 31 // 7)
    assert lib.s3f_mesh_workspace_bytes(edge, 1, 1) == 0
    assert lib.s3f_mesh_workspace_bytes(edge - 1, 1, 1) > 0
    integ = lambda nx, ny, nz, V=1, ws=8, nbytes=1 << 30, voxel=0.1, trunc=0.4, wmax=1.0: \
        lib.s3f_integrate(8, 8, 8, nx, ny, nz, 0.0, 0.0, 0.0, voxel, trunc, wmax, 8, None, None,
                          8, 8, V, 4, 4, ws, nbytes, None)
    for args, word in (((big, big, big), b"2^31"), ((edge, 1, 1), b"2^31"), ((0, 2, 2), b"dims"),
                       ((2, 2, 2, 0), b"n_views"), ((2, 2, 2, 1, 8, 159), b"workspace"),
                       ((2, 2, 2, 1, None), b"workspace"),
                       ((2, 2, 2, 1, 8, 1 << 30, 0.0), b"voxel"),
                       ((2, 2, 2, 1, 8, 1 << 30, 0.1, float("nan")), b"trunc"),
                       ((2, 2, 2, 1, 8, 1 << 30, 0.1, 0.4, -1.0), b"w_max")):
        assert integ(*args) == 1, args
        assert word in lib.s3_last_error(), (args, lib.s3_last_error())
    count = lambda nx, ny, nz, w_min=0.5, ws=8, nbytes=1 << 40: \
        lib.s3f_mesh_count(8, 8, nx, ny, nz, w_min, 8, ws, nbytes, None)
    for args, word in (((big, big, big), b"2^31"), ((edge, 1, 1), b"2^31"),
                       ((2, 2, -1), b"dims"), ((8, 8, 8, 0.0), b"w_min"),
                       ((8, 8, 8, 0.5, 8, 6 * 512 + 15), b"workspace")):
        assert count(*args) == 1, args
        assert word in lib.s3_last_error(), (args, lib.s3_last_error())
    emit = lambda nx, ny, nz, nv=10, nt=10, vcap=10, fcap=10, nbytes=1 << 40: \
        lib.s3f_mesh_emit(8, 8, nx, ny, nz, 0.0, 0.0, 0.0, 0.1, nv, nt, 8, 8, 8, vcap, fcap, 8,
                          nbytes, None)
    for args, word in (((big, big, big), b"2^31"), ((8, 8, 8, 10, 10, 9, 10), b"verts capacity"),
                       ((8, 8, 8, 10, 10, 10, 9), b"faces capacity"),
                       ((8, 8, 8, -1), b"counts"), ((8, 8, 8, 7 * 512 + 1, 10, 1 << 20), b"counts"),
                       ((8, 8, 8, 10, 10, 10, 10, 100), b"workspace")):
        assert emit(*args) == 1, args
        assert word in lib.s3_last_error(), (args, lib.s3_last_error())
    # an empty mesh is not an error, launches nothing and clears the message
    assert emit(8, 8, 8, 0, 0, 0, 0) == 0
    assert lib.s3_last_error() == b""


def test_grid_for_bounds_and_its_errors():
    from splatt3r_amd.mesh import ABI_MAX_VOXELS, grid_for_bounds
    origin, dims = grid_for_bounds((-1, 0, 2), (1, 0.5, 2), 0.25)
    assert origin == (-1.0, 0.0, 2.0) and dims == (9, 3, 1)
    assert 7 * ABI_MAX_VOXELS < 2 ** 31 <= 7 * (ABI_MAX_VOXELS + 1)
    with pytest.raises(ValueError) as e:
        grid_for_bounds((0, 0, 0), (10, 10, 10), 0.001)
    msg = str(e.value)
    assert "10001 x 10001 x 10001" in msg and str(10001 ** 3) in msg and "smallest voxel" in msg
    fit = float(msg.rsplit(" ", 1)[1])
    assert math.prod(grid_for_bounds((0, 0, 0), (10, 10, 10), fit * 1.001)[1]) <= ABI_MAX_VOXELS
    with pytest.raises(ValueError):
        grid_for_bounds((0, 0, 0), (10, 10, 10), fit * 0.99)
    with pytest.raises(ValueError) as e:
        grid_for_bounds((0, 0, 0), (1, 1, 1), 0.1, max_voxels=1000)
    assert "1331 voxels" in str(e.value) and "1000" in str(e.value)
    assert grid_for_bounds((0, 0, 0), (1, 1, 1), 0.1, max_voxels=1331)[1] == (11, 11, 11)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            grid_for_bounds((0, 0, 0), (1, 1, 1), bad)


# -------------------------------------------------------------------- GPU ---
def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_volume(c):
    from splatt3r_amd.mesh import TSDFVolume
    vol = TSDFVolume(dims=c["dims"], voxel=float(c["voxel"]), origin=tuple(c["origin"]),
                     trunc=float(c["trunc"]), w_max=float(c["w_max"]), device="cuda")
    assert (vol.voxel, vol.trunc, vol.w_max) == (float(c["voxel"]), float(c["trunc"]),
                                                 float(c["w_max"]))
    vol.tsdf.copy_(_t(c["tsdf0"]))
    vol.weight.copy_(_t(c["weight0"]))
    vol.rgb.copy_(_t(c["rgb0"]))
    return vol


def _gpu_integrate(c, vol=None, one_by_one=False):
    vol = vol or _gpu_volume(c)
    dev = [_t(c[k]) for k in ("depth", "T", "K", "color", "wmap")]
    if one_by_one:
        for v in range(c["V"]):
            d, T, K, col, wm = (None if a is None else a[v] for a in dev)
            vol.integrate(d, T, K, color=col, weight=wm)
    else:
        d, T, K, col, wm = dev
        vol.integrate(d, T, K, color=col, weight=wm)
    return vol


def _host_state(vol):
    return dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(),
                rgb=vol.rgb.cpu().numpy())


def _same_state(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
               for k in ("tsdf", "weight", "rgb"))


@pytest.mark.gpu
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("V", VIEWS)
@pytest.mark.parametrize("ii", range(len(IMAGES)), ids=lambda i: "%dx%d" % IMAGES[i])
@pytest.mark.parametrize("di", range(len(DIMS)), ids=lambda i: "%dx%dx%d" % DIMS[i])
def test_hip_integrate_matches_ref64(di, ii, V, s, parity):
    c, ref = _ref_cached(("m", (di, ii, V, s)))
    got = _host_state(_gpu_integrate(c))
    check_integrate(c, ref, got, parity, f"tsdf_{di}_{ii}_V{V}_s{s}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EXTRAS))
def test_hip_integrate_further_cases(name, parity):
    c, ref = _ref_cached(("x", name))
    got = _host_state(_gpu_integrate(c))
    check_integrate(c, ref, got, parity, f"tsdf_{name}")
    if name == "w_max_clamps":
        assert (got["weight"] <= 3.0).all() and (got["weight"] == 3.0).any()


@pytest.mark.gpu
def test_hip_integrate_is_pure():
    """A batch equals its views one by one, a second run equals the first,
    voxels no view sees keep their bits (check_integrate), and a second,
    unrelated volume integrated on another stream changes nothing."""
    import torch
    c, ref = _ref_cached(("x", "bad_depth"))
    got = _host_state(_gpu_integrate(c))
    check_integrate(c, ref, got)
    assert ref["updated"].any() and not ref["updated"].all()
    assert _same_state(_host_state(_gpu_integrate(c, one_by_one=True)), got)
    assert _same_state(_host_state(_gpu_integrate(c)), got)
    for key in (("m", (0, 0, 5, 2.3)), ("m", (3, 1, 5, 0.5))):
        cc, _ = _ref_cached(key)
        assert _same_state(_host_state(_gpu_integrate(cc, one_by_one=True)),
                           _host_state(_gpu_integrate(cc)))
    other, _ = _ref_cached(("m", (3, 1, 5, 1.0)))
    vol_a, vol_b = _gpu_volume(c), _gpu_volume(other)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(sb):
            _gpu_integrate(other, vol=vol_b)
    with torch.cuda.stream(sa):
        _gpu_integrate(c, vol=vol_a)
    with torch.cuda.stream(sb):
        _gpu_integrate(other, vol=vol_b)
    sa.synchronize()
    sb.synchronize()
    assert _same_state(_host_state(vol_a), got)
    # reset() gives a fresh volume
    vol_a.reset()
    st = _host_state(vol_a)
    assert (st["tsdf"] == 1).all() and not st["weight"].any() and not st["rgb"].any()


def _gpu_extract(v):
    from splatt3r_amd.mesh import TSDFVolume
    vol = TSDFVolume(dims=v["dims"], voxel=float(v["voxel"]), origin=tuple(v["origin"]),
                     device="cuda")
    vol.tsdf.copy_(_t(v["tsdf"]))
    vol.weight.copy_(_t(v["weight"]))
    vol.rgb.copy_(_t(v["rgb"]))
    before = _host_state(vol)
    verts, cols, faces = vol.extract(w_min=v["w_min"])
    assert _same_state(_host_state(vol), before)
    return verts.cpu().numpy(), cols.cpu().numpy(), faces.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MESH_CASES))
def test_hip_mesh_matches_ref64(name, parity):
    v, ref = mesh_case(name)
    verts, cols, faces = _gpu_extract(v)
    assert verts.dtype == np.float32 and faces.dtype == np.int32
    check_mesh(v, ref, verts, cols, faces, parity, f"mesh_{name}")
    if len(faces):
        check_mesh_properties(name, verts, faces, parity, f"mesh_{name}")
        again = _gpu_extract(v)
        assert all(np.array_equal(a, b) for a, b in zip(again, (verts, cols, faces)))


@pytest.mark.gpu
def test_hip_mesh_rejects_huge_dims_and_small_outputs():
    """The 2^31 rejection with no matching allocation (it must return before
    touching memory) and the capacity checks, on the device."""
    import torch
    from splatt3r_amd import _lib
    lib = _lib.lib()
    small = torch.zeros(64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    big = 1 << 20
    assert lib.s3f_mesh_count(small.data_ptr(), small.data_ptr(), big, big, big, 0.5,
                              counts.data_ptr(), small.data_ptr(), 256, None) == 1
    assert b"2^31" in lib.s3_last_error()
    assert lib.s3f_integrate(small.data_ptr(), small.data_ptr(), small.data_ptr(), 2048, 2048,
                             2048, 0.0, 0.0, 0.0, 0.1, 0.4, 1.0, small.data_ptr(), None, None,
                             small.data_ptr(), small.data_ptr(), 1, 4, 4, small.data_ptr(), 256,
                             None) == 1
    assert b"2^31" in lib.s3_last_error()
    v, ref = mesh_case("small")
    nv, nt = len(ref["verts"]), len(ref["faces"])
    from splatt3r_amd.mesh import TSDFVolume
    vol = TSDFVolume(dims=v["dims"], voxel=1.0, device="cuda")
    vol.tsdf.copy_(_t(v["tsdf"]))
    vol.weight.copy_(_t(v["weight"]))
    need = lib.s3f_mesh_workspace_bytes(*v["dims"])
    ws = torch.zeros((need + 7) // 8, dtype=torch.int64, device="cuda")
    assert lib.s3f_mesh_count(vol.tsdf.data_ptr(), vol.weight.data_ptr(), *v["dims"], 0.5,
                              counts.data_ptr(), ws.data_ptr(), need, None) == 0
    assert counts.tolist() == [nv, nt]
    out_v = torch.full((nv, 3), -7.0, device="cuda")
    out_f = torch.full((nt, 3), -7, dtype=torch.int32, device="cuda")
    emit = lambda vcap, fcap, nbytes: lib.s3f_mesh_emit(
        vol.tsdf.data_ptr(), None, *v["dims"], 0.0, 0.0, 0.0, 1.0, nv, nt, out_v.data_ptr(), None,
        out_f.data_ptr(), vcap, fcap, ws.data_ptr(), nbytes, None)
    assert emit(nv - 1, nt, need) == 1 and emit(nv, nt - 1, need) == 1
    assert emit(nv, nt, need - 1) == 1
    torch.cuda.synchronize()
    assert (out_v == -7).all() and (out_f == -7).all()
    assert emit(nv, nt, need) == 0
    assert np.array_equal(R.canonical_faces(out_f.cpu().numpy()), R.canonical_faces(ref["faces"]))


# --------------------------------- GPU: geometry through the public class ---
SPHERE_R, SPHERE_VOX = 0.5, 0.04
SPHERE_ORIGIN = tuple(-SPHERE_VOX * 31 / 2 + d for d in (0.003, 0.007, 0.001))
SPHERE_BACKGROUND = 4.0
# The float64 restatement's own radial error on these inputs (6 views of 64 x
# 48 fused into 32^3 voxels of 0.04 with nearest-pixel depth: one voxel, at
# the limbs), measured on the CPU; test_sphere_fusion_reference pins it.
SPHERE_RADIAL_REF = 0.04025


def _rig_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def sphere_views():
    """Analytic z-depth maps, ray-cast in float64, of a sphere of radius 0.5
    at the world origin in front of a background 4 away (rays that miss the
    sphere carve the free space around it, as a room's walls do), from 6
    cameras about 2 away along the axes of a randomly rotated frame, 64 x 48."""
    rng = np.random.default_rng(0)
    W, H = 64, 48
    f = 55.0
    K = np.array([[f, 0, (W - 1) / 2 + 0.37], [0, f, (H - 1) / 2 - 0.21], [0, 0, 1]], np.float32)
    a, b = np.meshgrid(np.arange(W), np.arange(H))
    rays = np.stack([(a - K[0, 2]) / K[0, 0], (b - K[1, 2]) / K[1, 1], np.ones_like(a, float)], -1)
    Q = _rig_rotation(rng)
    depths, Ts = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            z = np.zeros(3)
            z[axis] = -sign                         # looks at the origin
            x = np.zeros(3)
            x[(axis + 1) % 3] = 1.0
            Rm = Q @ np.stack([x, np.cross(z, x), z], 1)
            pos = -2.0 * Rm[:, 2] + rng.uniform(-0.03, 0.03, 3)
            d = rays @ Rm.T                         # world ray directions, z-component 1 in the camera
            qa = (d * d).sum(-1)
            qb = 2 * (d @ pos)
            qc = pos @ pos - SPHERE_R ** 2
            disc = qb * qb - 4 * qa * qc
            # the ray parameter is the z-depth
            depths.append(np.where(disc > 0, (-qb - np.sqrt(np.maximum(disc, 0))) / (2 * qa),
                                   SPHERE_BACKGROUND))
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = Rm, pos
            Ts.append(T)
    col = np.broadcast_to(np.array([0.2, 0.5, 0.8], np.float32)[None, :, None, None], (6, 3, H, W))
    return (np.array(depths, np.float32), np.array(Ts, np.float32), K,
            np.ascontiguousarray(col))


def _sphere_radial_error(verts):
    return float(np.abs(np.linalg.norm(np.asarray(verts, np.float64), axis=1) - SPHERE_R).max())


@functools.lru_cache(maxsize=None)
def sphere_fusion_ref():
    depth, T, K, col = sphere_views()
    out = R.integrate(*R.fresh((32, 32, 32)), SPHERE_ORIGIN, SPHERE_VOX, 4 * SPHERE_VOX, 64.0,
                      depth, np.broadcast_to(K, (6, 3, 3)), T, color=col)
    m = R.extract(out["tsdf"], out["weight"], out["rgb"], SPHERE_ORIGIN, SPHERE_VOX, 1.0)
    return out, m


def test_sphere_fusion_reference(parity):
    """The restatement end to end: the fused sphere is closed with chi = 2,
    and its radial error is what SPHERE_RADIAL_REF records."""
    out, m = sphere_fusion_ref()
    assert out["fragile_pairs"] <= 1e-3 * out["pairs"]
    st = R.mesh_stats(m["verts64"], m["faces"])
    assert st["closed"] and st["oriented"] and st["euler"] == 2 and st["volume"] > 0
    err = _sphere_radial_error(m["verts64"])
    parity("sphere_fusion_ref_radial", err=err, tol=SPHERE_RADIAL_REF)
    assert err <= SPHERE_RADIAL_REF < 1.05 * err + 1e-6


@pytest.mark.gpu
def test_hip_sphere_fusion_through_the_public_class(parity):
    from splatt3r_amd.mesh import TSDFVolume
    depth, T, K, col = sphere_views()
    ref_out, ref = sphere_fusion_ref()
    vol = TSDFVolume(dims=(32, 32, 32), voxel=SPHERE_VOX, origin=SPHERE_ORIGIN, device="cuda")
    assert vol.trunc == float(np.float32(4 * SPHERE_VOX))
    vol.integrate(_t(depth[:4]), _t(T[:4]), _t(K), color=_t(col[:4]))
    vol.integrate(_t(depth[4]), _t(T[4]), _t(K), color=_t(col[4]))
    vol.integrate(_t(depth[5:]), _t(T[5:]), _t(K)[None], color=_t(col[5:]))
    verts, cols, faces = (a.cpu().numpy() for a in vol.extract())
    st = R.mesh_stats(verts, faces)
    assert st["closed"] and st["oriented"] and st["euler"] == 2 and st["volume"] > 0
    err = _sphere_radial_error(verts)
    tol = SPHERE_RADIAL_REF + math.sqrt(3) * ulp32_of(np.abs(ref["verts64"]).max())
    parity("sphere_fusion_radial", err=err, tol=tol, ref=SPHERE_RADIAL_REF)
    assert err <= tol
    assert np.abs(cols - np.array([0.2, 0.5, 0.8], np.float32)).max() <= 6 * ULP


# ------------------------------------------------- GPU: rasterizer pinhole ---
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(33, 24), (32, 25)])
@pytest.mark.parametrize("centred", [True, False])
def test_rasterizer_pinhole_matches_the_fusion(W, H, centred):
    """One small opaque Gaussian at a known camera-space point: the pixel of
    maximal rendered alpha is the pixel s3f_integrate's rounding selects for
    that point under mesh.rasterizer_intrinsics (a one-voxel volume whose
    colour records the pixel it was updated from)."""
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer
    from splatt3r_amd.mesh import TSDFVolume, rasterizer_intrinsics
    from splatt3r_amd.refine import _cameras
    dev = torch.device("cuda", 0)
    f = 0.9 * W
    K = torch.tensor([[f, 0, W / 2 + (0 if centred else 4.4)],
                      [0, f * 1.07, H / 2 - (0 if centred else 3.1)], [0, 0, 1]])
    T = torch.eye(4)[None]
    settings, s = _cameras(T, K, H, W, 0.1, 1000.0, None, dev)
    K_r = rasterizer_intrinsics(settings[0])
    z = 2.0
    a_idx = torch.arange(W, dtype=torch.float32)[None, :].expand(H, W)
    b_idx = torch.arange(H, dtype=torch.float32)[:, None].expand(H, W)
    code = torch.stack([a_idx / 64, b_idx / 64, torch.zeros(H, W)])[None].to(dev).contiguous()
    for pa, pb in ((W * 0.25 + 0.3, H * 0.6 - 0.3), (W - 2.75, 1.2), (0.3, H - 1.3)):
        x_c = torch.tensor([(pa - float(K_r[0, 2])) / float(K_r[0, 0]) * z,
                            (pb - float(K_r[1, 2])) / float(K_r[1, 1]) * z, z])
        sigma = 0.3 * z / float(K_r[0, 0])           # a third of a pixel
        means = (x_c[None] * s).to(dev)
        cov = torch.tensor([[1.0, 0, 0, 1.0, 0, 1.0]], device=dev) * (sigma * s) ** 2
        out = GaussianRasterizer(settings[0])(
            means3D=means, means2D=torch.zeros_like(means), shs=None,
            colors_precomp=torch.ones(1, 3, device=dev),
            opacities=torch.full((1, 1), 0.99, device=dev), cov3D_precomp=cov, return_depth=True)
        alpha = out[3]
        assert float(alpha.max()) > 0.3
        flat = int(alpha.argmax())
        lit = (flat % W, flat // W)
        vol = TSDFVolume(dims=(1, 1, 1), voxel=1.0, origin=tuple(x_c.tolist()), device=dev)
        vol.integrate(torch.full((1, H, W), z, device=dev), T, K_r, color=code)
        assert float(vol.weight) == 1.0
        chosen = (round(float(vol.rgb[0]) * 64), round(float(vol.rgb[1]) * 64))
        assert chosen == (math.floor(pa + 0.5), math.floor(pb + 0.5))
        assert lit == chosen, (lit, chosen, (pa, pb))


# -------------------------------------------------------- GPU: map level ---
def _plane_map(n=4000, seed=5):
    """Gaussians on the plane z = 2 (world = the first camera's frame)."""
    import torch
    from splatt3r_amd.gaussian_map import SharedGaussians
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1.2, 1.2, (n, 2))
    means = np.concatenate([xy, 2.0 + 0.05 * xy[:, :1]], 1)
    cov = np.tile(np.array([4e-3, 0, 0, 4e-3, 0, 1e-5]), (n, 1))
    colors = np.stack([0.5 + 0.4 * np.sin(3 * xy[:, 0]), 0.5 + 0.4 * np.cos(2 * xy[:, 1]),
                       np.full(n, 0.3)], 1)
    gm = SharedGaussians(max_gaussians=n + 100, device="cuda")
    gm.append(_t(means.astype(np.float32)), _t(cov.astype(np.float32)),
              _t(colors.astype(np.float32)), torch.full((n,), 0.9, device="cuda"), 0)
    return gm


@pytest.mark.gpu
def test_map_extract_mesh_matches_ref64(parity):
    import torch
    from splatt3r_amd.mesh import grid_for_bounds
    gm = _plane_map()
    n = gm.n_gaussians
    assert n == 4000
    H, W, voxel = 48, 64, 0.08
    K = torch.tensor([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]])
    T = torch.eye(4).repeat(3, 1, 1)
    T[1, 0, 3], T[2, 1, 3] = 0.4, -0.3
    T[2, :3, :3] *= 1.5                     # a similarity: camera units 1.5 world units
    fields = (gm.means, gm.cov_triu, gm.colors, gm.opacities, gm.kf_id)
    before = [f.clone() for f in fields]
    verts, cols, faces = gm.extract_mesh(T, K, H, W, voxel, view_batch=2)
    for f, b in zip(fields, before):
        assert torch.equal(f.view(torch.int32), b.view(torch.int32))
    assert gm.n_gaussians == n
    depth, color, K_r = gm.render_depths(T, K, H, W)
    assert (depth > 0).float().mean() > 0.5
    # depth is z in each view's camera units: the plane is 2 world units away
    mid = depth[:, H // 2, W // 2].cpu()
    assert abs(float(mid[0]) - 2.0) < 0.1 and abs(float(mid[2]) - 2.0 / 1.5) < 0.1
    trunc = 4 * voxel
    lo, hi = gm.means[:n].amin(0).tolist(), gm.means[:n].amax(0).tolist()
    origin, dims = grid_for_bounds([v - trunc for v in lo], [v + trunc for v in hi], voxel)
    out = R.integrate(*R.fresh(dims), origin, voxel, trunc, 64.0, depth.cpu().numpy(),
                      K_r.numpy()[None].repeat(3, 0), T.numpy(), color=color.cpu().numpy())
    assert out["fragile_pairs"] == 0, "a rendered depth put a decision on its boundary"
    ref = R.extract(out["tsdf"], out["weight"], out["rgb"], origin, voxel, 1.0)
    verts, cols, faces = verts.cpu().numpy(), cols.cpu().numpy(), faces.cpu().numpy()
    assert len(faces) > 100
    v = dict(origin=origin, voxel=voxel)
    check_mesh(v, ref, verts, cols, faces, parity, "mesh_map_plane")
    assert cols.min() >= 0 and cols.max() <= 1
    assert abs(float(np.median(verts[:, 2])) - 2.0) < voxel
    with pytest.raises(ValueError, match="smallest voxel"):
        gm.extract_mesh(T, K, H, W, voxel, max_voxels=1000)
    assert gm.extract_mesh(T[:0], K, H, W, voxel) is None


@pytest.mark.gpu
def test_frontend_save_mesh(tmp_path):
    import torch
    from splatt3r_amd.evaluate import read_mesh_ply
    from splatt3r_amd.slam import Frontend
    from test_map_reanchor import _model_and_frames
    dev, model, frames = _model_and_frames()
    fe = Frontend(model, device=dev, spatial_stride=4, render=False, viz=True, max_gaussians=20000)
    fe.map_opacity_threshold = 0.1
    try:
        assert fe.save_mesh(tmp_path / "none.ply", 0.1) is None        # no keyframe yet
        for i in range(3):
            fe.step(i, frames[i])
        n = fe.gmap.n_gaussians
        assert n > 0 and len(fe.keyframes) >= 1
        extent = float((fe.gmap.means[:n].amax(0) - fe.gmap.means[:n].amin(0)).max())
        snap = [f.clone() for f in (fe.gmap.means, fe.gmap.cov_triu, fe.gmap.colors,
                                    fe.gmap.opacities, fe.gmap.kf_id)]
        got = fe.save_mesh(tmp_path / "sub" / "mesh.ply", extent / 40, max_voxels=2_000_000)
        assert got is not None
        nv, nt = got
        verts, cols, faces = read_mesh_ply(tmp_path / "sub" / "mesh.ply")
        assert (len(verts), len(faces)) == (nv, nt)
        assert cols is not None and len(cols) == nv
        assert nt == 0 or (faces.min() >= 0 and faces.max() < nv)
        for f, b in zip((fe.gmap.means, fe.gmap.cov_triu, fe.gmap.colors, fe.gmap.opacities,
                         fe.gmap.kf_id), snap):
            assert torch.equal(f, b)
    finally:
        fe.close()
    off = Frontend(model, device=dev, spatial_stride=4, render=False, viz=False)
    try:
        off.step(0, frames[0])
        assert off.save_mesh(tmp_path / "off.ply", 0.1) is None
        assert not (tmp_path / "off.ply").exists()
    finally:
        off.close()
