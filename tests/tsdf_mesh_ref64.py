"""Numpy float64 restatement of include/s3f.h: TSDF fusion of depth maps into a
dense volume and marching-tetrahedra extraction.  Written from the header's
definition, not from the kernels: the triangle orientation is decided
geometrically here (edge midpoints against the inside -> outside direction),
by a determinant of corner offsets there.
"""
import itertools

import numpy as np

DIRS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)])
_DIR_OF = {tuple(d): k for k, d in enumerate(DIRS)}
BOUNDARY_REL = 1e-9


def fresh(dims):
    """(tsdf, weight, rgb) of a fresh volume; dims = (nx, ny, nz)."""
    nx, ny, nz = dims
    return (np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32),
            np.zeros((3, nz, ny, nx), np.float32))


def centres(dims, origin, voxel):
    """[nz, ny, nx, 3] float64 voxel centres from the float32 origin and voxel."""
    nx, ny, nz = dims
    o = np.asarray(origin, np.float32).astype(np.float64)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return o + np.float64(np.float32(voxel)) * np.stack([i, j, k], -1).astype(np.float64)


def view_valid(K, T):
    K = np.asarray(K, np.float32).reshape(3, 3)
    T = np.asarray(T, np.float32).reshape(4, 4)
    vals = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], *T[:3, :4].ravel()], np.float64)
    if not np.isfinite(vals).all() or not (K[0, 0] > 0 and K[1, 1] > 0):
        return False
    s = np.linalg.norm(T[:3, 0].astype(np.float64))
    return bool(np.isfinite(s) and s > 0)


def integrate(tsdf, weight, rgb, origin, voxel, trunc, w_max, depth, K, T_WC, color=None,
              wmap=None):
    """V views into the volume, in index order.  depth [V, H, W], K [V, 3, 3],
    T_WC [V, 4, 4], color [V, 3, H, W] or None, wmap [V, H, W] or None, all
    float32.  Returns a dict: tsdf, weight, rgb (float32, rounded after every
    view), `updated` [nz, ny, nx] (some view updated the voxel), `fragile`
    (some decision of some view lies within BOUNDARY_REL of its boundary),
    `pairs` (voxel-view pairs) and `fragile_pairs`."""
    tsdf, weight, rgb = (np.array(a, np.float32) for a in (tsdf, weight, rgb))
    nz, ny, nx = tsdf.shape
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    K = np.asarray(K, np.float32).reshape(V, 3, 3)
    T_WC = np.asarray(T_WC, np.float32).reshape(V, 4, 4)
    xw = centres((nx, ny, nz), origin, voxel)
    trunc64, wmax64 = np.float64(np.float32(trunc)), np.float64(np.float32(w_max))
    updated = np.zeros(tsdf.shape, bool)
    fragile = np.zeros(tsdf.shape, bool)
    fragile_pairs = 0
    for v in range(V):
        if not view_valid(K[v], T_WC[v]):
            continue
        M = T_WC[v, :3, :3].astype(np.float64)
        t = T_WC[v, :3, 3].astype(np.float64)
        s = np.linalg.norm(M[:, 0])
        fx, fy, cx, cy = (np.float64(K[v, 0, 0]), np.float64(K[v, 1, 1]), np.float64(K[v, 0, 2]),
                          np.float64(K[v, 1, 2]))
        xc = (xw - t) @ M / (s * s)              # M^T (x_w - t) / s^2
        x, y, z = xc[..., 0], xc[..., 1], xc[..., 2]
        scale = np.linalg.norm(xc, axis=-1) + 1e-300
        frag = np.abs(z) < BOUNDARY_REL * scale
        live = z > 0
        with np.errstate(all="ignore"):
            u = fx * x / z + cx
            w_ = fy * y / z + cy
            a, b = np.floor(u + 0.5), np.floor(w_ + 0.5)
            for val in (u, w_):
                fr = (val + 0.5) - np.floor(val + 0.5)
                frag |= live & (np.minimum(fr, 1 - fr) < BOUNDARY_REL * np.maximum(1, np.abs(val)))
            inimg = (a >= 0) & (a <= W - 1) & (b >= 0) & (b <= H - 1)
        live &= inimg
        ai = np.where(live, a, 0).astype(np.int64)
        bi = np.where(live, b, 0).astype(np.int64)
        d = depth[v][bi, ai]
        live &= np.isfinite(d) & (d > 0)
        wo = wmap[v][bi, ai] if wmap is not None else np.ones_like(d)
        live &= np.isfinite(wo) & (wo > 0)
        with np.errstate(all="ignore"):
            sdf = s * (d.astype(np.float64) - z)
            frag |= live & (np.abs(sdf + trunc64) < BOUNDARY_REL * trunc64)
            live &= ~(sdf < -trunc64)
            fo = np.minimum(1.0, sdf / trunc64)
            w64, wo64 = weight.astype(np.float64), wo.astype(np.float64)
            tot = w64 + wo64
            new_f = (tsdf.astype(np.float64) * w64 + fo * wo64) / tot
            tsdf = np.where(live, new_f.astype(np.float32), tsdf)
            if color is not None:
                cv = np.asarray(color, np.float32)[v][:, bi, ai].astype(np.float64)
                new_c = (rgb.astype(np.float64) * w64 + cv * wo64) / tot
                rgb = np.where(live, new_c.astype(np.float32), rgb)
            weight = np.where(live, np.minimum(tot, wmax64).astype(np.float32), weight)
        updated |= live
        fragile |= frag
        fragile_pairs += int(frag.sum())
    return dict(tsdf=tsdf, weight=weight, rgb=rgb, updated=updated, fragile=fragile,
                pairs=V * tsdf.size, fragile_pairs=fragile_pairs)


# ------------------------------------------------------- marching tetrahedra
def kuhn_tetrahedra():
    """The 6 tetrahedra as 4 corner offsets each, permutations in
    lexicographic order."""
    out = []
    for perm in itertools.permutations(range(3)):
        c = np.zeros(3, int)
        path = [c.copy()]
        for ax in perm:
            c[ax] = 1
            path.append(c.copy())
        out.append(path)
    return out


def extract(tsdf, weight, rgb, origin, voxel, w_min):
    """The mesh of a volume.  Returns a dict: verts64, cols64 (float64,
    unrounded), verts, cols (float32), faces [nt, 3] int64, edge_ids [nv]."""
    tsdf = np.asarray(tsdf, np.float32)
    weight = np.asarray(weight, np.float32)
    nz, ny, nx = tsdf.shape
    f = tsdf.transpose(2, 1, 0)                     # [x, y, z]
    ok = (weight >= np.float32(w_min)).transpose(2, 1, 0)
    inside = f < 0
    empty = dict(verts64=np.zeros((0, 3)), cols64=np.zeros((0, 3)),
                 verts=np.zeros((0, 3), np.float32), cols=np.zeros((0, 3), np.float32),
                 faces=np.zeros((0, 3), np.int64), edge_ids=np.zeros(0, np.int64))
    if min(nx, ny, nz) < 2:
        return empty
    sl = lambda a, o: a[o[0]:nx - 1 + o[0], o[1]:ny - 1 + o[1], o[2]:nz - 1 + o[2]]
    corners = list(itertools.product((0, 1), repeat=3))
    valid = np.all([sl(ok, o) for o in corners], 0)
    n_in = np.sum([sl(inside, o) for o in corners], 0)
    mixed = valid & (n_in > 0) & (n_in < 8)
    cx, cy, cz = np.nonzero(mixed)
    order = np.argsort(cx + nx * (cy + ny * cz), kind="stable")
    tets = kuhn_tetrahedra()

    def eid(p, q):
        lo, hi = np.minimum(p, q), np.maximum(p, q)
        return 7 * (lo[0] + nx * (lo[1] + ny * lo[2])) + _DIR_OF[tuple(hi - lo)]

    tris = []
    for n in order:
        cell = np.array([cx[n], cy[n], cz[n]])
        for tet in tets:
            pts = [cell + o for o in tet]
            ins = [p for p in pts if inside[tuple(p)]]
            outs = [p for p in pts if not inside[tuple(p)]]
            if not ins or not outs:
                continue
            toward = np.mean(outs, 0) - np.mean(ins, 0)       # inside -> outside
            mid = lambda p, q: (p + q) / 2.0
            if len(ins) == 2:
                (a, b), (c, d) = ins, outs
                pairs = [(a, c), (a, d), (b, d), (b, c)]
            else:
                a = ins[0] if len(ins) == 1 else outs[0]
                others = outs if len(ins) == 1 else ins
                pairs = [(a, o) for o in others]
            m = [mid(p, q) for p, q in pairs]
            normal = np.cross(m[1] - m[0], m[2] - m[0])
            assert abs(normal @ toward) > 1e-9
            ids = [eid(p, q) for p, q in pairs]
            if normal @ toward < 0:
                ids = ids[::-1]
            if len(ids) == 3:
                tris.append(ids)
            else:
                k = int(np.argmin(ids))
                q = ids[k:] + ids[:k]
                tris.append([q[0], q[1], q[2]])
                tris.append([q[0], q[2], q[3]])
    if not tris:
        return empty
    tris = np.array(tris, np.int64)
    edge_ids = np.unique(tris)
    faces = np.searchsorted(edge_ids, tris)
    p = edge_ids // 7
    d = DIRS[edge_ids % 7]
    pa = np.stack([p % nx, (p // nx) % ny, p // (nx * ny)], 1)
    pb = pa + d
    fa = f[pa[:, 0], pa[:, 1], pa[:, 2]].astype(np.float64)
    fb = f[pb[:, 0], pb[:, 1], pb[:, 2]].astype(np.float64)
    assert ((fa < 0) != (fb < 0)).all()
    t = fa / (fa - fb)
    o = np.asarray(origin, np.float32).astype(np.float64)
    verts = o + np.float64(np.float32(voxel)) * (pa + t[:, None] * d)
    c = np.asarray(rgb, np.float32).transpose(0, 3, 2, 1).astype(np.float64)   # [3, x, y, z]
    ca = c[:, pa[:, 0], pa[:, 1], pa[:, 2]].T
    cb = c[:, pb[:, 0], pb[:, 1], pb[:, 2]].T
    cols = ca + t[:, None] * (cb - ca)
    return dict(verts64=verts, cols64=cols, verts=verts.astype(np.float32),
                cols=cols.astype(np.float32), faces=faces, edge_ids=edge_ids)


def canonical_faces(faces):
    """Each face rotated to start at its smallest index, rows sorted:
    orientation is kept, the order of triangles is not."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(faces) == 0:
        return faces
    k = np.argmin(faces, 1)
    rot = np.stack([faces[np.arange(len(faces)), (k + j) % 3] for j in range(3)], 1)
    return rot[np.lexsort(rot.T[::-1])]


def mesh_stats(verts, faces):
    """Topology and size of a triangle mesh: numbers of vertices, undirected
    edges and faces, Euler characteristic, `closed` (every undirected edge in
    exactly two triangles), `oriented` (every directed edge in exactly one),
    `boundary_edges`, signed volume (positive: normals outward) and area."""
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    de = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    big = int(faces.max()) + 1 if len(faces) else 1
    dkey = de[:, 0] * big + de[:, 1]
    ukey = de.min(1) * big + de.max(1)
    _, dcount = np.unique(dkey, return_counts=True)
    _, ucount = np.unique(ukey, return_counts=True)
    used = len(np.unique(faces))
    a, b, c = (verts[faces[:, k]] for k in range(3))
    volume = float(np.einsum("ni,ni->n", a, np.cross(b, c)).sum() / 6.0)
    area = float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)
    return dict(nv=used, ne=len(ucount), nf=len(faces), euler=used - len(ucount) + len(faces),
                closed=bool((ucount == 2).all()), oriented=bool((dcount == 1).all()),
                boundary_edges=int((ucount == 1).sum()), volume=volume, area=area)
