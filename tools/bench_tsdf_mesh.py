"""TSDF fusion and mesh extraction (include/s3f.h, csrc/tsdf_mesh.hip) against
a torch composition of the same definition, same device, same inputs.

Scene: a sphere of radius 0.5 at the origin in front of a background 4 away,
seen from `--views` cameras 2 away on a Fibonacci sphere, analytic z-depth
maps of 384 x 512 made on the device; the volume is the cube [-0.64, 0.64]^3
at `--sizes` voxels a side.

  integrate   hip: s3f_integrate, `--batch` views per launch (the volume read
              and written once per launch); every batch of the sequence is
              timed between two device events, median (min - max) per batch.
              hip_b1 ...: the same at other batch sizes (--batches), which is
              what separates the two bounds: bytes per launch barely change
              with the batch, the float64 work per launch is proportional to
              it.
              torch: the definition view by view in float64 tensor ops over
              the whole volume (what this kernel replaces), `--torch-views`
              views per round.  hip and torch rounds alternate.
  bytes       the model, from the shapes: the five volume planes read once and
              written once per launch (40 B a voxel) plus the batch's depth
              and colour maps (16 B a pixel).  tb_per_s is bytes / time,
              hbm_fraction_* that over the 8 TB/s peak and the 6.3 TB/s a
              streaming kernel achieves on this chip (MI355X_MICROARCH:
              float4 copy).  `bound` is "bandwidth" when the launch runs
              within 1.5 x of bytes / 6.3 TB/s, else "fp64 arithmetic"; the
              per-batch-size rows show the scaling behind the word.
  extract     hip: s3f_mesh_count (cells, edges, scan) and s3f_mesh_emit
              (vertices, triangles) timed separately, the host read of the two
              counts between them outside both; torch: the same mesh from
              gathers, a (tetrahedron, case) table and torch.unique for the
              welding.  The two are checked against each other on a 64^3
              volume first (same vertices, same oriented faces).

One JSON line per measurement, on stdout and, with --log, appended to that
file as well (profiles/tsdf_mesh_bench.log is such a file).

python -m tools.bench_tsdf_mesh [--sizes 256 512] [--views 256] [--batch 32]
                                [--log profiles/tsdf_mesh_bench.log]"""
from __future__ import annotations

import argparse
import itertools
import json
import math
import statistics

import torch

from splatt3r_amd import _lib
from splatt3r_amd.mesh import TSDFVolume

HBM_PEAK = 8.0e12
HBM_ACHIEVABLE = 6.3e12
LOG = None
H, W, FOCAL = 384, 512, 420.0
RADIUS, BACKGROUND, HALF = 0.5, 4.0, 0.64


def report(**out):
    line = json.dumps(out)
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")
    return out


def stats(t):
    return {"median": round(statistics.median(t), 1), "min": round(min(t), 1),
            "max": round(max(t), 1)}


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def scene(V, dev):
    """(depth [V, H, W], color [V, 3, H, W], T_WC [V, 4, 4], K [3, 3])."""
    i = torch.arange(V, dtype=torch.float64) + 0.5
    phi = math.pi * (1 + 5 ** 0.5) * i
    zc = 1 - 2 * i / V
    r = (1 - zc * zc).sqrt()
    look = -torch.stack([r * phi.cos(), r * phi.sin(), zc], 1)          # camera z axes
    up = torch.tensor([0.123, 0.456, 0.881], dtype=torch.float64).expand(V, 3)
    x = torch.linalg.cross(up, look)
    x = x / x.norm(dim=1, keepdim=True)
    y = torch.linalg.cross(look, x)
    Rm = torch.stack([x, y, look], 2)
    pos = -2.0 * look
    T = torch.eye(4, dtype=torch.float64).repeat(V, 1, 1)
    T[:, :3, :3], T[:, :3, 3] = Rm, pos
    K = torch.tensor([[FOCAL, 0, (W - 1) / 2], [0, FOCAL, (H - 1) / 2], [0, 0, 1]])
    b, a = torch.meshgrid(torch.arange(H, dtype=torch.float64),
                          torch.arange(W, dtype=torch.float64), indexing="ij")
    rays = torch.stack([(a - K[0, 2]) / FOCAL, (b - K[1, 2]) / FOCAL, torch.ones_like(a)], -1)
    rays, Rm, pos = rays.to(dev), Rm.to(dev), pos.to(dev)
    depth = torch.empty(V, H, W, device=dev)
    for v in range(V):
        d = rays @ Rm[v].T
        qa, qb = (d * d).sum(-1), 2 * (d @ pos[v])
        disc = qb * qb - 4 * qa * (pos[v] @ pos[v] - RADIUS ** 2)
        hit = (-qb - disc.clamp_min(0).sqrt()) / (2 * qa)
        depth[v] = torch.where(disc > 0, hit, torch.full_like(hit, BACKGROUND)).float()
    color = torch.rand(V, 3, H, W, device=dev, generator=torch.Generator(dev).manual_seed(0))
    return depth, color, T.float().to(dev), K


# ------------------------------------------------------------ torch baseline
class TorchVolume:
    """The definition of include/s3f.h in torch tensor ops, float64."""

    def __init__(self, n, dev):
        self.n, self.voxel, self.origin = n, 2 * HALF / (n - 1), -HALF
        self.trunc, self.w_max = 4 * self.voxel, 64.0
        self.tsdf = torch.ones(n, n, n, device=dev)
        self.weight = torch.zeros(n, n, n, device=dev)
        self.rgb = torch.zeros(3, n, n, n, device=dev)
        ax = self.origin + self.voxel * torch.arange(n, device=dev, dtype=torch.float64)
        k, j, i = torch.meshgrid(ax, ax, ax, indexing="ij")
        self.xw = torch.stack([i, j, k], -1)

    def integrate(self, depth, T, K, color):
        M, t = T[:3, :3].double(), T[:3, 3].double()
        s2 = (M[:, 0] ** 2).sum()
        s = s2.sqrt()
        xc = (self.xw - t) @ M / s2
        x, y, z = xc.unbind(-1)
        u = float(K[0, 0]) * x / z + float(K[0, 2])
        v = float(K[1, 1]) * y / z + float(K[1, 2])
        a, b = (u + 0.5).floor(), (v + 0.5).floor()
        live = (z > 0) & (a >= 0) & (a <= W - 1) & (b >= 0) & (b <= H - 1)
        pix = torch.where(live, b * W + a, torch.zeros_like(a)).long()
        d = depth.reshape(-1)[pix]
        live &= torch.isfinite(d) & (d > 0)
        sdf = s * (d.double() - z)
        live &= ~(sdf < -self.trunc)
        fo = (sdf / self.trunc).clamp_max(1.0)
        w = self.weight.double()
        tot = w + 1.0
        self.tsdf = torch.where(live, ((self.tsdf.double() * w + fo) / tot).float(), self.tsdf)
        c = color.reshape(3, -1)[:, pix].double()
        self.rgb = torch.where(live, ((self.rgb.double() * w + c) / tot).float(), self.rgb)
        self.weight = torch.where(live, tot.clamp_max(self.w_max).float(), self.weight)


TET = [(0, 1 << a, (1 << a) | (1 << b), 7) for a, b, _ in itertools.permutations(range(3))]
DIR_OF = {1: 0, 2: 1, 4: 2, 3: 3, 6: 4, 5: 5, 7: 6}


def _vec(c):
    return [(c >> k) & 1 for k in range(3)]


def _det(a, b, c, d):
    m = [[q - p for p, q in zip(_vec(a), _vec(o))] for o in (b, c, d)]
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1])
            - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def case_table(nx, nxny):
    """(tetrahedron, 4-bit case) -> triangles as 3 edge offsets (7 * lattice
    offset + direction) from the cell's edge id base."""
    off = lambda c: (c & 1) + nx * ((c >> 1) & 1) + nxny * ((c >> 2) & 1)
    eid = lambda p, q: 7 * off(p & q) + DIR_OF[(p | q) ^ (p & q)]
    table = {}
    for t, cs in enumerate(TET):
        for case in range(1, 15):
            ins = [c for k, c in enumerate(cs) if (case >> k) & 1]
            outs = [c for k, c in enumerate(cs) if not (case >> k) & 1]
            if len(ins) == 2:
                (a, b), (c, d) = ins, outs
                q = [eid(a, c), eid(a, d), eid(b, d), eid(b, c)]
                if _det(a, b, c, d) < 0:
                    q = q[::-1]
                m = q.index(min(q))
                q = q[m:] + q[:m]
                table[t, case] = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            else:
                lone_in = len(ins) == 1
                a, o = (ins[0], outs) if lone_in else (outs[0], ins)
                flip = (_det(a, *o) > 0) != lone_in
                table[t, case] = [[eid(a, o[0]), eid(a, o[2] if flip else o[1]),
                                   eid(a, o[1] if flip else o[2])]]
    return table


def torch_extract(tsdf, weight, rgb, origin, voxel, w_min):
    nz, ny, nx = tsdf.shape
    dev = tsdf.device
    inside, ok = tsdf < 0, weight >= w_min
    sl = lambda a, c: a[(c >> 2) & 1:nz - 1 + ((c >> 2) & 1), (c >> 1) & 1:ny - 1 + ((c >> 1) & 1),
                        c & 1:nx - 1 + (c & 1)]
    valid = sl(ok, 0).clone()
    for c in range(1, 8):
        valid &= sl(ok, c)
    base = 7 * torch.arange(nz * ny * nx, device=dev).view(nz, ny, nx)[:-1, :-1, :-1]
    table = case_table(nx, nx * ny)
    tris = []
    for t, cs in enumerate(TET):
        case = sum(sl(inside, c).to(torch.int32) << k for k, c in enumerate(cs))
        case = torch.where(valid, case, torch.zeros_like(case))
        for cv in range(1, 15):
            cells = base[case == cv]
            if cells.numel():
                for tri in table[t, cv]:
                    tris.append(cells[:, None] + torch.tensor(tri, device=dev))
    if not tris:
        return (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev),
                torch.zeros(0, 3, dtype=torch.int32, device=dev))
    tris = torch.cat(tris)
    edges, inverse = torch.unique(tris, return_inverse=True)
    p, d = edges // 7, edges % 7
    code = torch.tensor([1, 2, 4, 3, 6, 5, 7], device=dev)[d]
    step = torch.stack([code & 1, (code >> 1) & 1, (code >> 2) & 1], 1)
    q = p + step[:, 0] + nx * step[:, 1] + nx * ny * step[:, 2]
    f = tsdf.reshape(-1).double()
    tt = f[p] / (f[p] - f[q])
    pa = torch.stack([p % nx, (p // nx) % ny, p // (nx * ny)], 1).double()
    verts = torch.tensor(origin, device=dev, dtype=torch.float64) + voxel * (pa + tt[:, None] * step)
    c = rgb.reshape(3, -1).double()
    cols = (c[:, p] + tt * (c[:, q] - c[:, p])).T
    return verts.float(), cols.float(), inverse.to(torch.int32)


def canonical(faces):
    k = faces.argmin(1, keepdim=True)
    rot = torch.cat([faces.gather(1, (k + j) % 3) for j in range(3)], 1).long()
    key = (rot[:, 0] * (rot.max() + 1) + rot[:, 1]) * (rot.max() + 1) + rot[:, 2]
    return rot[key.argsort()]


# ------------------------------------------------------------------- parts
def make_volume(n, dev):
    return TSDFVolume(dims=(n, n, n), voxel=float(2 * HALF / (n - 1)), origin=(-HALF,) * 3,
                      device=dev)


def check_agreement(depth, color, T, K, dev):
    """hip and torch on a 64^3 volume and 4 views: the same state within one
    float32 ulp a view, the same mesh."""
    vol, tv = make_volume(64, dev), TorchVolume(64, dev)
    vol.integrate(depth[:4], T[:4], K, color=color[:4])
    for v in range(4):
        tv.integrate(depth[v], T[v], K, color[v])
    dt = float((vol.tsdf - tv.tsdf).abs().max())
    dw = float((vol.weight - tv.weight).abs().max())
    hv, hc, hf = vol.extract()
    tvv, tcc, tff = torch_extract(vol.tsdf, vol.weight, vol.rgb, vol.origin, vol.voxel, 1.0)
    same = hv.shape == tvv.shape and hf.shape == tff.shape and \
        bool((canonical(hf) == canonical(tff)).all())
    report(part="agreement", n=64, views=4, tsdf_max_abs_diff=dt, weight_max_abs_diff=dw,
           verts=int(hv.shape[0]), tris=int(hf.shape[0]), same_faces=same,
           verts_max_abs_diff=float((hv - tvv).abs().max()) if same else None)
    assert same and dt < 1e-5


def bench_integrate(n, depth, color, T, K, a, dev):
    V = depth.shape[0]
    nvox = n ** 3
    vol = make_volume(n, dev)
    batches = sorted(set(a.batches + [a.batch]))
    times = {b: [] for b in batches}
    torch_t = []
    tv = None if a.no_torch else TorchVolume(n, dev)
    for b in batches:                                            # warm up every shape
        vol.integrate(depth[:b], T[:b], K, color=color[:b])
    if tv is not None:
        tv.integrate(depth[0], T[0], K, color[0])
    torch.cuda.synchronize()
    starts = list(range(0, V - a.batch + 1, a.batch))
    for r, s0 in enumerate(starts):
        for b in batches:
            if b != a.batch and r >= a.rounds:
                continue
            sl = slice(s0, s0 + b)
            times[b].append(event_us(lambda: vol.integrate(depth[sl], T[sl], K, color=color[sl])))
        if tv is not None and r < a.rounds:
            for v in range(s0, s0 + a.torch_views):
                torch_t.append(event_us(lambda: tv.integrate(depth[v], T[v], K, color[v])))
    out = {}
    for b in batches:
        us = stats(times[b])
        nbytes = 40 * nvox + 16 * H * W * b
        sec = us["median"] * 1e-6
        floor_us = nbytes / HBM_ACHIEVABLE * 1e6
        out[b] = report(part="integrate", variant="hip", n=n, batch=b, launches=len(times[b]),
                        us_per_batch=us, us_per_view=round(us["median"] / b, 1), bytes=nbytes,
                        tb_per_s=round(nbytes / sec / 1e12, 3),
                        hbm_fraction_of_peak=round(nbytes / sec / HBM_PEAK, 3),
                        hbm_fraction_of_achievable=round(nbytes / sec / HBM_ACHIEVABLE, 3),
                        bandwidth_floor_us=round(floor_us, 1),
                        pairs_per_s=round(nvox * b / sec / 1e9, 2),
                        bound="bandwidth" if us["median"] <= 1.5 * floor_us else "fp64 arithmetic")
    if tv is not None:
        us = stats(torch_t)
        report(part="integrate", variant="torch_float64", n=n, views=len(torch_t), us_per_view=us,
               torch_over_hip_per_view=round(us["median"] / out[a.batch]["us_per_view"], 1))
        del tv
    torch.cuda.empty_cache()
    return vol


def bench_extract(n, vol, a, dev):
    lib = _lib.lib()
    need = int(lib.s3f_mesh_workspace_bytes(n, n, n))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    st = _lib.stream(dev)
    count = lambda: _lib.call("s3f_mesh_count", vol.tsdf.data_ptr(), vol.weight.data_ptr(), n, n,
                              n, 1.0, counts.data_ptr(), ws.data_ptr(), need, st)
    count()
    nv, nt = counts.tolist()
    verts, cols = torch.empty(nv, 3, device=dev), torch.empty(nv, 3, device=dev)
    faces = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    emit = lambda: _lib.call("s3f_mesh_emit", vol.tsdf.data_ptr(), vol.rgb.data_ptr(), n, n, n,
                             *vol.origin, vol.voxel, nv, nt, verts.data_ptr(), cols.data_ptr(),
                             faces.data_ptr(), nv, nt, ws.data_ptr(), need, st)
    emit()
    torch.cuda.synchronize()
    tc, te, tt = [], [], []
    for r in range(a.rounds):
        tc.append(event_us(count))
        te.append(event_us(emit))
        if not a.no_torch and r < a.torch_rounds:
            tt.append(event_us(lambda: torch_extract(vol.tsdf, vol.weight, vol.rgb, vol.origin,
                                                     vol.voxel, 1.0)))
    c, e = stats(tc), stats(te)
    report(part="extract", variant="hip", n=n, verts=nv, tris=nt, us_count=c, us_emit=e,
           us_total=round(c["median"] + e["median"], 1), workspace_bytes=need)
    if tt:
        us = stats(tt)
        report(part="extract", variant="torch", n=n, us=us,
               torch_over_hip=round(us["median"] / (c["median"] + e["median"]), 1))
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-views", type=int, default=2)
    ap.add_argument("--torch-rounds", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    global LOG
    LOG = a.log
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_mesh needs a GPU")
    dev = torch.device("cuda", 0)
    depth, color, T, K = scene(a.views, dev)
    report(part="scene", views=a.views, H=H, W=W, sphere_pixels=int((depth[0] < BACKGROUND).sum()))
    check_agreement(depth, color, T, K, dev)
    for n in a.sizes:
        vol = bench_integrate(n, depth, color, T, K, a, dev)
        bench_extract(n, vol, a, dev)
        del vol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
