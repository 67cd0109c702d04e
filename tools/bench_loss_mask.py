"""Co-visibility loss mask, fused HIP against a float32 torch-op composition of
the same definition on the same device (splatt3r_amd/loss_mask.py,
include/s3c.h).

  * fused: calculate_in_frustum_mask (the inverse prologue + one pass over the
    target pixels);
  * torch: torch.linalg.inv of the intrinsics and poses, the projection chain
    as einsums over [b, v1, v2, h, w, 3] intermediates, one F.grid_sample per
    (b, v1, v2), isclose and the two any().
The two variants alternate in one process; device events around every round,
`--warmup` rounds, then `--rounds` timed ones; median (min - max) in
microseconds.  The launch counts are counted, not timed: the aten operators a
variant dispatches in one round that launch a kernel (views and allocations
left out), plus the library's two launches for the fused variant.
s3c_loss_mask_us is the library call alone, back to back, and floor_us the
least time the bytes it must move could take at the achieved copy bandwidth
of the device (6.29 TB/s): 4 h w (v1 + v2) bytes of depth read plus the
h w v1 mask bytes written.

The scene is a wavy surface seen by cameras a few centimetres apart, so the
context reads are the coherent gather of real use.

python -m tools.bench_loss_mask [--rounds 50] [--warmup 3]"""
from __future__ import annotations

import argparse
import json
import math
import statistics

import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

from splatt3r_amd import _lib
from splatt3r_amd import loss_mask as LM

SHAPES = ((1, 1, 2, 384, 512), (1, 1, 2, 540, 960))
HIP_LAUNCHES = 2
COPY_BYTES_PER_S = 6.29e12
_NO_KERNEL = ("view", "reshape", "expand", "empty", "as_strided", "detach", "alias", "permute",
              "select", "slice", "squeeze", "unsqueeze", "transpose", "t.default", "_to_copy",
              "lift_fresh", "_local_scalar_dense", "unbind", "split")


class _OpCount(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func).replace("aten.", "")
        if not name.startswith(_NO_KERNEL):
            self.n += 1
        return func(*args, **(kwargs or {}))


@torch.no_grad()
def torch_composition(depth_1, K_1, c2w_1, depth_2, K_2, c2w_2):
    """The definition of include/s3c.h in float32 torch ops."""
    b, v1, h, w = depth_1.shape
    v2 = depth_2.shape[1]
    dev = depth_1.device
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32),
                            torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1)
    cam = torch.einsum("bvij,hwj->bvhwi", torch.linalg.inv(K_1), pix) * depth_1[..., None]
    cam = torch.cat([cam, torch.ones_like(cam[..., :1])], -1)
    world = torch.einsum("bvij,bvhwj->bvhwi", c2w_1, cam)[..., :3]
    world = torch.cat([world, torch.ones_like(world[..., :1])], -1)
    cp = torch.einsum("buij,bvhwj->bvuhwi", torch.linalg.inv(c2w_2), world)[..., :3]
    z = cp[..., 2]
    uv = torch.einsum("buij,bvuhwj->bvuhwi", K_2, cp / cp[..., 2:])[..., :2]
    u, v = uv[..., 0], uv[..., 1]
    fr = ((u > 0) & (u < w) & (v > 0) & (v < h)).any(2)
    grid = torch.stack([u / w, v / h], -1) * 2 - 1
    md = torch.empty_like(z, dtype=torch.bool)
    for bb in range(b):
        for i in range(v1):
            for j in range(v2):
                s = F.grid_sample(depth_2[bb, j][None, None], grid[bb, i, j][None],
                                  align_corners=False)[0, 0]
                md[bb, i, j] = torch.isclose(z[bb, i, j], s, atol=1e-1)
    return fr & (depth_1 > 1e-6) & md.any(2)


def scene(shape, device):
    b, v1, v2, h, w = shape
    g = torch.Generator().manual_seed(0)
    f = float(max(h, w))
    K = torch.tensor([[f, 0, w / 2.0], [0, 1.05 * f, h / 2.0], [0, 0, 1]])
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32),
                            torch.arange(w, dtype=torch.float32), indexing="ij")

    def view():
        T = torch.eye(4)
        T[:3, 3] = (torch.rand(3, generator=g) - 0.5) * 0.1
        a = float(torch.rand(1, generator=g) - 0.5) * 0.05
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
        depth = 3.0 + 0.3 * torch.sin(xs / 37.0 + T[0, 3]) * torch.cos(ys / 29.0)
        depth[torch.rand(h, w, generator=g) < 0.05] = 0.0
        return depth, K.clone(), T

    out = []
    for nv in (v1, v2):
        views = [[view() for _ in range(nv)] for _ in range(b)]
        for k in range(3):
            out.append(torch.stack([torch.stack([v[k] for v in row]) for row in views])
                       .to(device).contiguous())
    return out


def library_call_us(args, iters=20):
    """Stream time of s3c_loss_mask alone: device events around `iters`
    back-to-back calls on preallocated buffers."""
    b, v1, h, w = args[0].shape
    v2 = args[3].shape[1]
    dev = args[0].device
    L = _lib.lib()
    mask = torch.empty((b, v1, h, w), dtype=torch.bool, device=dev)
    ws = torch.empty(L.s3c_loss_mask_workspace_bytes(b, v1, v2), dtype=torch.uint8, device=dev)
    call = lambda: _lib.call("s3c_loss_mask", *[t.data_ptr() for t in args], b, v1, v2, h, w,
                             mask.data_ptr(), None, None, ws.data_ptr(), _lib.stream(dev))
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / iters, 1)


def bench_shape(shape, device, rounds, warmup):
    b, v1, v2, h, w = shape
    args = scene(shape, device)
    runs = {"fused": lambda: LM.calculate_in_frustum_mask(*args),
            "torch": lambda: torch_composition(*args)}
    out = {"shape": list(shape)}
    mf, mt = runs["fused"](), runs["torch"]()
    out["mask_fraction"] = round(float(mf.float().mean()), 4)
    out["differing_pixels"] = int((mf != mt).sum())      # float32 rounding at the edges
    out["s3c_loss_mask_us"] = library_call_us(args)
    nbytes = 4 * h * w * b * (v1 + v2) + h * w * b * v1
    out["bytes"] = nbytes
    out["floor_us"] = round(nbytes / COPY_BYTES_PER_S * 1e6, 2)
    for key, run in runs.items():
        with _OpCount() as oc:
            run()
        out[f"{key}_launching_ops"] = oc.n + (HIP_LAUNCHES if key == "fused" else 0)
    times = {k: [] for k in runs}
    for r in range(warmup + rounds):
        for key, run in runs.items():           # variants alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[key].append(e0.elapsed_time(e1) * 1e3)
    for key, v in times.items():
        out[f"{key}_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                            "max": round(max(v), 1)}
    out["torch_over_fused"] = round(out["torch_us"]["median"] / out["fused_us"]["median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_mask needs a GPU")
    device = torch.device("cuda", 0)
    for shape in SHAPES:
        print(json.dumps(bench_shape(shape, device, a.rounds, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
