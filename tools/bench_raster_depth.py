"""Depth + alpha from the blend pass against a second render with fake
colours (BASELINE config 3 scene: P synthetic Gaussians @ 960x540).

Three variants, alternated round by round in one process and timed with HIP
events on torch's current stream (the one the rasterizer launches on):

  colour    the colour-only forward / backward (GaussianRasterizer)
  fused     return_depth=True: colour + depth + alpha from one blend pass;
            backward with all three pixel gradients in one call
  two_pass  what a caller did before: the colour render, then a second full
            render (preprocess, both sorts, blend) with colors_precomp =
            (view z, 1, 0); backward = the two colour backwards

The forward is timed under no_grad; the backward times loss.backward() alone,
after the forward has finished, like tools/bench_raster.py.

  python -m tools.bench_raster_depth --P 4194304 --iters 10
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np
import torch

from tools.bench_raster import prepare


def _stats(ms):
    a = np.asarray(ms, np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def run(P=4_194_304, iters=10, warmup=3, device="cuda"):
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizer
    sc, rs, inputs, grad = prepare(P, device)
    H, W = sc["H"], sc["W"]
    rast = GaussianRasterizer(rs)
    leaf = {k: v.clone().requires_grad_(True) for k, v in inputs.items()}
    g = torch.Generator(device=device).manual_seed(5)
    g_d = torch.randn(H, W, generator=g, device=device)
    g_a = torch.randn(H, W, generator=g, device=device)
    grad2 = torch.stack([g_d, g_a, torch.zeros_like(g_d)])
    geo = dict(means3D=leaf["means3D"], opacities=leaf["opacities"],
               cov3D_precomp=leaf["cov3D_precomp"])
    # the second pass's colours: the kernel's own view z (identity camera: means z)
    with torch.no_grad():
        rast(means2D=torch.zeros_like(leaf["means3D"]), shs=leaf["shs"], **geo, return_depth=True)
    fake = torch.stack([dgr.last_view_z, torch.ones_like(dgr.last_view_z),
                        torch.zeros_like(dgr.last_view_z)], 1).contiguous().requires_grad_(True)

    def m2():
        return torch.zeros_like(leaf["means3D"], requires_grad=True)

    def colour():
        return rast(means2D=m2(), shs=leaf["shs"], **geo)

    def fused():
        return rast(means2D=m2(), shs=leaf["shs"], **geo, return_depth=True)

    def second():
        return rast(means2D=m2(), colors_precomp=fake, **geo)

    fwd = {"colour": lambda: (colour(),), "fused": lambda: (fused(),),
           "two_pass": lambda: (colour(), second())}

    def losses(name):
        if name == "colour":
            return [(colour()[0] * grad).sum()]
        if name == "fused":
            img, _, depth, alpha = fused()
            return [(img * grad).sum() + (depth * g_d).sum() + (alpha * g_a).sum()]
        return [(colour()[0] * grad).sum(), (second()[0] * grad2).sum()]

    def clear():
        for v in list(leaf.values()) + [fake]:
            v.grad = None

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    f_ms = {k: [] for k in fwd}
    b_ms = {k: [] for k in fwd}
    for it in range(warmup + iters):
        for name, f in fwd.items():
            torch.cuda.synchronize()
            ev[0].record()
            with torch.no_grad():
                f()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= warmup:
                f_ms[name].append(ev[0].elapsed_time(ev[1]))
        for name in fwd:
            clear()
            ls = losses(name)
            torch.cuda.synchronize()
            ev[0].record()
            for l in ls:
                l.backward()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= warmup:
                b_ms[name].append(ev[0].elapsed_time(ev[1]))
    # the two ways agree (depth / alpha bit for bit; the depth-to-mean term
    # of the fused backward is not in the two-pass sum: compare opacity)
    with torch.no_grad():
        img, _, depth, alpha = fused()
        img2 = second()[0]
    clear()
    for l in losses("fused"):
        l.backward()
    dop = leaf["opacities"].grad.clone()
    clear()
    for l in losses("two_pass"):
        l.backward()
    dop2 = leaf["opacities"].grad
    check = dict(depth_equal=bool(torch.equal(depth, img2[0])),
                 alpha_equal=bool(torch.equal(alpha, img2[1])),
                 dL_dopacity_rel=float((dop - dop2).abs().max() / dop2.abs().max()))
    out = dict(P=P, H=H, W=W, iters=iters, num_rendered=int(dgr.last_num_rendered),
               forward_ms={k: _stats(v) for k, v in f_ms.items()},
               backward_ms={k: _stats(v) for k, v in b_ms.items()}, check=check)
    for tag, d in (("forward", out["forward_ms"]), ("backward", out["backward_ms"])):
        out[f"{tag}_fused_over_colour"] = d["fused"]["median"] / d["colour"]["median"]
        out[f"{tag}_fused_over_two_pass"] = d["fused"]["median"] / d["two_pass"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=4_194_304)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    t0 = time.time()
    out = run(a.P, a.iters)
    print(json.dumps(out))
    for tag in ("forward", "backward"):
        for k, s in out[f"{tag}_ms"].items():
            print(f"# {tag:8s} {k:8s} median {s['median']:8.3f} ms  "
                  f"(min {s['min']:.3f}, max {s['max']:.3f})")
    print(f"# wall {time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
