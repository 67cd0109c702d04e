"""Lens undistortion on the device (splatt3r_amd/intrinsics.py, include/s3u.h)
at EuRoC's 752x480 with MH_01's cam0 maps:
  * `s3u_remap` alone, C = 1 and C = 3, B = 1 and B = 8: stream time per
    launch (HIP events around `--iters` back-to-back launches of the raw entry
    point, median of `--repeats` windows after a warm-up window), beside the
    traffic model (8 B of map per pixel once, 3 B out per pixel and frame, the
    source once per frame) at the achieved HBM bandwidth of a float4 copy.
    At B = 1 the window is bounded by the host's issue rate of a launch, not
    by the kernel: the kernel's own duration comes from a kernel trace
    (rocprofv3 --kernel-trace --stats -- python -m tools.bench_undistort
    --trace), which runs the same launches without timing them;
  * the chain `resize_img_device(frame, 512, undistort=intr)` (remap, then
    ingest) against `resize_img_device` alone, per call;
  * the host's numpy `remap_u8` per frame (wall clock).
python -m tools.bench_undistort [--iters 200] [--repeats 7] [--trace]"""
from __future__ import annotations

import argparse
import json
import statistics
import time

import numpy as np
import torch

from splatt3r_amd import _lib
from splatt3r_amd.dataio import EUROC_DISTORTION, EUROC_INTRINSICS, EUROC_RESOLUTION
from splatt3r_amd.ingest import resize_img_device
from splatt3r_amd.intrinsics import Intrinsics

ACHIEVED_HBM = 6.29e12         # B/s, float4 copy on this device


def windows(fn, iters, repeats):
    """Median / min / max stream time of one call, in us."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for rep in range(repeats + 1):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:                                          # window 0 warms up
            out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return {"median": round(statistics.median(out), 2), "min": round(min(out), 2),
            "max": round(max(out), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--trace", action="store_true",
                    help="only run the launches (for a kernel trace): no timing, no host remap")
    a = ap.parse_args()
    W, H = EUROC_RESOLUTION
    intr = Intrinsics.from_calib(512, W, H, [*EUROC_INTRINSICS, *EUROC_DISTORTION],
                                 always_undistort=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    mx, my = intr._map.on_device(dev)
    rng = np.random.default_rng(0)
    lib = _lib.lib()
    out = {"size": f"{W}x{H}", "iters": a.iters, "repeats": a.repeats}
    for C in (1, 3):
        for B in (1, 8):
            src = torch.from_numpy(rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)).to(dev)
            dst = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
            args = (src.data_ptr(), B, H, W, C, mx.data_ptr(), my.data_ptr(), H, W, dst.data_ptr(),
                    _lib.stream())
            fn = lambda: lib.s3u_remap(*args)
            assert fn() == 0
            model = H * W * (8 + B * (3 + C))
            if a.trace:
                for _ in range(a.iters):
                    fn()
                torch.cuda.synchronize()
                continue
            r = windows(fn, a.iters, a.repeats)
            r["model_bytes"] = model
            r["model_us_at_6.29TBps"] = round(model / ACHIEVED_HBM * 1e6, 2)
            out[f"remap_us_C{C}_B{B}"] = r
    if not a.trace:
        for C in (1, 3):
            frame = torch.from_numpy(rng.integers(0, 256, (H, W, C), dtype=np.uint8)).to(dev)
            out[f"remap_ingest_us_C{C}"] = windows(
                lambda: resize_img_device(frame, 512, undistort=intr), a.iters, a.repeats)
        rgb = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        out["ingest_alone_us"] = windows(lambda: resize_img_device(rgb, 512), a.iters, a.repeats)
        for C in (1, 3):
            img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)[..., 0] if C == 1 else \
                rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            intr.remap(img)
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                intr.remap(img)
                t.append((time.perf_counter() - t0) * 1e3)
            out[f"host_remap_u8_ms_C{C}"] = round(statistics.median(t), 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
