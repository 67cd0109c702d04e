"""Frame ingest, host against device (splatt3r_amd/ingest.py):
  * dataio.FrameLoader alone, drained over one synthetic 640x480 TUM-layout
    sequence: frames/s with ingest="host" and ingest="device", the two modes
    alternating, `--repeats` drains each after one warm-up drain each (wall
    clock from the loader's creation to a device synchronise after the last
    frame);
  * resize_img_device by itself on frames already on the device: stream time
    per call (HIP events around 50 back-to-back calls, so at B = 1 it is the
    host's issue rate of a call, not the kernel's duration) for B = 1 and
    B = 8 frames, 640x480 -> 512x384 and 1920x1080 -> 512x288.
python -m tools.bench_ingest [--frames 240] [--workers 4] [--repeats 5]"""
from __future__ import annotations

import argparse
import json
import shutil
import statistics
import tempfile
import time

import numpy as np
import torch

from splatt3r_amd.dataio import FrameLoader, TUMDataset, write_synthetic_tum
from splatt3r_amd.ingest import resize_img_device


def drain(ds, mode, workers):
    t0 = time.perf_counter()
    loader = FrameLoader(ds, "cuda", workers=workers, depth=2 * workers, ingest=mode)
    n = 0
    for lf in loader:
        lf.consume()
        n += 1
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    loader.close()
    return n / t


def call_us(B, h, w, iters=50):
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, h, w, 3),
                                                                dtype=np.uint8)).cuda()
    for _ in range(3):
        resize_img_device(frames, 512)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        resize_img_device(frames, 512)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    root = tempfile.mkdtemp(prefix="s3_ingest_")
    try:
        ds = TUMDataset(write_synthetic_tum(root, a.frames, seed=7))
        fps = {"host": [], "device": []}
        for rep in range(a.repeats + 1):
            for mode in ("host", "device"):
                f = drain(ds, mode, a.workers)
                if rep:                                  # repeat 0 warms both modes up
                    fps[mode].append(f)
        out = {"frames": a.frames, "workers": a.workers, "repeats": a.repeats}
        for mode, v in fps.items():
            out[f"loader_{mode}_fps"] = {"median": round(statistics.median(v), 1),
                                         "min": round(min(v), 1), "max": round(max(v), 1)}
        for B, h, w in ((1, 480, 640), (8, 480, 640), (1, 1080, 1920), (8, 1080, 1920)):
            out[f"call_us_B{B}_{w}x{h}"] = round(call_us(B, h, w), 1)
        print(json.dumps(out), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
