#!/usr/bin/env python3
"""Headline benchmark: SLAM frames/sec (TUM fr1_desk-shaped 512x384 frames)
+ Msplats/sec rasterized, on 1..8 MI355X.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \\
      --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps, writes the last timed
step's outputs when --dump-outputs is given and prints the result line.
Every other leg described below (per-kernel profile and roofline, end-to-end,
live camera, keyframe pairs, backend, C5 map, C3 raster, retrieval, CPU
baseline) runs only with --full, after the timed region.

A step is one frame of the reference's main loop in TRACKING mode
(main.py:451-506 with --no-viz, rendering on, spatial stride 4):
encoder on the new frame, fused decoder + both heads against the last
keyframe, dense matching, Gauss-Newton pose, pointmap fusion, keyframe test,
gaussians_to_world on every tracked frame (as the reference under --no-viz), and the Gaussian render
of the frame's 2*h*w splats read back to the host.  The tracker path does not
shard (frame i depends on frame i-1), so with N GPUs each rank runs an
independent replica on its own synthetic sequence: weak scaling, value =
frames of all ranks / max-over-ranks wall time.  The keyframe-pair batch
(the unit that does shard) is reported beside it by
splatt3r_amd/pairs.py through the sharded FactorGraph.add_factors path.

Further legs on rank 0 (N = 1, --full): `backend` -- the same frontend with the
reference's backend running concurrently on a worker thread / HIP stream
(base.yaml single_thread: False: retrieval + add_factors + GN per
keyframe), reported as a second frames/s; `map_c5` -- the full-map render
of an 8,388,608-Gaussian world map (C5) at 960x540; `raster_c3` (C3),
`retrieval`, and the CPU baseline.

Weights are portable-PRNG (no checkpoint offline) with the two decoder
branches and the two heads tied (weights.tie_symmetric: same architecture,
same FLOPs), which makes a view's cross prediction agree with a nearby
view's self prediction as trained weights do; with the synthetic sequence
panning 2 px/frame the reference's default thresholds (config/base.yaml)
then give ~57 % valid matches and GN convergence in ~5 iterations
(measured with the CPU oracle), i.e. the TRACKING path with realistic trip
counts.  Nothing in the configuration is changed.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [REPO, os.path.join(REPO, "splatt3r-slam_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

H, W = 384, 512
PEAK_F16_TFLOPS = 2500.0   # gfx950 dense FP16/BF16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBPS = 8000.0


def _args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1,
                    help="ranks (one per GPU); without an external launcher (WORLD_SIZE unset) "
                         "bench.py starts N worker processes itself")
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline (per-kernel profile and "
                         "roofline, end-to-end, live camera, keyframe pairs, backend, C5 map, "
                         "C3 raster, retrieval, CPU baseline); the --no-* options below pick "
                         "among them.  Without it only the headline's frame loop runs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned "
                         "(rank 0: pose, fused pointmap, confidence, render) as DIR/<name>.npy")
    ap.add_argument("--cpu-frames", type=int, default=2,
                    help="frames of the CPU restatement timed for cpu_baseline (rank 0, N=1)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-c3", action="store_true", help="skip the 4.19M-splat raster microbench")
    ap.add_argument("--no-pairs", action="store_true", help="skip the keyframe-pair batch leg")
    ap.add_argument("--strong-pairs", type=int, default=16,
                    help="keyframe pairs per batch of the strong-scaling pair leg (fixed total)")
    ap.add_argument("--no-backend", action="store_true",
                    help="skip the frontend + concurrent backend leg")
    ap.add_argument("--backend-steps", type=int, default=60)
    ap.add_argument("--no-map", action="store_true", help="skip the C5 full-map render leg")
    ap.add_argument("--no-e2e", action="store_true",
                    help="skip the end-to-end leg (dataset PNG read + resize + H2D + PNG write)")
    ap.add_argument("--no-live", action="store_true",
                    help="skip the live-camera leg (no lookahead: one frame at a time)")
    ap.add_argument("--pairs-per-rank", type=int, default=4)
    ap.add_argument("--no-kprof", action="store_true",
                    help="skip the per-launch network profile (roofline object)")
    ap.add_argument("--no-in-window", action="store_true",
                    help="skip the in-frame-loop kernel trace (roofline.in_window)")
    ap.add_argument("--enc-batch", type=int, default=8,
                    help="frames per encoder replay (lookahead over the sequence); the last "
                         "replay of the timed region is partial when --steps is not a multiple")
    ap.add_argument("--main-priority", type=int, default=-1,
                    help="HIP stream priority of the frame's main chain (-1 = high, the "
                         "default: the next frame's encoder yields to it); 0 = normal")
    ap.add_argument("--late-prefetch", action="store_true",
                    help="queue the next frame's encoder after the tracker's GN sync")
    ap.add_argument("--enc-ahead", type=int, default=8,
                    help="frames kept queued for encoding ahead of the current one "
                         "(0: the next enc-batch frames once frame i+1 is not queued)")
    ap.add_argument("--render-async", action="store_true",
                    help="render + PNG write / read-back on a render worker thread and stream "
                         "(slam._RenderWorker; measured slower, profiles/r03m_ab.log)")
    ap.add_argument("--no-decode-ahead", dest="decode_ahead", action="store_false",
                    help="decode each frame alone (default: the next frame is decoded "
                         "against the same keyframe in the same Bp=2 pair-plan replay, "
                         "used when no keyframe is added in between)")
    ap.add_argument("--e2e-loaders", type=int, default=4,
                    help="end-to-end leg: dataset read + resize_img threads")
    ap.add_argument("--e2e-writers", type=int, default=3,
                    help="end-to-end leg: render PNG writer threads")
    ap.add_argument("--no-deferred-render", dest="deferred_render", action="store_false",
                    help="two-call rasterizer (host read of num_rendered every frame)")
    ap.add_argument("--no-spans", action="store_true",
                    help="no per-frame HIP events in the timed region (no critical_path)")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="encode each frame inside its own step (no side-stream overlap)")
    ap.add_argument("--dist-dry-run", action="store_true",
                    help="CPU check of the launch path: spawn / rendezvous (gloo) / barrier / "
                         "max over ranks / pair sharding, no GPU work (tests/test_bench_plan.py)")
    a = ap.parse_args(argv)
    if not a.full and not a.dist_dry_run:
        # a plain run: the headline's frame loop alone (the dry run times
        # nothing: it walks the launch path of every sharded leg)
        for leg in _FULL_LEGS:
            setattr(a, "no_" + leg, True)
    return a


# the legs beside the headline (each has a --no-<leg> option), run with --full
_FULL_LEGS = ("cpu_baseline", "c3", "pairs", "backend", "map", "e2e", "live", "kprof",
              "in_window")


def dump_outputs(path, frame, render):
    """--dump-outputs: what the last timed Frontend.step handed back, one
    float32 .npy each: the tracked Frame's pose (Sim3 data: t, q xyzw, s),
    fused canonical pointmap and confidence, and the frame's Gaussian render
    as read back to the host (H x W x 3).  ~5 MB at 512x384."""
    os.makedirs(path, exist_ok=True)
    out = {"pose": frame.T_WC.data, "pointmap": frame.X_canon, "confidence": frame.C,
           "render": render}
    for name, t in out.items():
        if t is None:
            continue
        arr = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
        np.save(os.path.join(path, name + ".npy"), arr)


# S3_PLAN_OVERLAP=0: the first exact plan of the search (round-4 driver runs;
# the last timed replay is then queued by the last timed step) (A/B)
_PLAN_OVERLAP = os.environ.get("S3_PLAN_OVERLAP", "1") != "0"


def plan_encodes(steps: int, warmup: int, enc_batch: int, enc_ahead, pipeline: bool = True):
    """The encoder queueing of the bench's frame sequence, simulated with the
    frontend's own rule (slam.lookahead_batches), and the lookahead caps that
    make the timed region hold exactly `steps` image encodes.

    Frame 0 is INIT, frames 1..warmup are warm-up, frames warmup+1 ..
    warmup+steps are timed.  A frame not queued when it is stepped is encoded
    alone; each step hands over the next frames as lookahead: warm-up steps
    only frames below `cap_warm`, timed steps only frames below `cap`.  The
    caps are chosen so that the encodes queued by timed steps number exactly
    `steps` (the last replay is a partial batch when `steps` is not a
    multiple of `enc_batch`), every timed replay queued as far ahead of its
    first frame as in the steady state and the last one as early as that
    allows (see below; None = uncapped).  Returns {batches: [(first frame, count, timed)], cap,
    cap_warm, timed_encodes, next_enc_before (the frontend's _next_enc after
    warm-up), frames_needed, look}."""
    from splatt3r_amd.slam import lookahead_batches
    kb = max(1, int(enc_batch))
    look = kb + max(enc_ahead or 1, 1)
    nfr = warmup + steps + 1

    def sim(cap_warm, cap):
        nxt_enc, batches, before = 0, [], None
        sim.last_q = -1                     # frame whose step queued the last timed replay
        sim.slack = 1 << 30                 # min over timed replays: first frame - queuing frame
        for i in range(nfr):
            timed = i > warmup
            if i == warmup + 1:
                before = nxt_enc
            if nxt_enc <= i:                    # frame i not queued: encoded alone
                batches.append((i, 1, timed))
                nxt_enc = i + 1
            if not pipeline:
                continue
            c_ = cap if timed else cap_warm
            hi = i + 1 + look if c_ is None else min(i + 1 + look, c_)
            for s, c in lookahead_batches(i, nxt_enc, max(0, hi - (i + 1)), kb, enc_ahead):
                batches.append((s, c, timed))
                nxt_enc = s + c
                if timed:
                    sim.last_q = i
                    sim.slack = min(sim.slack, s - i)
        return batches, before, sum(c for _, c, t in batches if t)

    if not pipeline:
        batches, before, n = sim(None, None)
        return dict(batches=batches, cap=None, cap_warm=None, timed_encodes=n,
                    next_enc_before=before, frames_needed=nfr, look=look)
    # Of the (cap_warm, cap) pairs that give exactly `steps` timed encodes:
    # the largest lead of every timed replay over its first frame (the
    # steady state's: no frame waits for its encode), then the last timed
    # replay queued earliest, so that it overlaps later timed frames'
    # main-stream work as every replay does in the steady state (one queued
    # by the last timed step would run alone after the last frame, for
    # frames past the region).
    best = None
    for cap_warm in [None] + list(range(warmup + 1 + look, warmup, -1)):
        _, before, _ = sim(cap_warm, None)
        # timed encodes are non-decreasing in the cap, by at most one per frame
        for cap in range(before + steps, before + steps + look + kb + 2):
            b, bf, n = sim(cap_warm, cap)
            key = ((abs(n - steps), -sim.slack, sim.last_q) if _PLAN_OVERLAP
                   else (abs(n - steps),))
            if best is None or key < best[5]:
                best = (cap_warm, cap, b, n, bf, key)
            if n >= steps:
                break
    cap_warm, cap, batches, n, before, _ = best
    need = max(nfr + look, cap)
    return dict(batches=batches, cap=cap, cap_warm=cap_warm, timed_encodes=n,
                next_enc_before=before, frames_needed=need, look=look)


def _spawn(a, argv) -> int:
    """`--gpus N` without an external launcher: start N worker processes of
    this script (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* as torchrun sets
    them, rendezvous on 127.0.0.1) and return the worst exit status.  The
    parent never touches the GPU (no HIP call before the children start)."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus),
                   LOCAL_WORLD_SIZE=str(a.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv),
                                      env=env))
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            r = p.poll()
            if r is None:
                continue
            live.remove(p)
            if r != 0 and rc == 0:
                rc = r
                # a failed rank leaves the others blocked in a collective
                for q in live:
                    q.terminate()
        time.sleep(0.05)
    for p in procs:
        p.wait()
    return rc if rc >= 0 else 128 - rc


def _dist(a):
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if ws != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={ws}: launch one process per GPU "
                         f"(torch.distributed.run --nproc-per-node {a.gpus}) or drop WORLD_SIZE")
    backend = None
    if ws > 1:
        if a.dist_dry_run:
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        backend = dist.get_backend()
        assert dist.get_world_size() == a.gpus, (dist.get_world_size(), a.gpus)
    return ws, rank, local, backend


def _barrier(ws):
    if ws > 1:
        dist.barrier()


def _max_over_ranks(x: float, ws: int, dev) -> float:
    if ws == 1:
        return x
    t = torch.tensor([x], device=dev if dist.get_backend() == "nccl" else "cpu",
                     dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def _frame_units(net, before, steps):
    """[(replays per frame, plans)] of the plans the timed frames replayed:
    the frame's network composition (with an encoder batch of kb, 1/kb of an
    encoder replay per frame; with decode-ahead, a Bp = 2 pair replay covers
    two frames, a Bp = 1 replay one)."""
    out = []
    for key, (n, plans) in net.plan_units().items():
        d = n - before.get(key, (0, None))[0]
        if d > 0:
            out.append((d / steps, plans))
    return out


def _kernel_profile(units, reps=3):
    """Per-launch HIP-event timing of every network call (eager replay of
    the same plans, same kernels as the graphs), weighted by replays per
    frame: {kind: [launches, flops, ms] per frame}."""
    torch.cuda.synchronize()
    agg = {}
    for wgt, plans in units:
        recs = []
        for _ in range(reps):
            for plan in plans:
                recs += plan.run_timed()
        torch.cuda.synchronize()
        for kind, flops, e0, e1, *_ in recs:
            a = agg.setdefault(kind, [0.0, 0.0, 0.0])
            a[0] += wgt / reps
            a[1] += flops * wgt / reps
            a[2] += e0.elapsed_time(e1) * wgt / reps
    return agg


# k_gemm / k_gemm_pp: A mode = template argument 5; k_gemm_bd (B-direct
# tiles) are dense only
_KFAM = re.compile(r"k_gemm(?:_pp)?<([^>]*)>")


def _algo_bytes(units, kind):
    """Algorithmic HBM bytes per frame of one kernel family (ops.Call.nbytes:
    every operand read once, every output written once), weighted by the
    plans' replays per frame like the FLOPs."""
    return sum(wgt * sum(getattr(c, "nbytes", 0) for c in pl.calls
                         if getattr(c, "kind", None) == kind)
               for wgt, plans in units for pl in plans)


def _family(name: str):
    """Roofline family of a network kernel name (None: not a network kernel)."""
    m = _KFAM.search(name)
    if "k_gemm_bd<" in name:
        return "gemm.dense"
    if m:
        return "gemm.dense" if m.group(1).split(",")[4].strip() == "0" else "gemm.conv"
    if "k_conv3_halo" in name:             # the halo-reuse conv tiles (net_gemm_t6.hip)
        return "gemm.conv"
    if "k_splitk_reduce" in name:
        return "gemm.dense"
    if "k_attn" in name:
        return "s3n_attention"
    if "k_layernorm" in name:
        return "s3n_layernorm"
    return None


def bench_in_window(model, dev, steps, warmup, kb, enc_ahead, decode_ahead, main_priority):
    """Kernel durations INSIDE a frame loop: a second
    frontend with the headline's configuration runs `steps` frames of
    another synthetic sequence under a torch.profiler (roctracer) kernel
    trace, encoder side stream and main chain running concurrently as in the
    timed region; per frame: {family: [launches, ms, executed GFLOP]}.
    The trace slows the host a little, so this window is not the headline;
    the kernels' own durations are what it measures."""
    from torch.profiler import ProfilerActivity, profile
    from splatt3r_amd.slam import Frontend
    from splatt3r_amd.synthetic import tum_like_sequence
    look = kb + max(1, enc_ahead or 1)
    n = warmup + 1 + steps
    frames = tum_like_sequence(n + look + 1, H, W, seed=300, step_px=2.0, device=dev)
    fe = Frontend(model, device=dev, spatial_stride=4, render=True, enc_batch=kb,
                  enc_ahead=enc_ahead, decode_ahead=decode_ahead, main_priority=main_priority)
    nxt = lambda i: [frames[j] for j in range(i + 1, min(i + 1 + look, frames.shape[0]))]
    try:
        for i in range(warmup + 1):
            fe.step(i, frames[i], next_img=nxt(i))
        fe.drain()
        torch.cuda.synchronize()
        units0 = model.encoder.plan_units()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for i in range(warmup + 1, n):
                fe.step(i, frames[i], next_img=nxt(i))
            fe.drain()
            torch.cuda.synchronize()
        units = _frame_units(model.encoder, units0, steps)
    finally:
        fe.close()
    fam = {}
    for e in prof.events():
        if "CUDA" not in str(e.device_type):
            continue
        k = _family(e.name)
        if k is None:
            continue
        f = fam.setdefault(k, [0.0, 0.0, 0.0])
        if "k_splitk_reduce" not in e.name:
            f[0] += 1.0 / steps
        f[1] += e.device_time_total / 1e3 / steps
    for wgt, plans in units:
        for pl in plans:
            for c in pl.calls:
                k = getattr(c, "kind", None)
                if k in fam:
                    fam[k][2] += wgt * c.flops / 1e9
    return fam


def _kernel_trace(units, reps=5):
    """{family: [launches per frame, ms per frame]} of the network kernels:
    a torch.profiler (roctracer) kernel trace of `reps` serial replays of
    every plan's HIP graph (the graphs the frontend replays per frame), one
    stream, nothing else running -- the per-kernel durations a rocprofv3
    kernel trace of the bench reports (its streams run serialised too), with
    no event packets between the kernels.  gemm.dense / gemm.conv = k_gemm
    by its A-operand mode (template argument 5); split-K reduces are timed
    with the dense family (the conv launches do not split at these shapes)."""
    from torch.profiler import ProfilerActivity, profile
    fam = {}
    for wgt, plans in units:
        for pl in plans:
            pl.replay()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                for pl in plans:
                    pl.replay()
            torch.cuda.synchronize()
        for e in prof.events():
            if "CUDA" not in str(e.device_type):
                continue
            k = _family(e.name)
            if k is None:
                continue
            f = fam.setdefault(k, [0.0, 0.0])
            if "k_splitk_reduce" not in e.name:
                f[0] += wgt / reps
            f[1] += e.device_time_total / 1e3 * wgt / reps
    return fam


def _pmc_traffic(kind: str):
    """HBM bytes per launch of the roofline kernel family, from the newest
    committed PMC summary (profiles/*_pmc_traffic.json, written by
    gpurun_traffic.sh: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE
    passes over one-frame replays, FETCH_SIZE x2 per the gfx950 note).
    PMC counters cannot be read inside a timed run, so this is the
    counter pass of the same kernels, named by file."""
    import glob
    fam = {"gemm.dense": "gemm_dense", "gemm.conv": "gemm_conv"}.get(kind)
    paths = sorted(glob.glob(os.path.join(REPO, "profiles", "*_pmc_traffic.json")))
    if not fam:
        return None
    d = None
    for path in reversed(paths):          # the newest summary that has the family
        with open(path) as fh:
            d = json.load(fh)["families"].get(fam)
        if d:
            paths = [path]
            break
    if not d:
        return None
    return {"bytes_per_launch": d["bytes_per_launch"], "bytes_per_frame": d["bytes_per_frame"],
            "read_bytes_per_frame": d["read_bytes_per_frame"],
            "write_bytes_per_frame": d["write_bytes_per_frame"],
            "source": os.path.relpath(paths[-1], REPO)}


def cpu_baseline(model_cfg, seed, frames, n_frames):
    """The CPU restatement (oracle/, `port`) of one tracked frame: torch-CPU
    network forward (oracle/net_ref.py) + C matching + C rasterizer on its
    outputs, timed on this host's cores."""
    import oracle
    import oracle.net_ref as R
    from splatt3r_amd import weights as Wt
    sd = {k: v.float().cpu() for k, v in
          Wt.prng_state_dict(model_cfg, seed, torch.device("cuda")).items()}
    sd = Wt.tie_symmetric(sd)
    torch.cuda.synchronize()
    threads = torch.get_num_threads()
    with torch.no_grad():
        fk, pk = R.encode(sd, model_cfg, frames[0].cpu())
    times = []
    for i in range(n_frames):
        img = frames[1 + i].cpu()
        t0 = time.perf_counter()
        r1, r2 = R.frame_forward(sd, model_cfg, img, fk, pk)
        X11, X21 = r1["pts3d"].numpy(), r2["pts3d"].numpy()
        D11, D21 = r1["desc"].numpy(), r2["desc"].numpy()
        oracle.match(X11, X21, D11, D21)
        _cpu_render(oracle, r1, r2, img, frames[0].cpu(), threads)
        times.append(time.perf_counter() - t0)
    return dict(value=n_frames / sum(times), unit="frames/s", cores=threads, kind="port",
                sample=f"{n_frames} tracked frame(s) 512x384: torch-CPU network (oracle/net_ref.py,"
                       f" fp32) + C matching + C rasterizer (oracle/), {sum(times):.1f} s")


def _cpu_render(oracle, r1, r2, img, kimg, threads):
    from splatt3r_amd.synthetic import quat_xyzw_to_rot
    cat = lambda k, c: torch.cat([r1[k].reshape(-1, c), r2[k].reshape(-1, c)]).numpy()
    means = cat("means", 3) * 10.0
    sc = cat("scales", 3)
    Rm = quat_xyzw_to_rot(cat("rotations", 4))
    cov = np.einsum("nij,nj,nkj->nik", Rm, sc * sc, Rm) * 100.0
    iu = np.triu_indices(3)
    cov6 = cov[:, iu[0], iu[1]]
    rgb = lambda t: (t[0].permute(1, 2, 0).reshape(-1, 3).numpy() * 0.5 + 0.5).clip(0, 1)
    sh = cat("sh", 3) + (np.concatenate([rgb(img), rgb(kimg)]) - 0.5) / 0.28209479177387814
    opac = cat("opacities", 1)[:, 0]
    f = float(max(H, W))
    tx, ty = (W / 2) / f, (H / 2) / f
    near, far = 1.0, 10000.0
    Pm = np.zeros((4, 4), np.float32)
    Pm[0, 0], Pm[1, 1] = 1 / tx, 1 / ty
    Pm[3, 2], Pm[2, 2], Pm[2, 3] = 1, far / (far - near), -(far * near) / (far - near)
    settings = dict(image_height=H, image_width=W, tanfovx=tx, tanfovy=ty, bg=[0, 0, 0],
                    scale_modifier=1.0, viewmatrix=np.eye(4, dtype=np.float32).ravel(),
                    projmatrix=Pm.T.ravel(), sh_degree=0, campos=[0, 0, 0])
    oracle.raster(settings, means, opac, shs=sh.reshape(-1, 1, 3), cov3D_precomp=cov6,
                  nthreads=threads)


def bench_backend(model, dev, steps, rank, ws=1, enc_batch=1, enc_ahead=None, decode_ahead=False,
                  main_priority=None, warmup=5):
    """The frontend with the reference backend running concurrently
    (config/base.yaml single_thread: False, main.py:122-190): keyframe tasks
    (retrieval update, add_factors over consecutive + retrieved keyframes,
    GN) on a worker thread and its own lowest-priority HIP stream
    (backend.worker_stream_priority).  The frontend runs the HEADLINE's
    configuration (encoder lookahead batch, frames queued ahead, decode-ahead,
    main-chain priority).  Two rates: `frames_per_s` over the frontend loop's
    window with the backend running beside it -- the reference's FPS window
    (main.py:363-535: FPS = i / (time - fps_timer), the backend process is
    not waited for) -- and `frames_per_s_drained`, from the first timed frame
    until the backend has also drained its queue.  With ws > 1 the
    backend's keyframe-pair batches are sharded (pairs.PairShard: keyframe
    features broadcast from rank 0's worker thread, each pair's two decode
    directions on ranks u mod ws, idx / valid / Q gathered back to rank 0);
    ranks > 0 serve the tasks (pairs.serve_backend) until rank 0 stops."""
    from splatt3r_amd.backend import Backend, worker_stream_priority
    from splatt3r_amd.frame import Keyframes
    from splatt3r_amd.pairs import PairShard, serve_backend
    from splatt3r_amd.slam import Frontend
    from splatt3r_amd.synthetic import tum_like_sequence
    for b in range(1, 5):                   # backend pair plans, built before timing
        model.encoder.pair_plan(b, H, W, tag="backend")
    if rank > 0:
        sh = serve_backend(model, dev)
        return {"rank": rank, "served_units": sh.stats["units"]}
    kb = max(1, int(enc_batch))
    look = kb + max(1, enc_ahead or 1)
    n = warmup + 1 + steps
    frames = tum_like_sequence(n + look + 1, H, W, seed=100 + rank, step_px=2.0, device=dev)
    shard = PairShard(model, dev) if ws > 1 else None
    be = Backend(model, Keyframes(), device=dev, shard=shard)
    be.start_worker()
    fe = Frontend(model, device=dev, spatial_stride=4, render=True, backend=be, enc_batch=kb,
                  enc_ahead=enc_ahead, decode_ahead=decode_ahead, main_priority=main_priority)
    nxt = lambda i: [frames[j] for j in range(i + 1, min(i + 1 + look, frames.shape[0]))]
    try:
        for i in range(warmup + 1):         # frame 0 = INIT, then warm-up frames
            fe.step(i, frames[i], next_img=nxt(i))
        fe.drain()
        be.wait()
        torch.cuda.synchronize()
        fe.reserve_memory()
        s0, b0 = dict(fe.stats), dict(be.stats)
        t0 = time.perf_counter()
        for i in range(warmup + 1, n):
            fe.step(i, frames[i], next_img=nxt(i))
        fe.drain()
        torch.cuda.synchronize()
        t_front = time.perf_counter() - t0
        opt_front = be.stats["optimized"] - b0.get("optimized", 0)
        be.wait()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
    finally:
        be.stop()                           # also releases ranks > 0 (OP_STOP)
        fe.close()
    st = {k: fe.stats[k] - s0[k] for k in fe.stats}
    bs = {k: be.stats[k] - b0.get(k, 0) for k in be.stats if isinstance(be.stats[k], int)}
    out = {"frames_per_s": steps / t_front, "frames_per_s_drained": steps / t,
           "frames_per_s_definition": "frames_per_s: frames / the frontend loop's wall time "
                                      "with the backend worker running beside it (the "
                                      "reference's FPS window, main.py:363-535); "
                                      "frames_per_s_drained: until the backend queue is empty too",
           "steps": steps, "keyframes": st["keyframes"], "tracked": st["tracked"],
           "keyframe_rate": st["keyframes"] / steps, "backend_tasks": bs["optimized"],
           "backend_tasks_done_in_frontend_window": opt_front,
           "factor_graph_edges": be.stats["edges"],
           "retrieval_candidates": bs["retrieval_candidates"],
           "worker_stream_priority": worker_stream_priority(),
           "frontend_config": {"encoder_batch": kb, "encoder_ahead": enc_ahead,
                               "decode_ahead": decode_ahead, "main_priority": main_priority},
           "mode": "single_thread: False (worker thread + lowest-priority HIP stream, same GPU)"}
    if shard is not None:
        out["mode"] += (f"; keyframe-pair batches sharded over {ws} ranks (PairShard, directed "
                        f"units u -> rank u mod {ws})")
        out["rank0_units"] = shard.stats["units"]
    return out


def _dry_match_dir(fa, pa, fb, pb, sa, sb):
    """--dist-dry-run stand-in for splatt3r_match_directed: deterministic per
    directed unit (keyframe ids carried in the features), whatever batch."""
    hw = int(sa[0].reshape(-1)[0]) * int(sa[0].reshape(-1)[1])
    ka, kb = fa[:, 0, 0].long(), fb[:, 0, 0].long()
    ar = torch.arange(hw)
    idx = (ar[None] * (ka[:, None] + 1) + kb[:, None]) % hw
    q = (1.0 + (ar[None] % 5).float() + ka[:, None].float())[..., None]
    return idx, ((ar[None] + kb[:, None]) % 3 != 0)[..., None], q, q + 1.0


_DRY_CAP = 10


def _dry_map(pairs, poses, hp):
    """--dist-dry-run stand-in for PairShard._map_records: 3..9 records per
    edge of _DRY_CAP rows, valued from the edge, its pose and the filters."""
    buf = torch.full((len(pairs), _DRY_CAP, 13), -7.0)
    cnt = torch.zeros(len(pairs), dtype=torch.int64)
    for p, (i, j) in enumerate(pairs):
        n = 3 + (5 * i + j) % 7
        base = float(poses[i].sum()) + float(hp[1]) + 10 * i + j
        buf[p, :n] = base + torch.arange(n * 13, dtype=torch.float32).reshape(n, 13) * 0.5
        cnt[p] = n
    return buf, cnt


def _dry_frames(n_kf, H=32, W=48):
    import lietorch
    from splatt3r_amd.frame import Frame
    from splatt3r_amd.net import positions
    out = []
    for k in range(n_kf):
        f = Frame(k, torch.zeros(1, 3, H, W), torch.tensor([[H, W]]),
                  torch.tensor([[H, W]]), T_WC=lietorch.Sim3.Identity(1))
        f.feat = torch.full((1, 6, 8), float(k))
        f.pos = positions(1, 2, 3, "cpu")
        out.append(f)
    return out


def _dry_shard_check(ws, rank, n_kf=6):
    """--dist-dry-run: the sharded-unit self-check of `bench.py --gpus N`
    (pairs.bench_pairs shard_check / map_shard_check) on the CPU stand-ins:
    rank 0 gathers a pair batch and a map refresh over the ranks, then
    re-decodes units / edges other ranks produced and compares bit for bit."""
    from splatt3r_amd.pairs import PairShard
    sh = PairShard(None, "cpu", match_dir_fn=_dry_match_dir, map_fn=_dry_map,
                   map_cap=lambda pairs, hp: _DRY_CAP)
    if rank > 0:
        sh.serve()
        return None
    for k, f in enumerate(_dry_frames(n_kf)):
        if ws > 1:
            sh.broadcast_keyframe(k, f)
        else:
            sh.register_local(k, f)
    pairs = [(k - d, k) for k in range(1, n_kf) for d in (1, 2) if k - d >= 0]
    ii, jj = [p[0] for p in pairs], [p[1] for p in pairs]
    if ws == 1:
        # one rank: the stand-in symmetric match is the two directed units
        sh.match_fn = lambda fi, pi, fj, pj, si, sj: (
            lambda a, b: (a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3]))(
            _dry_match_dir(fi, pi, fj, pj, si, sj), _dry_match_dir(fj, pj, fi, pi, sj, si))
    got = sh.match_pairs(ii, jj)
    poses = torch.arange(n_kf * 8, dtype=torch.float32).reshape(n_kf, 8) * 0.1
    mi = list(range(n_kf))
    mj = [k + 1 if k + 1 < n_kf else k - 1 for k in mi]
    recs = sh.refresh_map(mi, mj, poses, spatial_stride=4, opacity_threshold=0.0)
    sh.stop()
    u = sh.check_units(ii, jj, got, max_units=4)
    m = sh.check_map(mi, mj, poses, (4.0, 0.98, 1.0, 1.5, 0.0), recs, max_pairs=2)
    return {"pairs": u, "map": m, "equal": u["equal"] and m["equal"]}


def _dry_backend(ws, rank, n_kf=9):
    """--dist-dry-run: the sharded backend's protocol on the CPU (gloo): rank
    0's Backend on its worker thread with a PairShard, ranks > 0 in
    pairs.serve_backend; network, retrieval and GN are deterministic
    stand-ins (no GPU work).  Returns the edge / unit counts."""
    import lietorch
    from splatt3r_amd.backend import Backend
    from splatt3r_amd.frame import Frame, Keyframes
    from splatt3r_amd.net import positions
    from splatt3r_amd.pairs import PairShard, serve_backend

    match_dir = _dry_match_dir

    if rank > 0:
        sh = serve_backend(None, "cpu", match_dir_fn=match_dir)
        return {"rank": rank, "units": sh.stats["units"], "keyframes": sh.stats["keyframes"]}

    class _Retrieval:
        def update(self, frame, add_after_query=True, k=3, min_thresh=0.0):
            return [j for j in (frame.frame_id - 2, frame.frame_id - 3) if j >= 0]

    class _Be(Backend):
        def _solve(self):                   # no GN without a GPU
            return None

    sh = PairShard(None, "cpu", match_dir_fn=match_dir)
    be = _Be(None, Keyframes(), device="cpu", retrieval=_Retrieval(), shard=sh)
    be.start_worker()
    try:
        for k in range(n_kf):
            f = Frame(k, torch.zeros(1, 3, 32, 48), torch.tensor([[32, 48]]),
                      torch.tensor([[32, 48]]), T_WC=lietorch.Sim3.Identity(1))
            f.feat = torch.full((1, 6, 8), float(k))
            f.pos = positions(1, 2, 3, "cpu")
            be.keyframes.append(f)
            be.on_keyframe(k, f)
            be.queue_global_optimization(k)
        be.wait()
    finally:
        be.stop()
    return {"keyframes": n_kf, "edges": int(be.factor_graph.ii.numel()),
            "rank0_units": sh.stats["units"], "pairs": sh.stats["pairs"]}


def bench_end_to_end(model, dev, steps, warmup, main_priority=-1, workers=4, writers=3,
                     enc_batch=1, enc_ahead=None, decode_ahead=False, render_async=False):
    """The reference's FPS definition (main.py:363-535): frames / wall time of
    the whole loop, with the host work inside it -- the dataset read (PNG
    decode of 640x480 TUM-layout frames), create_frame's resize_img (PIL
    LANCZOS -> 512x384) + ImgNorm + H2D (dataio.FrameLoader, worker
    threads), the tracking step, and the per-frame gs_init_* / gs_track_*
    PNG write (dataio.RenderWriter, writer threads).  The frames are written
    to a scratch TUM layout before the timed region; the timed region ends
    when every PNG is on disk."""
    import shutil
    import tempfile
    from splatt3r_amd.dataio import FrameLoader, RenderWriter, TUMDataset, write_synthetic_tum
    from splatt3r_amd.slam import Frontend
    root = tempfile.mkdtemp(prefix="s3_tum_")
    try:
        n = warmup + steps + 2 + enc_batch + max(1, enc_ahead or 1)
        write_synthetic_tum(os.path.join(root, "seq"), n, seed=7)
        ds = TUMDataset(os.path.join(root, "seq"))
        writer = RenderWriter(os.path.join(root, "renders"), workers=writers)
        fe = Frontend(model, device=dev, spatial_stride=4, render=True, render_writer=writer,
                      main_priority=main_priority, enc_batch=enc_batch, enc_ahead=enc_ahead,
                      decode_ahead=decode_ahead, render_async=render_async)
        look = enc_batch + max(1, enc_ahead or 1)   # lookahead frames, as the headline
        n = warmup + steps + 1 + look
        loader = FrameLoader(ds, dev, workers=workers, depth=max(2 * workers, look + 2))
        win = [next(loader).consume() for _ in range(look + 1)]   # frames i .. i + look
        t0 = None
        for i in range(warmup + steps + 1):
            if i == warmup + 1:                  # frame 0 = INIT, W warm-up frames
                fe.drain()
                writer.flush()
                fe.reserve_memory()
                torch.cuda.synchronize()
                s0 = dict(fe.stats)
                t0 = time.perf_counter()
            fe.step(i, win[0], next_img=win[1:])
            win = win[1:] + ([next(loader).consume()] if i + look + 1 < n else [])
        fe.drain()
        torch.cuda.synchronize()
        writer.flush()
        t = time.perf_counter() - t0
        st = {k: fe.stats[k] - s0[k] for k in fe.stats}
        fe.close()
        loader.close()
        writer.close()
        written = len(os.listdir(os.path.join(root, "renders")))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return {"frames_per_s": steps / t, "steps": steps, "tracked": st["tracked"],
            "reloc": st["reloc"], "keyframes": st["keyframes"],
            "keyframe_rate": st["keyframes"] / steps, "pngs_written": written,
            "loader_threads": workers, "png_writer_threads": writers,
            "input": "640x480 PNG frames, TUM layout (rgb.txt), synthetic panning texture",
            "includes": "PNG decode + resize_img (PIL LANCZOS) + ImgNorm + H2D, tracking step, "
                        "render D2H + uint8 + PNG encode/write (compress_level 1)"}


def bench_map(dev, n=8_388_608, iters=5, warmup=2, seed=0):
    """C5 full-map render: an n-Gaussian world map (SharedGaussians, filled
    through s3w_map_append in 1M-record batches) rasterized with
    colors_precomp at 960x540 (half of a 1920x1080 viewport), vfov 45,
    near 0.05 / far 100 (visualization.py:467-600).  Synthetic Gaussians in
    a 4 m x 2.5 m x 4 m room in front of the camera."""
    from splatt3r_amd.gaussian_map import SharedGaussians, render_map
    from splatt3r_amd.synthetic import c5_map_batches
    gm = SharedGaussians(max_gaussians=n, device=dev)
    for k, (means, cov, col, op) in enumerate(c5_map_batches(n, seed=seed, device=dev)):
        gm.append(means, cov, col, op, kf_idx=k, opacity_threshold=0.3)
    out = {"map_gaussians": gm.n_gaussians, "image": "960x540", "vfov_deg": 45.0}
    T = np.eye(4, dtype=np.float32)
    import diff_gaussian_rasterization as dgr
    for label, cnt in (("4.19M", n // 2), ("8.39M", n)):
        for _ in range(warmup):
            render_map(gm, T, 960, 540, 45.0, n=cnt)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            render_map(gm, T, 960, 540, 45.0, n=cnt)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        out[label] = {"ms": ms, "msplats_per_s": cnt / (ms * 1e-3) / 1e6,
                      "instances": int(dgr.last_num_rendered)}
    return out


def _encodes(net) -> int:
    """Images encoded so far by the network's encoder plans (replays x B)."""
    return sum(ep.calls * key[0] for key, ep in net._enc.items())


def _critical_path(fe, net_events, wall_s, steps, ev_t0=None):
    """Where the frame period goes, from the HIP events of the timed region
    (one stream each): the main chain of frame i (Frontend.spans "main",
    decoder + heads + matching + GN + render on the main stream) and the
    pair-plan replays inside it (Splatt3RNet.events "pair").  The four terms
    sum to ms_per_step by construction:
      main_network_ms   decoder + heads replays on the main stream
      main_other_ms     the rest of the main chain (matching, GN, world
                        records, render, read-back, waits on the encoder)
      main_idle_ms      the main stream between two frames' chains (host
                        issue of the next frame)
      edge_ms           before the first chain and after the last (first
                        issue, final drain + synchronise)
    The encoder batches (side stream, overlapped) are reported beside."""
    mains = [(e0, e1) for tag, _, e0, e1 in fe.spans if tag == "main"]
    encs = [(e0, e1) for tag, _, e0, e1 in fe.spans if tag == "enc" and e0 is not None]
    span = mains[0][0].elapsed_time(mains[-1][1])
    busy = sum(e0.elapsed_time(e1) for e0, e1 in mains)
    pair = sum(e0.elapsed_time(e1) for tag, e0, e1 in net_events if tag == "pair")
    enc = sum(e0.elapsed_time(e1) for e0, e1 in encs)
    wall = wall_s * 1e3
    out = {"main_network_ms": pair / steps, "main_other_ms": (busy - pair) / steps,
           "main_idle_ms": (span - busy) / steps, "edge_ms": (wall - span) / steps,
           "encoder_side_stream_ms": enc / steps,
           "source": "HIP events on the main / encoder streams over the timed region"}
    out["sum_ms"] = (out["main_network_ms"] + out["main_other_ms"] + out["main_idle_ms"]
                     + out["edge_ms"])
    # the edge, split: timer start -> first chain, and the encoder side
    # stream's work still running after the last chain (ms, whole region)
    if ev_t0 is not None:
        out["edge_head_ms_total"] = round(ev_t0.elapsed_time(mains[0][0]), 3)
    if encs:
        # the encoder side stream's work still running after the last chain
        # (0 when the last encode ended first), and the signed offset of the
        # last encode's end from the last chain's end
        off = mains[-1][1].elapsed_time(max(
            (e1 for _, e1 in encs), key=lambda e: mains[0][0].elapsed_time(e)))
        out["enc_after_last_chain_ms_total"] = round(max(0.0, off), 3)
        out["last_enc_end_minus_last_chain_end_ms"] = round(off, 3)
    # main-stream idle between consecutive frames' chains, per frame
    out["idle_gaps_ms"] = [round(a[1].elapsed_time(b[0]), 3) for a, b in zip(mains, mains[1:])]
    # gaps over 1 ms: which frame, and how the next chain's start sits
    # against the nearest encoder batch end (~0 => it waited on the encoder)
    ids = [i for tag, i, _, _ in fe.spans if tag == "main"]
    big = []
    for k, g in enumerate(out["idle_gaps_ms"]):
        if g > 1.0:
            b0 = mains[k + 1][0]
            near = min((e1.elapsed_time(b0) for _, e1 in encs), key=abs, default=None)
            big.append({"frame": ids[k + 1], "gap_ms": g,
                        "chain_start_minus_nearest_enc_end_ms":
                            None if near is None else round(near, 3)})
    out["big_gaps"] = big
    return out


def _spec_flops(net, ahead, kind, H, W):
    """FLOPs of family `kind` in the decode-ahead slots that were computed and
    never used (paired - used; one slot = half of a Bp = 2 tracker replay)."""
    pp = net._pair.get((2, H, W, False, None))
    if pp is None:
        return 0.0
    fl = sum(c.flops for plan in (pp.decoder_plan, pp.head_plan) for c in plan.calls
             if getattr(c, "kind", None) == kind)
    return max(0, ahead["paired"] - ahead["used"]) * fl / 2


def bench_live(model, dev, frames, steps, warmup, main_priority=-1):
    """A live camera (RealSense / webcam / MP4 sources, dataloader.py:151-231)
    has no lookahead: each frame is encoded, decoded against the keyframe,
    matched, tracked and rendered alone (encoder batch 1, no decode-ahead, no
    next-frame pipelining), then the render is read back to the host.
    Per-frame latency = frame handed to the frontend -> render on the host
    (device synchronised); frames/s = frames / sum of latencies."""
    from splatt3r_amd.slam import Frontend
    fe = Frontend(model, device=dev, spatial_stride=4, render=True, enc_batch=1,
                  decode_ahead=False, main_priority=main_priority)
    lat = []
    prof = None
    if os.environ.get("S3_PROFILE_LIVE"):      # host cProfile of the timed frames (diagnostic)
        import cProfile
        prof = cProfile.Profile()
    try:
        for i in range(warmup + 1 + steps):
            if prof is not None and i == warmup + 1:
                prof.enable()
            if i == warmup + 1:
                fe.reserve_memory()
            torch.cuda.synchronize()
            if i == warmup + 1:
                s0 = dict(fe.stats)
            t0 = time.perf_counter()
            fe.step(i, frames[i])
            fe.last_render                    # waits for the render's host copy
            torch.cuda.synchronize()
            if i > warmup:
                lat.append(time.perf_counter() - t0)
        st = {k: fe.stats[k] - s0[k] for k in fe.stats}
    finally:
        fe.close()
    if prof is not None:
        import io
        import pstats
        import sys
        prof.disable()
        out = io.StringIO()
        pstats.Stats(prof, stream=out).sort_stats("tottime").print_stats(25)
        print(out.getvalue(), file=sys.stderr)
    ms = np.sort(np.array(lat) * 1e3)
    return {"frames_per_s": len(lat) / float(np.sum(lat)), "steps": len(lat),
            "latency_ms": {"p50": float(np.percentile(ms, 50)),
                           "p99": float(np.percentile(ms, 99)),
                           "mean": float(ms.mean()), "max": float(ms[-1])},
            "tracked": st["tracked"], "keyframes": st["keyframes"], "reloc": st["reloc"],
            "config": "encoder batch 1, no decode-ahead, no next-frame pipelining, frame "
                      "resident in HBM, render read back to host memory"}


def _dry_run(a, ws, rank):
    """--dist-dry-run: the launch / rendezvous / timing / sharding skeleton on
    the CPU (gloo), no GPU work: every rank takes its pairs of a fixed pair
    list (pairs.shard, p -> rank p mod W), the timed region is bracketed by
    barriers, and rank 0 prints the JSON line with the max over ranks."""
    from splatt3r_amd.pairs import shard
    pairs = [(k - d, k) for k in range(1, 9) for d in (1, 2, 3, 4) if k - d >= 0]
    _barrier(ws)
    t0 = time.perf_counter()
    mine = shard(pairs, ws, rank)
    acc = sum(i * 31 + j for i, j in mine)
    _barrier(ws)
    t = _max_over_ranks(time.perf_counter() - t0, ws, "cpu")
    tot = torch.tensor([acc, len(mine)], dtype=torch.int64)
    if ws > 1:
        dist.all_reduce(tot)
    # the sharded backend leg's protocol (bench_backend with ws > 1)
    be = _dry_backend(ws, rank) if not a.no_backend else None
    units = torch.tensor([be["units"] if rank else be["rank0_units"]] if be else [0],
                         dtype=torch.int64)
    if ws > 1:
        dist.all_reduce(units)
    # the sharded-unit self-check the GPU run prints as shard_check
    chk = _dry_shard_check(ws, rank)
    if rank == 0:
        line = {"metric": "dist-dry-run", "n_gpus": ws, "world_size": ws,
                "dist_backend": dist.get_backend() if ws > 1 else None,
                "pairs": len(pairs), "pairs_covered": int(tot[1]),
                "checksum": int(tot[0]), "t_max_s": t, "shard_check": chk}
        if be is not None:
            line["backend"] = dict(be, units_all_ranks=int(units[0]),
                                   mode="Backend worker thread + PairShard over the ranks "
                                        "(serve_backend on ranks > 0), CPU stand-ins")
        print(json.dumps(line), flush=True)
    if ws > 1:
        dist.destroy_process_group()


def _prewarm(local):
    """One-shot warm process before this one touches the GPU (a child
    process, started and waited for here; S3_BENCH_PREWARM=0 skips it).  On
    a fresh box the first GPU process pays a one-time ~6 ms stall inside its
    timed window (`profiles/r05first_run_gap.log`: first runs 184-189
    frames/s with one 5.9 ms gap, later runs 194-199 without), which a
    trivial torch process run first removes (`profiles/r05first_run_gap.log`,
    last call): the ROCm libraries such a process loads are then paged in.
    The timed region itself is unchanged."""
    import subprocess
    code = ("import torch; d = torch.device('cuda', %d); a = torch.randn(4, 4, device=d); "
            "b = torch.linalg.inv_ex(a)[0] @ a; torch.cuda.synchronize(d)" % local)
    try:
        subprocess.run([sys.executable, "-c", code], timeout=300, check=False,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    except (OSError, subprocess.SubprocessError):
        pass


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    a = _args(argv)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one process per GPU, started here before anything touches the GPU
        sys.exit(_spawn(a, argv))
    ws, rank, local, backend = _dist(a)
    if a.dist_dry_run:
        return _dry_run(a, ws, rank)
    prewarmed = os.environ.get("S3_BENCH_PREWARM", "1") != "0"
    if prewarmed:
        _prewarm(local)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    # the frame loop's dedicated streams first, before anything takes a
    # stream from torch's pool: each gets a hardware queue of its own
    from splatt3r_amd import _lib
    _lib.reserve_frame_streams(dev)
    from splatt3r_amd.slam import Frontend
    from splatt3r_amd.splatt3r_utils import load_splatt3r
    from splatt3r_amd.synthetic import tum_like_sequence
    from splatt3r_amd.weights import FULL

    seed = 1234
    model = load_splatt3r(None, device=dev, cfg=FULL, seed=seed, symmetric=True)
    nfr = a.warmup + a.steps + 1
    kb = a.enc_batch
    a.enc_ahead = a.enc_ahead or None
    plan = plan_encodes(a.steps, a.warmup, kb, a.enc_ahead, pipeline=not a.no_pipeline)
    look = plan["look"]
    if look > 16:
        raise SystemExit("--enc-batch + --enc-ahead must be <= 16")
    # a fixed length past the timed frames: the texture (and so every frame)
    # does not depend on the lookahead configuration (the same sequence as
    # rounds 1-3); lookahead images past it (encoded by the last timed steps,
    # never tracked) repeat its last frame
    frames = tum_like_sequence(nfr + 16, H, W, seed=rank, step_px=2.0, device=dev)
    if plan["frames_needed"] > frames.shape[0]:
        pad = plan["frames_needed"] - frames.shape[0]
        frames = torch.cat([frames, frames[-1:].expand(pad, *frames.shape[1:])])
    fe = Frontend(model, device=dev, spatial_stride=4, render=True, enc_batch=kb,
                  main_priority=a.main_priority, late_prefetch=a.late_prefetch,
                  decode_ahead=a.decode_ahead, enc_ahead=a.enc_ahead,
                  render_async=a.render_async, deferred_render=a.deferred_render)
    # lookahead only below plan["cap_warm"] in warm-up, plan["cap"] when timed
    cap = [plan["cap_warm"]]

    def nxt(i):
        if a.no_pipeline:
            return None
        hi = i + 1 + look if cap[0] is None else min(i + 1 + look, cap[0])
        return [frames[j] for j in range(i + 1, hi)]

    # every encoder batch size the run can queue (a partial last batch when
    # --steps is not a multiple of --enc-batch, lookahead tails of the other
    # legs): plans built and captured here, never inside a timed region
    for b in range(1, kb + 1):
        model.encoder.encoder_plan(b, H, W)
    for i in range(a.warmup + 1):          # frame 0 = INIT, then W tracked frames
        fe.step(i, frames[i], next_img=nxt(i))
    fe.drain()
    torch.cuda.synchronize()
    if not a.no_pipeline:
        assert fe._next_enc == plan["next_enc_before"], (fe._next_enc, plan["next_enc_before"])
    cap[0] = plan["cap"]
    s0 = dict(fe.stats)
    model.encoder.events = []
    fe.spans = None if a.no_spans else []
    ahead0 = dict(model.encoder.ahead_counts)
    units0 = model.encoder.plan_units()
    enc0 = _encodes(model.encoder)
    if os.environ.get("S3_RESERVE", "1") != "0":
        fe.reserve_memory()                # plans are captured: grow the allocator's cache now
    if os.environ.get("S3_GC_FREEZE", "1") != "0":
        # the warm-up's objects (plans, frames, tensors) leave the collected
        # generations: a garbage collection inside the timed region then
        # walks only what the timed frames allocate
        import gc
        gc.collect()
        gc.freeze()
    hprof = None
    if os.environ.get("S3_PROFILE_HOST"):  # host cProfile of the timed region (diagnostic)
        import cProfile
        hprof = cProfile.Profile()
    _barrier(ws)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev_t0 = None
    if fe.spans is not None:
        ev_t0 = torch.cuda.Event(enable_timing=True)
        ev_t0.record(fe.main_stream or torch.cuda.current_stream(dev))
    if hprof is not None:
        hprof.enable()
    host_ms = []
    phases = None
    if os.environ.get("S3_HOST_PHASES"):     # host time between tracker phases (diagnostic)
        phases = []
        fe.tracker.mark = lambda name: phases.append((len(host_ms), name, time.perf_counter()))
    if os.environ.get("S3_STALL_TRACE"):
        # diagnostic: a watchdog dumps every thread's Python stack when the
        # host spends more than S3_STALL_TRACE ms in a frame's issue phases
        # (step start -> GN queued, GN done -> step end; the GN wait itself
        # is not armed)
        import faulthandler
        lim = float(os.environ["S3_STALL_TRACE"]) * 1e-3
        prev = getattr(fe.tracker, "mark", None)

        def _mark(name, prev=prev):
            if prev is not None:
                prev(name)
            if name in ("step_begin", "gn_done", "step_end"):
                # (step_end arms the window between steps: the bench loop)
                faulthandler.dump_traceback_later(lim, exit=False)
            elif name == "spec_queued":
                faulthandler.cancel_dump_traceback_later()
        fe.tracker.mark = _mark
    hev = None
    if os.environ.get("S3_HOST_EVENTS"):
        # diagnostic: every host phase mark also records a timing event on an
        # idle stream (it completes when the host records it: host time on
        # the device clock), and the tracker marks the device time its first
        # GN chunk ends (gpu_mark on the main stream)
        hev, idle = [], torch.cuda.Stream(dev)
        prev_h = getattr(fe.tracker, "mark", None)

        def _hmark(name, prev=prev_h):
            if prev is not None:
                prev(name)
            e = torch.cuda.Event(enable_timing=True)
            e.record(idle)
            hev.append((len(host_ms), "host:" + name, e))

        def _gmark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(dev))
            hev.append((len(host_ms), "gpu:" + name, e))
        fe.tracker.mark = _hmark
        fe.tracker.gpu_mark = _gmark
    if os.environ.get("S3_WAIT_EVENTS"):   # device time of the waits on encoder batches (diagnostic)
        fe.wait_log = []
    ms0 = torch.cuda.memory_stats(dev)
    # Python garbage collections inside the timed region: (generation, step,
    # pause ms) -- a host pause of the frame loop that the critical path
    # would show as an idle gap
    import gc
    gc_log, gc_t = [], [0.0]

    def _gc_cb(phase, info):
        if phase == "start":
            gc_t[0] = time.perf_counter()
        else:
            gc_log.append((info.get("generation"), len(host_ms),
                           round((time.perf_counter() - gc_t[0]) * 1e3, 3)))
    gc.callbacks.append(_gc_cb)
    last = None
    for i in range(a.warmup + 1, nfr):
        h0 = time.perf_counter()
        last = fe.step(i, frames[i], next_img=nxt(i))
        host_ms.append(round((time.perf_counter() - h0) * 1e3, 3))
    fe.drain()                             # every frame's render issued
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    gc.callbacks.remove(_gc_cb)
    if hprof is not None:
        import io
        import pstats
        hprof.disable()
        for key in ("tottime", "cumulative"):
            out = io.StringIO()
            pstats.Stats(hprof, stream=out).sort_stats(key).print_stats(45)
            print(out.getvalue(), file=__import__("sys").stderr)
    _barrier(ws)
    t_max = _max_over_ranks(t, ws, dev)
    if a.dump_outputs and rank == 0 and last is not None:
        dump_outputs(a.dump_outputs, last, fe.last_render)
    ev = model.encoder.events
    model.encoder.events = None
    encodes = _encodes(model.encoder) - enc0
    crit = _critical_path(fe, ev, t, a.steps, ev_t0) if fe.spans is not None else None
    if os.environ.get("S3_STALL_TRACE"):
        import faulthandler
        faulthandler.cancel_dump_traceback_later()
    if phases is not None or os.environ.get("S3_STALL_TRACE") or hev is not None:
        fe.tracker.mark = None
    if hev is not None:
        fe.tracker.gpu_mark = None
        if crit is not None and ev_t0 is not None:
            # per step: [(mark, ms after the timed region's start on the device clock)]
            steps = {}
            for k, name, e in hev:
                steps.setdefault(k, []).append((name, round(ev_t0.elapsed_time(e), 3)))
            mains = [(i, e0, e1) for tag, i, e0, e1 in fe.spans if tag == "main"]
            for n, (i, e0, e1) in enumerate(mains):
                if n in steps:
                    steps[n] += [("chain_start", round(ev_t0.elapsed_time(e0), 3)),
                                 ("chain_end", round(ev_t0.elapsed_time(e1), 3))]
            crit["host_device_marks"] = steps
    if phases is not None:
        if crit is not None:
            by = {}
            for k, name, tt in phases:
                by.setdefault(k, []).append((name, tt))
            crit["host_phases_ms"] = {k: [(n, round((t1 - v[0][1]) * 1e3, 3)) for n, t1 in v]
                                      for k, v in by.items()}
    if crit is not None:
        crit["host_step_ms"] = host_ms      # host time inside each Frontend.step
        # garbage collections in the timed region: [generation, step, pause ms]
        crit["gc_pauses"] = gc_log
        if fe.wait_log is not None:
            # waits on encoder batches that held the stream > 0.5 ms: [what, frame, ms]
            crit["encoder_waits"] = [(w, i, round(e0.elapsed_time(e1), 3))
                                     for w, i, e0, e1 in fe.wait_log
                                     if e0.elapsed_time(e1) > 0.5]
            fe.wait_log = None
        # device allocations (caching-allocator segments) made by the timed frames
        ms1 = torch.cuda.memory_stats(dev)
        crit["segments_allocated"] = {
            k: ms1.get(f"segment.{k}.allocated", 0) - ms0.get(f"segment.{k}.allocated", 0)
            for k in ("small_pool", "large_pool")}
    fe.spans = None
    net_ms = sum(e0.elapsed_time(e1) for _, e0, e1 in ev) / a.steps
    st = {k: fe.stats[k] - s0[k] for k in fe.stats}
    ahead = {k: model.encoder.ahead_counts[k] - ahead0[k] for k in ahead0}

    frames_all = a.steps * ws
    value = frames_all / t_max
    P_frame = 2 * H * W
    result = {
        "metric": "SLAM frames/sec (TUM fr1_desk, 512px) + Msplats/sec rasterized; 1->8 GPU",
        "value": value, "unit": "frames/s", "n_gpus": ws, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": t_max / a.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "fp16 MFMA (fp32 accumulate); fp32 geometry/raster",
        "data": "synthetic: panning smooth-noise 512x384 sequence (TUM fr1_desk shape), "
                "portable-PRNG weights of the MASt3R ViT-L/Base/DPT-Gaussian architecture "
                "(no dataset or checkpoint offline: keyframe rate and match fractions are "
                "those of this sequence, not of fr1_desk)",
        "value_definition": "frames tracked / wall time with the frames resident in HBM (the "
                            "bench contract), frontend only (the headline's synthetic pan makes "
                            "a keyframe of every other frame); the reference's own FPS window "
                            "(main.py:363-535) adds the host I/O -- end_to_end_fps (PNG read + "
                            "resize_img + H2D + PNG write) -- and runs the backend process "
                            "beside the frontend -- fps_with_backend (same frontend "
                            "configuration, backend worker on a lowest-priority stream; "
                            "fps_with_backend_drained also waits for its queue to empty)",
        "world_size": ws, "dist_backend": backend,
        # a throwaway GPU child process ran before this one (bench._prewarm):
        # on a fresh box the FIRST GPU process pays a one-time ~6 ms stall in
        # its frame loop whose cause lies outside this tree;
        # S3_BENCH_PREWARM=0 measures the unwarmed first process
        "prewarm_child": prewarmed,
        "config": {"workload": "C2 per-frame SLAM tracking, 512x384, config/base.yaml, --no-viz, "
                               "render on, spatial stride 4", "model": "Splatt3R (MASt3RGaussians)",
                   "global_batch": ws, "seq_len": 768,
                   "parallelism": f"replicas x{ws} (tracker path does not shard)",
                   "encoder_batch": kb, "encoder_ahead": a.enc_ahead,
                   "decode_ahead": a.decode_ahead, "render_async": a.render_async,
                   "render_stream": "aux" if getattr(fe, "render_on_aux", False) else "main",
                   "timed_encodes": encodes, "planned_encodes": plan["timed_encodes"]},
        "msplats_per_s": P_frame * st["rendered"] * ws / t_max / 1e6,
        "critical_path": crit,
        "frame_breakdown": {"network_event_ms": net_ms,
                            "gn_iters_avg": st["gn_iters"] / max(1, st["tracked"]),
                            "keyframes": st["keyframes"],
                            "keyframe_rate": st["keyframes"] / max(1, a.steps),
                            "reloc": st["reloc"],
                            "decode_ahead": ahead,
                            "rendered": st["rendered"], "tracked": st["tracked"],
                            # sync-free renders that did not fit the learnt
                            # capacity / key width and were re-rendered
                            "rerendered": st.get("rerendered", 0),
                            # a lost frame (RELOC) in this frontend-only loop would
                            # turn later frames into untracked mono inferences
                            "tracking_complete": st["tracked"] == a.steps and st["reloc"] == 0},
    }
    if encodes != a.steps:
        print(f"[bench] WARNING: {encodes} image encodes in the timed region for {a.steps} "
              f"frames", file=sys.stderr, flush=True)
    if not result["frame_breakdown"]["tracking_complete"]:
        print(f"[bench] WARNING: tracked {st['tracked']} of {a.steps} frames, reloc {st['reloc']}: "
              "the frame rate is not a tracking frame rate", file=sys.stderr, flush=True)
    if rank == 0 and not a.no_kprof:
        # after the timed region: kernel durations of the plans' graph
        # replays (roctracer trace) and a per-launch eager profile
        units = _frame_units(model.encoder, units0, a.steps)
        trace = _kernel_trace(units)
        prof = _kernel_profile(units)
        flops_frame = sum(v[1] for v in prof.values())
        net_tflops = sum(v[1] for v in prof.values()) / (sum(v[2] for v in prof.values()) * 1e-3) / 1e12
        dom = max((k for k in prof if prof[k][1] > 0), key=lambda k: prof[k][2])
        n_l, fl_run, ms = prof[dom]
        # only the work the frames needed: decode-ahead slots computed and
        # never used are reported apart and not counted as achieved FLOPs
        fl_spec = _spec_flops(model.encoder, ahead, dom, H, W) / a.steps
        fl = fl_run - fl_spec
        source = "HIP event pair around each launch of an eager replay of the plans"
        if trace and dom in trace and abs(trace[dom][0] - n_l) < 0.5:
            # the traced frames ran exactly this frame's launches of the
            # family: time them as they run inside the graphs (the event
            # pairs of the eager replay flush caches between launches)
            ms = trace[dom][1]
            source = (f"roctracer kernel timestamps (torch.profiler) of serial replays of the "
                      f"plans' HIP graphs after the timed region; eager per-launch event "
                      f"timing: {prof[dom][2]:.3f} ms/frame")
        achieved = fl / (ms * 1e-3) / 1e12
        tr = _pmc_traffic(dom)
        # algorithmic bytes of the same (non-speculative) launches (units'
        # weights are replays per frame: already per frame)
        ab = _algo_bytes(units, dom) * (fl / fl_run if fl_run else 1.0)
        result["roofline"] = {
            "bound": "mfma", "kernel": f"s3n {dom} (all launches of one frame)",
            "achieved": achieved, "peak": PEAK_F16_TFLOPS, "unit": "TFLOP/s",
            "frac": achieved / PEAK_F16_TFLOPS,
            # per frame, like `achieved` (all launches of the family in one frame)
            "traffic": tr["bytes_per_frame"] if tr else None,
            "traffic_unit": "HBM bytes per frame (PMC FETCH_SIZE x2 + WRITE_SIZE)",
            "algorithmic_bytes_per_frame": ab,
            "traffic_over_algorithmic": (tr["bytes_per_frame"] / ab) if (tr and ab) else None,
            "launches_per_frame": n_l, "avg_launch_us": ms / n_l * 1e3,
            "ms_per_frame": ms, "timing": source,
            "algorithmic_gflop_per_frame": fl / 1e9,
            "speculative_gflop_per_frame": fl_spec / 1e9,
            "executed_gflop_per_frame": fl_run / 1e9,
            "flops_counted": "non-speculative: every frame's encoder + its decoder/heads; "
                             "decode-ahead slots computed and dropped are in "
                             "speculative_gflop_per_frame and excluded from achieved"}
        if trace:
            result["roofline"]["trace_ms_per_frame"] = {k: v[1] for k, v in trace.items()}
        if not a.no_in_window:
            iw = bench_in_window(model, dev, 16, a.warmup, kb, a.enc_ahead, a.decode_ahead,
                                 a.main_priority)
            if dom in iw and iw[dom][1] > 0:
                l_iw, ms_iw, gf_iw = iw[dom]
                result["roofline"]["in_window"] = {
                    "achieved": gf_iw / ms_iw, "frac": gf_iw / ms_iw / PEAK_F16_TFLOPS,
                    "ms_per_frame": ms_iw, "launches_per_frame": l_iw,
                    "executed_gflop_per_frame": gf_iw,
                    "timing": "roctracer kernel timestamps (torch.profiler) of 16 frames of a "
                              "frame loop with the headline's configuration (encoder side stream "
                              "and main chain concurrent), executed FLOPs of the same window",
                    "families_ms_per_frame": {k: v[1] for k, v in iw.items()}}
        if tr:
            result["roofline"]["traffic_detail"] = tr
        result["network"] = {"kernels": {k: {"launches": v[0], "gflop": v[1] / 1e9, "ms": v[2]}
                                         for k, v in sorted(prof.items(), key=lambda x: -x[1][2])},
                             "tflops_in_kernels": net_tflops,
                             "mfma_util_in_kernels": net_tflops / PEAK_F16_TFLOPS,
                             "gflop_per_frame": flops_frame / 1e9,
                             "tflops_wall": flops_frame / (net_ms * 1e-3) / 1e12}
    result["device_path_fps"] = value
    fe.close()
    # fp16 store guards of the network (GEMM epilogues, LayerNorm) that fired
    # since the process started: > 0 means activations beyond +-65504 were
    # saturated (the Frontend warns at close() too)
    from splatt3r_amd import ops as _ops
    result["f16_saturations"] = _ops.f16_saturations()
    if rank == 0 and not a.no_e2e:
        e2e = bench_end_to_end(model, dev, a.steps, a.warmup, a.main_priority,
                               workers=a.e2e_loaders, writers=a.e2e_writers,
                               enc_batch=kb, enc_ahead=a.enc_ahead, decode_ahead=a.decode_ahead,
                               render_async=a.render_async)
        result["end_to_end_fps"] = e2e["frames_per_s"]
        result["end_to_end"] = e2e
    if rank == 0 and not a.no_live:
        result["live_camera"] = bench_live(model, dev, frames, a.steps, a.warmup,
                                           a.main_priority)
    if not a.no_pairs:
        from splatt3r_amd.pairs import bench_pairs
        result["pairs"] = bench_pairs(model, frames, ws, rank, dev, a.pairs_per_rank)
        result["pairs"]["scaling"] = "weak"
        # strong scaling: a fixed pair batch split over the ranks
        result["pairs_strong"] = dict(bench_pairs(model, frames, ws, rank, dev,
                                                  total=a.strong_pairs, with_map=False),
                                      scaling="strong")
        # C4 (EuRoC MH_01 shape): 512x320 frames, 640 tokens, same pair path
        c4 = tum_like_sequence(12, 320, 512, seed=200 + rank, step_px=2.0, device=dev)
        result["pairs_c4"] = dict(bench_pairs(model, c4, ws, rank, dev, a.pairs_per_rank),
                                  image="512x320 (C4, EuRoC MH_01 shape)", scaling="weak")
        if rank == 0:
            # units / map edges decoded on other ranks, re-decoded on rank 0
            # after the timed batches and compared bit for bit
            legs = {k: {c: result[k].get(c) for c in ("shard_check", "map_shard_check")
                        if result[k].get(c) is not None}
                    for k in ("pairs", "pairs_strong", "pairs_c4")}
            result["shard_check"] = {
                "equal": all(v["equal"] for leg in legs.values() for v in leg.values()),
                "world_size": ws, "dist_backend": backend, "legs": legs}
    if not a.no_backend:
        # ws > 1: rank 0's backend shards its pair batches over every rank
        be = bench_backend(model, dev, a.backend_steps, rank, ws, enc_batch=kb,
                           enc_ahead=a.enc_ahead, decode_ahead=a.decode_ahead,
                           main_priority=a.main_priority)
        if rank == 0:
            result["backend"] = be
            # beside `value`: the same frontend configuration with the
            # reference's concurrent backend (base.yaml single_thread: False)
            result["fps_with_backend"] = be["frames_per_s"]
            result["fps_with_backend_drained"] = be["frames_per_s_drained"]
    if rank == 0 and not a.no_map:
        result["map_c5"] = bench_map(dev)
    if rank == 0 and not a.no_c3:
        from tools.bench_raster import run as raster_run
        r = raster_run(4_194_304, iters=5, warmup=2, backward=True, device=dev)
        result["raster_c3"] = {k: r[k] for k in ("P", "fwd_ms", "msplats_per_s", "fwd_GBps",
                                                 "phases_ms", "bwd_ms", "bwd_GBps",
                                                 "num_rendered", "visible", "fwd_deferred_ms",
                                                 "deferred_equal")}
        result["raster_c3"]["hbm_frac"] = r["fwd_GBps"] / PEAK_HBM_GBPS
        # BASELINE config 3 is forward + backward
        result["raster_c3"]["fwd_bwd_ms"] = r["fwd_ms"] + r["bwd_ms"]
        result["raster_c3"]["msplats_per_s_fwd_bwd"] = r["P"] / ((r["fwd_ms"] + r["bwd_ms"])
                                                                 * 1e-3) / 1e6
    if rank == 0 and not a.no_c3:
        from splatt3r_amd.retrieval_database import bench as retrieval_bench
        result["retrieval"] = retrieval_bench(dev)
    if rank == 0 and ws == 1 and not a.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(FULL, seed, frames, a.cpu_frames)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if ws > 1:
        # ranks > 0 wait for rank 0's single-GPU legs, then all leave together
        _barrier(ws)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
