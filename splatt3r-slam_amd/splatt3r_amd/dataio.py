"""Harness input/output around the per-frame path, inside
the reference's FPS window (main.py:363-535):

  TUMDataset      splatt3r_slam/dataloader.py:18-60 (+ TUM rgb.txt parsing,
                  :63-78): dataset[i] -> (timestamp, HxWx3 float32 in [0, 1])
  EurocDataset    dataloader.py:92-116: mav0/cam0 (data.csv, sensor.yaml,
                  data/*.png), greyscale, always undistorted
  load_dataset    dataloader.py:320-327: the reader by the path's segments
  FrameLoader     dataset[i] -> create_frame's host work (resize_img: PIL
                  LANCZOS 640x480 -> 512x384 + centre crop + ImgNorm,
                  splatt3r_utils.py:658-693, frame.py:122-133) -> pinned
                  buffer -> H2D on a copy stream, on worker threads a few
                  frames ahead of the tracker; ingest="device" uploads the
                  raw uint8 frame instead and does that work in one HIP
                  launch (splatt3r_amd/ingest.py), with the same result
  RenderWriter    the per-frame render export (main.py:436-446 `gs_init_*`,
                  :490-506 `gs_track_*`): D2H of the rendered [1,1,3,H,W]
                  image into a pinned ring, then uint8 conversion and the
                  PNG write on writer threads
  write_synthetic_euroc  a EuRoC-layout sequence of 752x480 greyscale frames
                  with MH_01's cam0 calibration
  write_synthetic_tum  a TUM-layout sequence (rgb/*.png + rgb.txt) of 640x480
                  frames for the benchmark when fr1_desk itself is absent

The reference does all of this synchronously in the tracking loop (its
dataset read, its resize and its cv2.imwrite sit between the GPU calls);
here the host work runs on threads that overlap the GPU, with the same
bytes in and out: the frames the tracker sees are resize_img's output (of
the undistorted frame when the dataset is calibrated: intrinsics.py, cv2.remap
restated; on the device with ingest="device"), and
each PNG holds `uint8(clamp(render, 0, 1) * 255)` (truncation, as the
reference's `.astype("uint8")`), in RGB order (cv2 writes the BGR array it
was given, i.e. RGB on disk; PIL writes RGB).  cv2 is not installed here:
PIL does the PNG codec work, at cv2's default compression level 1.
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import pathlib
import queue
import re
import threading
from typing import Optional

import numpy as np
import torch


# ------------------------------------------------------------------ input --
# dataloader.py:76-89: fx fy cx cy [k1 k2 p1 p2 k3] of the three TUM cameras
TUM_CALIB = {
    1: (517.3, 516.5, 318.6, 255.3, 0.2624, -0.9531, -0.0054, 0.0026, 1.1633),
    2: (520.9, 521.0, 325.1, 249.7, 0.2312, -0.7849, -0.0033, -0.0001, 0.9172),
    3: (535.4, 539.2, 320.1, 247.6),
}


class MonocularDataset:
    """dataloader.py:20-64: dataset[i] -> (timestamp, img float32 [H,W,3] in
    [0, 1], RGB).  With `use_calibration` the frame is undistorted first
    (camera_intrinsics.remap on the uint8 image, on the host here; the
    FrameLoader's device mode does it on the GPU)."""

    def __init__(self, dtype=np.float32):
        from splatt3r_amd.config import config
        self.dtype = dtype
        self.rgb_files: list = []
        self.timestamps = np.zeros(0, dtype=np.float64)
        self.img_size = 512
        self.camera_intrinsics = None
        self.use_calibration = bool(config["use_calib"])

    def __len__(self):
        return len(self.rgb_files)

    def read_img(self, idx) -> np.ndarray:
        from PIL import Image
        with Image.open(self.rgb_files[idx]) as im:
            return np.asarray(im.convert("RGB"))

    def get_image(self, idx) -> np.ndarray:
        img = self.read_img(idx)
        if self.use_calibration and self.camera_intrinsics is not None:
            img = self.camera_intrinsics.remap(img)
        if img.ndim == 2:                                   # greyscale: GRAY2BGR
            img = np.repeat(img[..., None], 3, axis=2)
        return img.astype(self.dtype) / 255.0

    def __getitem__(self, idx):
        return self.timestamps[idx], self.get_image(idx)

    def has_calib(self) -> bool:
        return self.camera_intrinsics is not None


class TUMDataset(MonocularDataset):
    """TUM RGB-D layout (rgb.txt: "timestamp rgb/<file>.png", '#' comments),
    dataloader.py:67-89.  cv2.imread + BGR2RGB in the reference; PIL reads
    RGB.  A path that names its camera (`freiburg1` .. `freiburg3`) gets that
    camera's calibration (used when config use_calib is on); any other path
    has none."""

    def __init__(self, root, subsample: int = 1):
        super().__init__()
        self.root = pathlib.Path(root)
        rows = []
        with open(self.root / "rgb.txt") as f:
            for line in f:
                if line.startswith("#") or not line.strip():
                    continue
                t, path = line.split()[:2]
                rows.append((float(t), self.root / path))
        rows = rows[::subsample]
        self.timestamps = np.array([t for t, _ in rows], dtype=np.float64)
        self.rgb_files = [p for _, p in rows]
        m = re.search(r"freiburg(\d+)", str(root))
        if m is not None and int(m.group(1)) in TUM_CALIB:
            from splatt3r_amd.intrinsics import Intrinsics
            self.camera_intrinsics = Intrinsics.from_calib(self.img_size, 640, 480,
                                                           TUM_CALIB[int(m.group(1))])
        if self.camera_intrinsics is None:
            self.use_calibration = False
        # sensor depth: depth.txt ("timestamp depth/<file>.png") when present,
        # each RGB frame paired with the nearest depth stamp within 0.02 s
        self.depth_files: list = [None] * len(self.rgb_files)
        if (self.root / "depth.txt").exists():
            from splatt3r_amd.evaluate import associate
            drows = []
            with open(self.root / "depth.txt") as f:
                for line in f:
                    if line.startswith("#") or not line.strip():
                        continue
                    t, path = line.split()[:2]
                    drows.append((float(t), self.root / path))
            ia, ib = associate(self.timestamps, [t for t, _ in drows], 0.02)
            for i, j in zip(ia.tolist(), ib.tolist()):
                self.depth_files[i] = drows[j][1]

    DEPTH_FACTOR = 5000.0          # TUM: a 16-bit PNG value of 5000 is 1 m, 0 is no reading

    def read_depth(self, idx) -> Optional[np.ndarray]:
        """The sensor depth of RGB frame idx in metres, float32 [H, W] at the
        sensor's resolution with 0 where there is no reading
        (ingest.resize_depth brings it to the network's geometry), or None
        when the frame has no depth partner (or the sequence no depth.txt).
        A sequence read undistorted has no depth: undistorting depth is not
        done here."""
        if self.use_calibration:
            raise NotImplementedError(
                "TUMDataset.read_depth: the sequence is read undistorted (use_calib); "
                "undistorting depth is not implemented")
        path = self.depth_files[idx]
        if path is None:
            return None
        from PIL import Image
        with Image.open(path) as im:
            raw = np.asarray(im)
        return raw.astype(np.float32) / np.float32(self.DEPTH_FACTOR)


class EurocDataset(MonocularDataset):
    """EuRoC MAV layout, dataloader.py:92-116: mav0/cam0/data.csv
    ("timestamp [ns],filename", '#' comments), mav0/cam0/sensor.yaml
    (resolution, intrinsics, distortion_coefficients) and
    mav0/cam0/data/*.png.  Always undistorted ("the distortion is too much to
    handle for MASt3R"), whether or not use_calib is on.  read_img returns
    the greyscale frame uint8 [H,W]; timestamps are int64 nanoseconds."""

    def __init__(self, root, subsample: int = 1):
        super().__init__()
        import yaml
        from splatt3r_amd.intrinsics import Intrinsics
        self.use_calibration = True
        self.root = pathlib.Path(root)
        cam0 = self.root / "mav0" / "cam0"
        rows = []
        with open(cam0 / "data.csv") as f:
            for line in f:
                if line.startswith("#") or not line.strip():
                    continue
                t, name = (v.strip() for v in line.split(",")[:2])
                rows.append((int(t), cam0 / "data" / name))
        rows = rows[::subsample]
        self.timestamps = np.array([t for t, _ in rows], dtype=np.int64)
        self.rgb_files = [p for _, p in rows]
        with open(cam0 / "sensor.yaml") as f:
            self.cam0 = yaml.safe_load(f)
        W, H = self.cam0["resolution"]
        calib = [*self.cam0["intrinsics"], *self.cam0["distortion_coefficients"]]
        self.camera_intrinsics = Intrinsics.from_calib(self.img_size, W, H, calib,
                                                       always_undistort=True)

    def read_img(self, idx) -> np.ndarray:
        from PIL import Image
        with Image.open(self.rgb_files[idx]) as im:
            return np.asarray(im.convert("L"))


def load_dataset(path):
    """dataloader.py:320-327: the reader named by a segment of the path
    (`tum` or `euroc`)."""
    parts = str(path).split("/")
    if "tum" in parts:
        return TUMDataset(path)
    if "euroc" in parts:
        return EurocDataset(path)
    raise ValueError(f"load_dataset: no reader for {str(path)!r}: the path needs a segment "
                     "'tum' or 'euroc' (the reference's other kinds -- eth3d, 7-scenes, "
                     "realsense, webcam, video and plain image folders -- are not served)")


# MH_01 cam0 (mav0/cam0/sensor.yaml of the EuRoC MAV dataset)
EUROC_RESOLUTION = (752, 480)
EUROC_INTRINSICS = (458.654, 457.296, 367.215, 248.375)
EUROC_DISTORTION = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)


def write_synthetic_euroc(root, n: int, seed: int = 0, step_px: float = 2.5) -> pathlib.Path:
    """A EuRoC-layout sequence of n 752x480 greyscale PNG frames (the texture
    of write_synthetic_tum) with MH_01's cam0 sensor.yaml, for tests and for
    users without the dataset."""
    from PIL import Image
    from splatt3r_amd.synthetic import smooth_texture
    root = pathlib.Path(root)
    cam0 = root / "mav0" / "cam0"
    (cam0 / "data").mkdir(parents=True, exist_ok=True)
    W, H = EUROC_RESOLUTION
    pad = int(np.ceil(step_px * n)) + 8
    tex = smooth_texture(H + pad, W + pad, seed).mean(0)    # [H', W'] in [0, 1]
    lines = ["#timestamp [ns],filename"]
    for i in range(n):
        oy = int(round(0.5 * step_px * i)) + 4
        ox = int(round(step_px * i)) + 4
        t = 1403636579763555584 + i * 50000000              # 20 Hz
        Image.fromarray(np.round(tex[oy:oy + H, ox:ox + W] * 255).astype(np.uint8)).save(
            cam0 / "data" / f"{t}.png", compress_level=1)
        lines.append(f"{t},{t}.png")
    (cam0 / "data.csv").write_text("\n".join(lines) + "\n")
    (cam0 / "sensor.yaml").write_text(
        "# synthetic EuRoC-layout sequence, MH_01 cam0 calibration\n"
        "sensor_type: camera\n"
        "rate_hz: 20\n"
        f"resolution: [{W}, {H}]\n"
        "camera_model: pinhole\n"
        f"intrinsics: [{', '.join(repr(v) for v in EUROC_INTRINSICS)}]\n"
        "distortion_model: radial-tangential\n"
        f"distortion_coefficients: [{', '.join(repr(v) for v in EUROC_DISTORTION)}]\n")
    return root


def write_synthetic_tum(root, n: int, H: int = 480, W: int = 640, seed: int = 0,
                        step_px: float = 2.5, depth: bool = False) -> pathlib.Path:
    """A TUM-layout sequence of n H x W PNG frames panning over a smooth
    multi-scale texture (synthetic.tum_like_sequence's generator at the
    camera's native 640x480, before resize_img).

    depth=True also writes the sensor depth of that planar scene, as TUM
    ships it: depth/<t>.png (16-bit, 5000 per metre, 0 for no reading) and
    depth.txt, stamped 5 ms after the colour frames.  The plane is 2 m away
    and tilted by 0.25 m across the image width, and an 8-pixel band on the left
    has no reading (the shadow of a real sensor's baseline).  The other
    files are the same bytes with and without it."""
    from PIL import Image
    from splatt3r_amd.synthetic import smooth_texture
    root = pathlib.Path(root)
    (root / "rgb").mkdir(parents=True, exist_ok=True)
    if depth:
        (root / "depth").mkdir(parents=True, exist_ok=True)
        plane = np.broadcast_to(2.0 + 0.25 * np.arange(W, dtype=np.float64) / W, (H, W))
        raw = np.round(plane * TUMDataset.DEPTH_FACTOR).astype(np.uint16)
        raw[:, :8] = 0
        dlines = ["# depth maps", "# synthetic TUM-layout sequence", "# timestamp filename"]
        for i in range(n):
            t = 1305031102.175304 + i / 30.0 + 0.005
            name = f"depth/{t:.6f}.png"
            Image.fromarray(raw).save(root / name, compress_level=1)
            dlines.append(f"{t:.6f} {name}")
        (root / "depth.txt").write_text("\n".join(dlines) + "\n")
    pad = int(np.ceil(step_px * n)) + 8
    tex = smooth_texture(H + pad, W + pad, seed)           # [3, H', W'] in [0, 1]
    lines = ["# color images", "# synthetic TUM-layout sequence", "# timestamp filename"]
    for i in range(n):
        oy = int(round(0.5 * step_px * i)) + 4
        ox = int(round(step_px * i)) + 4
        frame = tex[:, oy:oy + H, ox:ox + W].transpose(1, 2, 0)
        t = 1305031102.175304 + i / 30.0
        name = f"rgb/{t:.6f}.png"
        Image.fromarray(np.round(frame * 255).astype(np.uint8)).save(root / name,
                                                                      compress_level=1)
        lines.append(f"{t:.6f} {name}")
    (root / "rgb.txt").write_text("\n".join(lines) + "\n")
    return root


class LoadedFrame:
    """One frame as create_frame needs it: img [1,3,H,W] on the device
    (ImgNorm), true_shape [[H, W]], the unnormalised uint8 image (a numpy
    array; with device ingest a device tensor) and the copy-stream event
    after which `img` is valid."""

    __slots__ = ("index", "timestamp", "img", "true_shape", "uimg", "ready")

    def __init__(self, index, timestamp, img, true_shape, uimg, ready):
        self.index, self.timestamp, self.img = index, timestamp, img
        self.true_shape, self.uimg, self.ready = true_shape, uimg, ready

    def consume(self, stream=None):
        """Order `stream` (default: the current one) after the upload and
        tell the allocator the image is used there."""
        s = stream or torch.cuda.current_stream(self.img.device)
        s.wait_event(self.ready)
        self.img.record_stream(s)
        if torch.is_tensor(self.uimg) and self.uimg.is_cuda:    # device ingest
            self.uimg.record_stream(s)
        return self.img


class FrameLoader:
    """dataset[i] + create_frame's host work + H2D, `depth` frames ahead of
    the consumer on `workers` threads (PIL releases the GIL in its decode and
    resample loops).  Frames come out in index order: `next()` or
    iteration.  `close()` stops the workers."""

    def __init__(self, dataset, device, img_size: int = 512, workers: int = 3, depth: int = 6,
                 start: int = 0, stop: Optional[int] = None, ingest: Optional[str] = None):
        """ingest: "host" (resize_img on the worker, float32 upload) or
        "device" (the raw uint8 frame is uploaded and ingest.resize_img_device
        resizes, crops and normalises it on the loader's stream; the same
        `img`, and `uimg` stays on the device).  None: the environment
        variable S3_INGEST, default "host".

        A dataset with `use_calibration` set has its frames undistorted with
        `dataset.camera_intrinsics` before the resize, in both modes and with
        identical `img` and `uimg`: "device" runs the HIP remap (s3u_remap)
        in front of the ingest launch on the loader's stream; "host" runs the
        numpy restatement intrinsics.remap_u8 on the worker, which is slow
        (tens of milliseconds per frame) and correct."""
        self.ds = dataset
        self.device = torch.device(device)
        self.img_size = img_size
        self.ingest = os.environ.get("S3_INGEST", "host") if ingest is None else ingest
        if self.ingest not in ("host", "device"):
            raise ValueError(f"FrameLoader: ingest must be 'host' or 'device', got {self.ingest!r}")
        # device mode: pinned uint8 staging buffers [buffer, event of the
        # last upload that read it]; a worker takes one, waits for that
        # event, fills it, and puts it back with its own upload's event
        self._ring: "queue.Queue" = queue.Queue()
        for _ in range(workers + 1):
            self._ring.put([None, None])
        self.stream = torch.cuda.Stream(device=self.device)
        self._pool = cf.ThreadPoolExecutor(max_workers=workers, thread_name_prefix="s3-load")
        self._next = start
        self._stop = len(dataset) if stop is None else min(stop, len(dataset))
        self._futs: dict = {}
        self._depth = depth
        self._lock = threading.Lock()
        self._undistort = (getattr(dataset, "camera_intrinsics", None)
                           if getattr(dataset, "use_calibration", False) else None)
        self._fill()

    def _fill(self):
        while len(self._futs) < self._depth:
            i = self._next + len(self._futs)
            if i >= self._stop:
                break
            self._futs[i] = self._pool.submit(self._load, i)

    def _load_device(self, i) -> LoadedFrame:
        from splatt3r_amd.ingest import resize_img_device
        raw = self.ds.read_img(i)                          # uint8 [H, W, 3] (greyscale: [H, W])
        slot = self._ring.get()
        try:
            buf, busy = slot
            if busy is not None:
                busy.synchronize()                         # the upload that last read buf
            if buf is None or buf.shape != raw.shape:
                buf = slot[0] = torch.empty(raw.shape, dtype=torch.uint8, pin_memory=True)
            buf.numpy()[...] = raw
            with self._lock, torch.cuda.stream(self.stream):
                dev = buf.to(self.device, non_blocking=True)
                slot[1] = torch.cuda.Event()
                slot[1].record(self.stream)
                r = resize_img_device(dev, self.img_size, stream=self.stream,
                                      undistort=self._undistort)
                ev = torch.cuda.Event()
                ev.record(self.stream)
        finally:
            self._ring.put(slot)
        return LoadedFrame(i, self.ds.timestamps[i], r["img"], torch.tensor(r["true_shape"]),
                           r["unnormalized_img"], ev)

    def _load(self, i) -> LoadedFrame:
        if self.ingest == "device":
            return self._load_device(i)
        from splatt3r_amd.splatt3r_utils import resize_img
        t, img = self.ds[i]
        r = resize_img(img, self.img_size)
        host = r["img"].pin_memory()
        # one upload stream shared by the workers: the lock keeps each
        # copy + its event together
        with self._lock, torch.cuda.stream(self.stream):
            dev = host.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        # (torch's caching host allocator keeps the pinned block until the
        # non_blocking copy that read it has completed)
        return LoadedFrame(i, t, dev, torch.tensor(r["true_shape"]), r["unnormalized_img"], ev)

    def __len__(self):
        return self._stop

    def __iter__(self):
        return self

    def __next__(self) -> LoadedFrame:
        if self._next >= self._stop:
            raise StopIteration
        f = self._futs.pop(self._next).result()
        self._next += 1
        self._fill()
        return f

    def close(self):
        for f in self._futs.values():
            f.cancel()
        self._pool.shutdown(wait=True)


# ----------------------------------------------------------------- output --
def render_to_uint8(img_hwc: np.ndarray) -> np.ndarray:
    """main.py:441-444 / 501-504: clamp(0, 1) -> * 255 -> astype(uint8)
    (truncating, as numpy's cast)."""
    return (np.clip(img_hwc, 0.0, 1.0) * 255).astype(np.uint8)


class RenderWriter:
    """Per-frame render PNGs (main.py:436-446, 490-506) off the tracking
    thread.  submit() queues an async D2H copy of the [3,H,W] (or
    [1,1,3,H,W]) render into a pinned buffer of a ring of `ring` buffers on
    the current stream; writer threads wait for the copy, convert and write
    `{render_dir}/{prefix}_{i:06d}.png`.  When every buffer is in flight
    submit() waits for the oldest write (back-pressure: the reference writes
    synchronously, this never drops a frame)."""

    def __init__(self, render_dir, workers: int = 3, ring: int = 8, compress_level: int = 1):
        self.dir = pathlib.Path(render_dir)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.compress_level = compress_level
        self._free: "queue.Queue" = queue.Queue()
        self._ring = ring
        self._bufs: list = []
        self._pool = cf.ThreadPoolExecutor(max_workers=workers, thread_name_prefix="s3-png")
        self._pending: list = []
        self._count_lock = threading.Lock()
        self.written = 0

    def _buffer(self, shape):
        if self._bufs and tuple(self._bufs[0].shape) != tuple(shape):
            self.flush()
            self._bufs, self._free = [], queue.Queue()
        if len(self._bufs) < self._ring and self._free.empty():
            b = torch.empty(shape, dtype=torch.float32, pin_memory=True)
            self._bufs.append(b)
            return b
        return self._free.get()

    def submit(self, index: int, img: torch.Tensor, prefix: str = "gs_track"):
        x = img.detach()
        while x.dim() > 3:
            x = x[0]
        x = x.permute(1, 2, 0)                            # [H, W, 3]
        buf = self._buffer(tuple(x.shape))
        buf.copy_(x, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        path = self.dir / f"{prefix}_{index:06d}.png"
        self._pending.append(self._pool.submit(self._write, buf, ev, path))
        self._pending = [f for f in self._pending if not f.done() or f.exception()]

    def _write(self, buf, ev, path):
        from PIL import Image
        try:
            ev.synchronize()
            Image.fromarray(render_to_uint8(buf.numpy())).save(path, compress_level=self.compress_level)
            with self._count_lock:
                self.written += 1
        finally:
            self._free.put(buf)

    def flush(self):
        for f in self._pending:
            f.result()
        self._pending = []

    def close(self):
        self.flush()
        self._pool.shutdown(wait=True)
