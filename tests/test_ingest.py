"""Device-side frame ingest (splatt3r_amd/ingest.py, include/s3i.h): a raw
uint8 frame resized, cropped and normalised on the GPU, bit for bit what the
host path (splatt3r_utils.resize_img: PIL resize + centre crop + ImgNorm)
gives.  Every comparison is exact equality.

References: resize_img itself, PIL.Image.resize (for the coefficient
tables), and for the seven shapes of test_host_input.CASES the fixture
tests/golden/resize_img.npz that the reference's own function text produced.
"""
import functools
import os
import threading

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_host_input import CASES, resize_input

# (h, w, size, square_ok): the fixture's cases, then small / odd / large ones
SHAPES = tuple((h, w, s, False) for h, w, s in CASES) + (
    (37, 53, 512, False), (96, 128, 512, False), (601, 803, 512, False),
    (1080, 1920, 512, False), (512, 512, 512, True))
SWEEP_H = (37, 96, 300, 480, 512, 540, 601, 640, 1080)
SWEEP_W = (53, 128, 400, 512, 640, 752, 803, 960, 1920)


@functools.lru_cache(maxsize=None)
def frame_u8(h, w, i, kind):
    """The uint8 frame of case i: the fixture's smooth recipe (as resize_img
    quantises it) or uniform noise, which drives both ends of the clamp."""
    if kind == "smooth":
        a = np.uint8(resize_input(h, w, i) * 255)
    else:
        a = np.random.default_rng(i).integers(0, 256, (h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def host_result(h, w, size, square_ok, i, kind):
    """resize_img of the frame, computed once and shared (read-only)."""
    from splatt3r_amd.splatt3r_utils import resize_img
    u8 = frame_u8(h, w, i, kind)
    return resize_img(u8.astype(np.float32) / 255.0, size, square_ok=square_ok,
                      return_transformation=True)


def apply_tables(img, coeffs, bounds):
    """Pillow's 8-bit pass along axis 0 in int64: clamp((2^21 + sum) >> 22)."""
    src = img.astype(np.int64)
    out = np.empty((len(coeffs),) + img.shape[1:], np.uint8)
    for o, (xmin, cnt) in enumerate(bounds):
        acc = (1 << 21) + np.tensordot(coeffs[o, :cnt].astype(np.int64), src[xmin:xmin + cnt], 1)
        out[o] = np.clip(acc >> 22, 0, 255)
    return out


def resize_by_tables(u8, W, H, filt):
    """Horizontal pass into a uint8 image, then the vertical pass over it; a
    pass is skipped when that axis keeps its size (as PIL.Image.resize)."""
    from splatt3r_amd.ingest import resample_tables
    h, w = u8.shape[:2]
    x = u8
    if W != w:
        x = apply_tables(x.transpose(1, 0, 2), *resample_tables(w, W, filt)).transpose(1, 0, 2)
    if H != h:
        x = apply_tables(x, *resample_tables(h, H, filt))
    return x


# ------------------------------------------------------------------- CPU ---
def test_round_trip_of_a_uint8_frame_through_the_float_input_is_the_identity():
    """resize_img starts with np.uint8(img * 255); for img = uint8 / 255.0
    that gives the uint8 frame back, so the device path may start from it."""
    u = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(np.uint8((u.astype(np.float32) / 255.0) * 255), u)


@pytest.mark.parametrize("size", [512, 224])
def test_geometry_matches_resize_img(size):
    from splatt3r_amd.ingest import BICUBIC, LANCZOS, ingest_geometry
    from splatt3r_amd.splatt3r_utils import resize_img
    for h in SWEEP_H:
        for w in SWEEP_W:
            img = np.zeros((h, w, 3), np.float32)
            for square_ok in (False, True):
                res, tr = resize_img(img, size, square_ok=square_ok, return_transformation=True)
                (W, H), filt, box, tr_d = ingest_geometry(h, w, size, square_ok)
                where = f"{h}x{w} size {size} square_ok {square_ok}"
                assert [box[3] - box[1], box[2] - box[0]] == res["true_shape"][0].tolist(), where
                assert tr_d == tr, where
                assert 0 <= box[0] <= box[2] <= W and 0 <= box[1] <= box[3] <= H, where
                long_edge = round(size * max(w / h, h / w)) if size == 224 else size
                assert filt == (LANCZOS if max(h, w) > long_edge else BICUBIC), where


@pytest.mark.parametrize("case", range(len(SHAPES) - 1))
def test_tables_reproduce_pil_resize(case):
    """The coefficient tables applied in integer arithmetic equal
    PIL.Image.resize: what the kernel computes from them is Pillow's result."""
    import PIL.Image
    from splatt3r_amd.ingest import LANCZOS, ingest_geometry
    h, w, size, square_ok = SHAPES[case]
    (W, H), filt, _, _ = ingest_geometry(h, w, size, square_ok)
    for kind in ("smooth", "noise"):
        u8 = frame_u8(h, w, case, kind)
        want = np.asarray(PIL.Image.fromarray(u8).resize(
            (W, H), PIL.Image.LANCZOS if filt == LANCZOS else PIL.Image.BICUBIC))
        np.testing.assert_array_equal(resize_by_tables(u8, W, H, filt), want, err_msg=kind)


def test_tables_shape_and_edge_windows():
    """Layout of the tables, and the border windows: xmin clamps to 0 and
    count is cut at the image's end; every row of coefficients sums to about
    2^22 (each is rounded on its own)."""
    from splatt3r_amd.ingest import BICUBIC, LANCZOS, resample_tables
    k, b = resample_tables(1920, 512, LANCZOS)
    assert k.dtype == np.int32 and b.dtype == np.int32
    assert k.shape == (512, 25) and b.shape == (512, 2)            # ceil(3 * 3.75) * 2 + 1
    assert b[0, 0] == 0 and b[0, 1] < b[256, 1]
    assert b[-1, 0] + b[-1, 1] == 1920 and b[-1, 1] < b[256, 1]
    assert np.all(np.diff(b[:, 0]) >= 0) and np.all(np.diff(b.sum(1)) >= 0)
    assert np.all(np.abs(k.astype(np.int64).sum(1) - (1 << 22)) <= 25)
    k, b = resample_tables(300, 384, BICUBIC)
    assert k.shape == (384, 5) and np.all(b[:, 1] <= 5)            # upscale: support 2
    assert resample_tables(300, 384, BICUBIC)[0] is k              # cached


def test_abi_rejects_bad_arguments_before_any_device_work():
    from splatt3r_amd import _lib, ingest  # noqa: F401
    lib = _lib.lib()

    def call(B=1, in_h=8, in_w=8, res_w=8, res_h=8, crop=(0, 0, 8, 8), src=1):
        return lib.s3i_ingest(src, B, in_h, in_w, None, None, 0, res_w, None, None, 0, res_h,
                              *crop, 1, 1, None, None, None)

    bad = ((dict(B=0), b"B = 0"), (dict(in_h=0), b"input size"),
           (dict(in_w=-3), b"input size"), (dict(crop=(0, 0, 0, 8)), b"crop size"),
           (dict(crop=(1, 0, 8, 8)), b"outside the resized image"),
           (dict(crop=(0, 4, 8, 5)), b"outside the resized image"),
           (dict(res_w=6, crop=(0, 0, 6, 8)), b"res_w != in_w"),
           (dict(res_h=9), b"res_h != in_h"), (dict(src=None), b"must not be NULL"))
    got = []
    # the last-error message is per thread: a thread of its own leaves the
    # calling thread's untouched
    t = threading.Thread(target=lambda: got.extend((call(**kw), lib.s3_last_error())
                                                   for kw, _ in bad))
    t.start()
    t.join()
    assert len(got) == len(bad)
    for (kw, msg), (status, err) in zip(bad, got):
        assert status == 1 and msg in err, (kw, status, err)
    assert lib.s3i_workspace_bytes(2, 480, 512) == 2 * 480 * 512 * 3
    assert lib.s3i_fused_fits(480, 640, 9, 512, 9, 384) == 1
    assert lib.s3i_fused_fits(1080, 1920, 25, 512, 25, 288) == 1
    assert lib.s3i_fused_fits(6000, 8000, 95, 512, 95, 384) == 0   # two launches


def test_input_validation():
    """Checked before anything touches the device."""
    from splatt3r_amd.ingest import resize_img_device
    u8 = np.zeros((48, 64, 3), np.uint8)
    for bad in (u8.astype(np.float32), u8[:, ::2], np.zeros((48, 64, 4), np.uint8),
                torch.zeros(48, 64, 3), torch.zeros(48, 64, 3, dtype=torch.uint8)[:, ::2],
                torch.zeros(2, 48, 64, 4, dtype=torch.uint8), np.zeros((64, 3), np.uint8)):
        with pytest.raises(RuntimeError):
            resize_img_device(bad, 512)


# ------------------------------------------------------------------- GPU ---
def assert_same(res, tr, want, want_tr):
    assert res["img"].dtype == torch.float32 and res["img"].is_cuda
    assert torch.equal(res["img"].cpu(), want["img"])
    assert res["unnormalized_img"].dtype == torch.uint8 and res["unnormalized_img"].is_cuda
    np.testing.assert_array_equal(res["unnormalized_img"].cpu().numpy(), want["unnormalized_img"])
    assert res["true_shape"].dtype == np.int32
    np.testing.assert_array_equal(res["true_shape"], want["true_shape"])
    assert tr == want_tr


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_resize_img_device_matches_resize_img(case):
    from splatt3r_amd.ingest import resize_img_device
    h, w, size, square_ok = SHAPES[case]
    for kind in ("smooth", "noise"):
        want, want_tr = host_result(h, w, size, square_ok, case, kind)
        res, tr = resize_img_device(frame_u8(h, w, case, kind), size, square_ok=square_ok,
                                    return_transformation=True)
        assert_same(res, tr, want, want_tr)
        if kind == "smooth" and case < len(CASES):
            g = np.load(os.path.join(GOLDEN, "resize_img.npz"))
            np.testing.assert_array_equal(res["unnormalized_img"].cpu().numpy(),
                                          g[f"case{case}_uimg"])
            np.testing.assert_array_equal(res["true_shape"], g[f"case{case}_true_shape"])
            np.testing.assert_array_equal(np.float64(tr), g[f"case{case}_transform"])
            ref = (g[f"case{case}_uimg"].astype(np.float32) / 255.0 - 0.5) / 0.5
            np.testing.assert_array_equal(res["img"][0].permute(1, 2, 0).cpu().numpy(), ref)


@pytest.mark.gpu
def test_first_use_with_cold_caches():
    """The first frame of a process: the host tables and their device copies
    are built inside the call (a shape no other test uses, caches emptied),
    from two threads at once as the loader's workers do."""
    from splatt3r_amd import ingest
    from splatt3r_amd.splatt3r_utils import resize_img
    u8 = np.random.default_rng(9).integers(0, 256, (50, 70, 3), dtype=np.uint8)
    want = resize_img(u8.astype(np.float32) / 255.0, 512)
    ingest._TABLES.clear()
    ingest._DEVICE.clear()
    got = [None, None]

    def work(j):
        got[j] = ingest.resize_img_device(u8, 512, stream=torch.cuda.Stream())
    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    for res in got:
        assert torch.equal(res["img"].cpu(), want["img"])
        np.testing.assert_array_equal(res["unnormalized_img"].cpu().numpy(),
                                      want["unnormalized_img"])
    assert len(ingest._TABLES) == 2 and len(ingest._DEVICE) == 5    # 2 x (k, b) + the LUT


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1, 5, 6, 7, 10, 11])
def test_two_launch_path_matches_resize_img(case):
    """The workspace path (taken on its own when no tile fits the LDS):
    Lanczos, bicubic, the 224 crop, 25 taps and the pure crop."""
    from splatt3r_amd import ingest
    h, w, size, square_ok = SHAPES[case]
    want, want_tr = host_result(h, w, size, square_ok, case, "noise")
    ingest.set_path(1)
    try:
        res, tr = ingest.resize_img_device(frame_u8(h, w, case, "noise"), size,
                                           square_ok=square_ok, return_transformation=True)
    finally:
        ingest.set_path(0)
    assert_same(res, tr, want, want_tr)


@pytest.mark.gpu
@pytest.mark.parametrize("path", [0, 1])
def test_single_axis_passes_and_offset_crop(path):
    """s3i_ingest with a table on one axis only and a crop that starts inside
    the image, for B = 2 frames of odd size whose rows start at every byte
    alignment, against the tables applied in numpy."""
    from splatt3r_amd import _lib, ingest
    from splatt3r_amd.ingest import LANCZOS, norm_lut, resample_tables
    B, h, w = 2, 41, 57
    u8 = np.random.default_rng(5).integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    src = torch.from_numpy(u8).cuda()
    lut = norm_lut().cuda()
    ingest.set_path(path)
    try:
        for axis, out in ((1, 31), (0, 23)):
            k, b = resample_tables(u8.shape[1 + axis], out, LANCZOS)
            kd, bd = torch.from_numpy(k.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
            want = np.stack([apply_tables(f.transpose(1, 0, 2), k, b).transpose(1, 0, 2)
                             if axis else apply_tables(f, k, b) for f in u8])
            res_h, res_w = want.shape[1:3]
            x0, y0, cw, ch = 3, 2, res_w - 7, res_h - 5
            want = want[:, y0:y0 + ch, x0:x0 + cw]
            img = torch.empty(B, 3, ch, cw, device="cuda")
            uimg = torch.empty(B, ch, cw, 3, dtype=torch.uint8, device="cuda")
            ws = torch.empty(_lib.lib().s3i_workspace_bytes(B, h, res_w), dtype=torch.uint8,
                             device="cuda")
            hk = (kd.data_ptr(), bd.data_ptr(), k.shape[1]) if axis else (None, None, 0)
            vk = (None, None, 0) if axis else (kd.data_ptr(), bd.data_ptr(), k.shape[1])
            _lib.call("s3i_ingest", src.data_ptr(), B, h, w, *hk, res_w, *vk, res_h,
                      x0, y0, cw, ch, lut.data_ptr(), img.data_ptr(), uimg.data_ptr(),
                      ws.data_ptr(), _lib.stream())
            np.testing.assert_array_equal(uimg.cpu().numpy(), want)
            assert torch.equal(img.cpu(), norm_lut()[torch.from_numpy(want).long()]
                               .permute(0, 3, 1, 2))
    finally:
        ingest.set_path(0)


@pytest.mark.gpu
def test_batch_equals_single_frames():
    from splatt3r_amd.ingest import resize_img_device
    frames = np.stack([frame_u8(96, 128, i, "noise") for i in range(3)])
    res = resize_img_device(frames, 512)
    assert res["img"].shape == (3, 3, 384, 512)
    assert res["unnormalized_img"].shape == (3, 384, 512, 3)
    np.testing.assert_array_equal(res["true_shape"], np.int32([[384, 512]] * 3))
    for i in range(3):
        one = resize_img_device(frames[i], 512)
        assert one["img"].shape == (1, 3, 384, 512)
        assert one["unnormalized_img"].shape == (384, 512, 3)
        assert torch.equal(res["img"][i], one["img"][0])
        assert torch.equal(res["unnormalized_img"][i], one["unnormalized_img"])
    # a device tensor goes in as it is
    dev = resize_img_device(torch.from_numpy(frames).cuda(), 512)
    assert torch.equal(dev["img"], res["img"])


@pytest.mark.gpu
def test_create_frame_takes_a_uint8_frame():
    from splatt3r_amd.frame import create_frame
    u8 = frame_u8(480, 752, 1, "smooth")
    got = create_frame(0, u8, device="cuda")
    want = create_frame(0, u8.astype(np.float32) / 255.0, device="cuda")
    assert got.img.is_cuda and torch.equal(got.img, want.img)
    assert torch.equal(got.img_true_shape, want.img_true_shape)
    assert torch.equal(got.img_shape, want.img_shape)
    assert got.uimg.is_cuda and got.uimg.dtype == torch.float32
    assert torch.equal(got.uimg.cpu(), want.uimg)
    # a uint8 frame with a CPU device goes through the host path
    cpu = create_frame(0, u8, device="cpu")
    assert torch.equal(cpu.img, want.img.cpu()) and torch.equal(cpu.uimg, want.uimg)


@pytest.mark.gpu
def test_frame_loader_device_ingest_matches_host(tmp_path, monkeypatch):
    from splatt3r_amd.dataio import FrameLoader, TUMDataset, write_synthetic_tum
    ds = TUMDataset(write_synthetic_tum(tmp_path / "seq", 4, seed=3))
    host = FrameLoader(ds, "cuda", workers=2, depth=3, ingest="host")
    # more frames than staging buffers per worker: the pinned ring is reused
    device = FrameLoader(ds, "cuda", workers=1, depth=3, ingest="device")
    n = 0
    for a, b in zip(host, device):
        assert a.index == b.index == n and a.timestamp == b.timestamp
        assert torch.equal(a.consume(), b.consume())
        assert torch.equal(a.true_shape, b.true_shape)
        assert b.uimg.is_cuda and b.uimg.dtype == torch.uint8
        np.testing.assert_array_equal(b.uimg.cpu().numpy(), a.uimg)
        n += 1
    assert n == 4
    host.close()
    device.close()
    monkeypatch.setenv("S3_INGEST", "device")
    env = FrameLoader(ds, "cuda", workers=1, depth=1, stop=1)
    assert env.ingest == "device" and next(env).uimg.is_cuda
    env.close()
    monkeypatch.delenv("S3_INGEST")
    default = FrameLoader(ds, "cuda", workers=1, depth=1, stop=1)
    assert default.ingest == "host"
    default.close()
    with pytest.raises(ValueError):
        FrameLoader(ds, "cuda", ingest="gpu")
