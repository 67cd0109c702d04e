"""Lens undistortion (splatt3r_amd/intrinsics.py, include/s3u.h,
csrc/undistort.hip): cv2's getOptimalNewCameraMatrix, initUndistortRectifyMap
and 8-bit INTER_LINEAR remap restated on the host, the remap as a HIP kernel,
and the readers and frame loop that use them (dataloader.py:67-116, 277-327).

Every comparison is exact or carries a bound stated where it is used.
References: tests/undistort_ref64.py (float64, independent of the code under
test) for the host functions; `remap_u8` -- itself checked against the
float64 bilinear -- for the device.
"""
import functools
import threading

import numpy as np
import pytest
import torch

from undistort_ref64 import (CAMERAS, K_of, bilinear64, direct_maps, distort64, edge_case_maps,
                             five_iterations64, noise_u8, quantised_coords, ulp32)


@functools.lru_cache(maxsize=None)
def camera(name, center, scale=1):
    """(K, D, K_opt, mapx, mapy, W, H) of a test camera, its intrinsics and
    size divided by `scale`; computed once and shared (read-only maps)."""
    from splatt3r_amd import intrinsics as I
    f4, D, W, H = CAMERAS[name]
    W, H = W // scale, H // scale
    K = K_of(f4, scale)
    K_opt = I.get_optimal_new_camera_matrix(K, D, (W, H), 0, (W, H), center=center)
    mapx, mapy = I.init_undistort_rectify_map(K, D, K_opt, (W, H))
    for a in (K, K_opt, mapx, mapy):
        a.setflags(write=False)
    return K, D, K_opt, mapx, mapy, W, H


def small_intrinsics(name):
    """An Intrinsics of the camera at 1/8 scale (EuRoC 94 x 60, TUM 80 x 60)."""
    from splatt3r_amd.intrinsics import Intrinsics
    K, D, K_opt, mapx, mapy, W, H = camera(name, True, 8)
    return Intrinsics(512, W, H, K.copy(), K_opt.copy(), np.array(D), mapx, mapy)


# ------------------------------------------------------------------- CPU ---
def test_zero_distortion_without_centering_is_the_identity():
    from splatt3r_amd import intrinsics as I
    f4, _, W, H = CAMERAS["euroc"]
    K = K_of(f4)
    K_opt = I.get_optimal_new_camera_matrix(K, np.zeros(4), (W, H), 0, (W, H), center=False)
    # the 81 points are stored as float32: about 6e-8 relative per coordinate
    for r, c in ((0, 0), (1, 1), (0, 2), (1, 2)):
        assert abs(K_opt[r, c] - K[r, c]) <= 1e-6 * abs(K[r, c]), (r, c, K_opt[r, c], K[r, c])
    assert np.array_equal(K_opt[[0, 1, 1, 2, 2, 2], [1, 0, 0, 0, 1, 2]], K[[0, 1, 1, 2, 2, 2], [1, 0, 0, 0, 1, 2]])
    # the new camera equal to the old one: every pixel maps to itself
    mapx, mapy = I.init_undistort_rectify_map(K, np.zeros(4), K, (W, H))
    assert mapx.dtype == np.float32 and mapx.shape == (H, W) == mapy.shape
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ex, ey = np.abs(mapx - j) / ulp32(np.maximum(j, 1)), np.abs(mapy - i) / ulp32(np.maximum(i, 1))
    print(f"identity maps: max error {ex.max():.3f} / {ey.max():.3f} float32 ulp")
    assert ex.max() <= 1.0 and ey.max() <= 1.0
    img = noise_u8(H, W, 3, 0)
    assert np.array_equal(I.remap_u8(img, np.rint(mapx), np.rint(mapy)), img)
    assert np.array_equal(I.remap_u8(img, mapx, mapy), img)     # 1 ulp << 1/64 pixel
    assert np.array_equal(I.remap_u8(img[..., 0].copy(), mapx, mapy), img[..., 0])
    # through K_opt itself: its entries carry the float32 storage error above
    # (<= 1e-6 relative), which moves a coordinate by <= 1e-6 * (j + cx) <
    # 2e-6 * W pixels -- far more than an ulp of a small coordinate, far less
    # than the 1/64 pixel at which the 1/32 quantisation would change
    ox, oy = I.init_undistort_rectify_map(K, np.zeros(4), K_opt, (W, H))
    assert max(np.abs(ox - j).max(), np.abs(oy - i).max()) <= 2e-6 * W
    assert np.array_equal(I.remap_u8(img, ox, oy), img)


def test_zero_distortion_with_centering_moves_the_principal_point_only():
    from splatt3r_amd import intrinsics as I
    for name in CAMERAS:
        f4, _, W, H = CAMERAS[name]
        K = K_of(f4)
        K_opt = I.get_optimal_new_camera_matrix(K, np.zeros(4), (W, H), 0, (W, H), center=True)
        assert K_opt[0, 2] == (W - 1) / 2 and K_opt[1, 2] == (H - 1) / 2
        s = K_opt[0, 0] / K[0, 0]
        assert s >= 1.0                       # the centred view is cut inside the image
        assert K_opt[1, 1] == K[1, 1] * s or abs(K_opt[1, 1] / K[1, 1] - s) <= 4e-16 * s


@pytest.mark.parametrize("name", sorted(CAMERAS))
@pytest.mark.parametrize("center", [True, False])
def test_maps_match_a_direct_float64_evaluation(name, center):
    """<= 1 float32 ulp of the value: the cast contributes <= 0.5 ulp and the
    running double sums along a row can flip that rounding."""
    K, D, K_opt, mapx, mapy, W, H = camera(name, center)
    rx, ry = direct_maps(K, D, K_opt, W, H)
    ex, ey = np.abs(mapx - rx) / ulp32(rx), np.abs(mapy - ry) / ulp32(ry)
    print(f"{name} center={center}: max map error {ex.max():.3f} / {ey.max():.3f} float32 ulp")
    assert ex.max() <= 1.0 and ey.max() <= 1.0
    # alpha = 0: every pixel of the new view reads inside the source (half a pixel of slack)
    assert mapx.min() > -0.5 and mapx.max() < W - 0.5 and mapy.min() > -0.5 and mapy.max() < H - 0.5


# The residual of cv2's five fixed-point iterations at the 9x9 grid, in pixels.
# The issue's first bound is 0.01 px (cv2's stopping scale for this routine);
# both cameras miss it: the iteration contracts by about 1/3 per step here
# (EuRoC 31.8, 8.68, 2.64, 0.871, 0.290 px after steps 1..5; TUM fr1 13.2,
# 3.99, 1.29, 0.412, 0.132 px; step 10 reaches 1.3e-3 / 4.4e-4 px), so five
# steps stop at the values below.  cv2 does not iterate further in
# getOptimalNewCameraMatrix, and neither does this: the bound is the recorded
# residual, as the issue prescribes for this case.
FIFTH_ITERATE_RESIDUAL_PX = {"euroc": 0.2903, "tum_fr1": 0.1318}


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_undistort_points_inverts_the_distortion(name):
    """Distorting the fifth iterate returns the 9x9 grid within the recorded
    residual of five iterations (0.01 px, cv2's stopping scale, is missed by
    both cameras: see FIFTH_ITERATE_RESIDUAL_PX), and the iterate itself
    equals an independent scalar evaluation of the five steps."""
    from splatt3r_amd import intrinsics as I
    f4, D, W, H = CAMERAS[name]
    K = K_of(f4)
    g = np.arange(9, dtype=np.float64)
    pts = np.stack(np.meshgrid(g * (W - 1) / 8, g * (H - 1) / 8), -1).reshape(-1, 2)
    und = I.undistort_points(pts, K, D)
    assert und.dtype == np.float32 and und.shape == (81, 2)
    u, v = distort64(und[:, 0].astype(np.float64), und[:, 1].astype(np.float64), K, D)
    err = np.hypot(u - pts[:, 0], v - pts[:, 1])
    print(f"{name}: max residual of the fifth iterate {err.max():.4e} px")
    assert err.max() <= FIFTH_ITERATE_RESIDUAL_PX[name]
    ref = five_iterations64(pts, K, D)
    assert np.abs(und - ref).max() <= ulp32(np.abs(ref).max())      # the float32 store
    # with P the output is in P's pixels
    und_p = I.undistort_points(pts, K, D, P=K)
    want = np.stack([K[0, 0] * und[:, 0].astype(np.float64) + K[0, 2],
                     K[1, 1] * und[:, 1].astype(np.float64) + K[1, 2]], 1)
    assert np.abs(und_p - want).max() <= 2 * ulp32(max(W, H))


def test_get_rectangles_inner_and_outer_at_alpha_one():
    """inner lies inside outer; at alpha = 1 (center off) the whole source is
    kept: the outer rectangle's corners land on the new image's corners."""
    from splatt3r_amd import intrinsics as I
    for name in CAMERAS:
        f4, D, W, H = CAMERAS[name]
        K = K_of(f4)
        inner, outer = I.get_rectangles(K, D, None, W, H)
        assert outer[0] <= inner[0] and outer[1] <= inner[1]
        assert outer[0] + outer[2] >= inner[0] + inner[2] and outer[1] + outer[3] >= inner[1] + inner[3]
        K1 = I.get_optimal_new_camera_matrix(K, D, (W, H), 1.0, (W, H), center=False)
        x0, y0 = K1[0, 0] * outer[0] + K1[0, 2], K1[1, 1] * outer[1] + K1[1, 2]
        x1 = K1[0, 0] * (outer[0] + outer[2]) + K1[0, 2]
        y1 = K1[1, 1] * (outer[1] + outer[3]) + K1[1, 2]
        assert max(abs(x0), abs(y0), abs(x1 - (W - 1)), abs(y1 - (H - 1))) <= 1e-9 * W
        K0 = I.get_optimal_new_camera_matrix(K, D, (W, H), 0.0, (W, H), center=False)
        Kh = I.get_optimal_new_camera_matrix(K, D, (W, H), 0.5, (W, H), center=False)
        np.testing.assert_allclose(Kh, 0.5 * K0 + 0.5 * K1, rtol=1e-15)
        # centred: alpha = 1 scales by the smallest of the four ratios, so it zooms out
        Kc0 = I.get_optimal_new_camera_matrix(K, D, (W, H), 0.0, (W, H), center=True)
        Kc1 = I.get_optimal_new_camera_matrix(K, D, (W, H), 1.0, (W, H), center=True)
        assert Kc1[0, 0] < Kc0[0, 0] and Kc1[0, 2] == Kc0[0, 2] == (W - 1) / 2


@pytest.mark.parametrize("channels", [0, 3])
def test_remap_u8_rounds_the_exact_bilinear(channels):
    """Against the float64 bilinear at the quantised coordinates, zero outside
    the image: |out - exact| <= 0.5 and out == floor(exact + 0.5)."""
    from splatt3r_amd.intrinsics import remap_u8
    H, W = 37, 53
    rng = np.random.default_rng(11)
    mapx = rng.uniform(-3.0, W + 2.0, (29, 41)).astype(np.float32)
    mapy = rng.uniform(-3.0, H + 2.0, (29, 41)).astype(np.float32)
    for maps in ((mapx, mapy), edge_case_maps(W, H)):
        img = noise_u8(H, W, channels, 4)
        out = remap_u8(img, *maps)
        exact = bilinear64(img, *maps)
        assert out.dtype == np.uint8 and out.shape == exact.shape
        assert np.abs(out - exact).max() <= 0.5
        assert np.array_equal(out, np.floor(exact + 0.5).astype(np.uint8))


def test_quantisation_edge_cases():
    from splatt3r_amd.intrinsics import _quantise, remap_u8
    m = np.float32([[3.015625, 3.046875, -17 / 32, 2.0 ** 20, -2.0 ** 20, -0.5, -1.0, 52 + 1 / 32]])
    i, f = _quantise(m)
    s = i * 32 + f
    assert s[0, :2].tolist() == [96, 98]                     # 96.5 -> 96, 97.5 -> 98: half to even
    assert (i[0, 2], f[0, 2]) == (-1, 15)                    # arithmetic shift, two's-complement mask
    assert i[0, 3] == 32767 and i[0, 4] == -32768            # saturated to the short range
    assert (i[0, 5], f[0, 5]) == (-1, 16) and (i[0, 6], f[0, 6]) == (-1, 0)
    assert (i[0, 7], f[0, 7]) == (52, 1)
    qi, qf = quantised_coords(m)
    assert np.array_equal(i, qi) and np.array_equal(f, qf)
    img = noise_u8(37, 53, 3, 4)
    out = remap_u8(img, m, np.full_like(m, 5.0))
    assert not out[0, 3].any() and not out[0, 4].any()       # +-2^20: every tap outside -> 0
    # -0.5: half of column 0 (p00 outside); 52 + 1/32: 31/32 of the last column
    assert np.array_equal(out[0, 5], (16 * img[5, 0].astype(int) * 32 + 512) >> 10)
    assert np.array_equal(out[0, 7], (31 * 32 * img[5, 52].astype(int) + 512) >> 10)


def test_map_and_coefficient_validation():
    from splatt3r_amd import intrinsics as I
    ok = np.zeros((4, 5), np.float32)
    I.UndistortMap(ok, ok, 5, 4)
    bad = []
    for v in (np.nan, np.inf, -np.inf, np.float32(2.0 ** 20) * np.float32(1.0000002), -1.1e6):
        m = ok.copy()
        m[1, 2] = v
        bad.append(m)
    bad += [ok.astype(np.float64), ok.astype(np.int32), ok[0], ok[None], np.zeros((0, 5), np.float32),
            ok.tolist()]
    for m in bad:
        for pair in ((m, ok), (ok, m)):
            with pytest.raises(ValueError):
                I.check_maps(*pair)
            with pytest.raises(ValueError):
                I.UndistortMap(*pair, 5, 4)
    with pytest.raises(ValueError):
        I.check_maps(ok, np.zeros((5, 4), np.float32))
    with pytest.raises(ValueError):
        I.remap_u8(np.zeros((4, 5, 3), np.uint8), ok, ok.astype(np.float64))
    edge = ok.copy()
    edge[0, 0], edge[0, 1] = 2.0 ** 20, -2.0 ** 20           # the limit itself is allowed
    I.check_maps(edge, edge)
    K = K_of(CAMERAS["euroc"][0])
    with pytest.raises(ValueError):
        I.Intrinsics(512, 5, 4, K, K.copy(), np.zeros(4), bad[0], ok)
    with pytest.raises(ValueError):                          # maps of another size than the camera
        I.Intrinsics(512, 6, 4, K, K.copy(), np.zeros(4), ok, ok)
    for n in (0, 3, 6, 7, 9, 12, 14):
        with pytest.raises(ValueError):
            I.get_optimal_new_camera_matrix(K, np.zeros(n), (752, 480))
        with pytest.raises(ValueError):
            I.init_undistort_rectify_map(K, np.zeros(n), K, (8, 8))
        with pytest.raises(ValueError):
            I.undistort_points(np.zeros((1, 2)), K, np.zeros(n))
    with pytest.raises(ValueError):                          # calib = 4 intrinsics + 6 coefficients
        I.Intrinsics.from_calib(512, 752, 480, [*CAMERAS["euroc"][0], *np.zeros(6)],
                                always_undistort=True)
    # 8 coefficients: the rational model's denominator is used
    mx8, _ = I.init_undistort_rectify_map(K, [0.1, 0, 0, 0, 0, 0.1, 0, 0], K, (64, 48))
    mx0, _ = I.init_undistort_rectify_map(K, np.zeros(4), K, (64, 48))
    assert np.abs(mx8 - mx0).max() <= 2 * ulp32(64)          # k1 == k4: kr == 1


@pytest.mark.parametrize("W,H", [(752, 480), (640, 480)])
def test_k_frame_follows_the_ingest_geometry(W, H):
    """dataloader.py:286-293 on resize_img's transformation tuple."""
    from splatt3r_amd.config import config
    from splatt3r_amd.ingest import ingest_geometry
    from splatt3r_amd.intrinsics import Intrinsics
    from splatt3r_amd.splatt3r_utils import resize_img
    name = "euroc" if W == 752 else "tum_fr1"
    intr = Intrinsics.from_calib(512, W, H, [*CAMERAS[name][0], *CAMERAS[name][1]],
                                 always_undistort=True)
    assert (intr.img_size, intr.W, intr.H) == (512, W, H)
    assert intr.mapx.shape == (H, W) and intr.mapx.dtype == np.float32
    assert np.array_equal(intr.K_orig, K_of(CAMERAS[name][0]))
    assert np.array_equal(intr.distortion, CAMERAS[name][1])
    assert config["dataset"]["center_principle_point"] is True
    assert np.array_equal(intr.K, camera(name, True)[2])
    assert np.array_equal(intr.mapx, camera(name, True)[3])
    sw, sh, hw, hh = ingest_geometry(H, W, 512)[3]
    assert (sw, sh, hw, hh) == resize_img(np.zeros((H, W, 3), np.float32), 512,
                                          return_transformation=True)[1]
    K = intr.K
    want = np.array([[K[0, 0] / sw, 0, K[0, 2] / sw - hw], [0, K[1, 1] / sh, K[1, 2] / sh - hh],
                     [0, 0, 1]])
    assert np.array_equal(intr.K_frame, want)
    assert not np.array_equal(intr.K_frame, intr.K)
    # use_calib off and no always_undistort: no calibration at all (dataloader.py:300-301)
    assert config["use_calib"] is False
    assert Intrinsics.from_calib(512, W, H, CAMERAS[name][0]) is None


def test_euroc_reader_round_trips_the_synthetic_sequence(tmp_path):
    from PIL import Image
    from splatt3r_amd import dataio
    from splatt3r_amd.intrinsics import remap_u8
    root = dataio.write_synthetic_euroc(tmp_path / "euroc" / "MH_01", 3)
    ds = dataio.EurocDataset(root)
    assert len(ds) == 3 and ds.use_calibration and ds.has_calib()
    assert ds.timestamps.dtype == np.int64 and np.all(np.diff(ds.timestamps) == 50_000_000)
    intr = ds.camera_intrinsics
    assert (intr.W, intr.H) == (752, 480)
    assert np.array_equal(intr.K_orig, K_of(CAMERAS["euroc"][0]))
    assert np.array_equal(intr.distortion, CAMERAS["euroc"][1])
    assert np.array_equal(intr.K, camera("euroc", True)[2])
    raw = ds.read_img(1)
    assert raw.shape == (480, 752) and raw.dtype == np.uint8
    assert np.array_equal(raw, np.asarray(Image.open(ds.rgb_files[1])))
    t, img = ds[1]
    assert t == ds.timestamps[1] and img.shape == (480, 752, 3) and img.dtype == np.float32
    und = remap_u8(raw, intr.mapx, intr.mapy)
    assert np.array_equal(img, np.repeat(und[..., None], 3, 2).astype(np.float32) / 255.0)
    assert not np.array_equal(und, raw)
    assert isinstance(dataio.load_dataset(str(root)), dataio.EurocDataset)
    assert len(dataio.EurocDataset(root, subsample=2)) == 2
    with pytest.raises(ValueError, match="tum"):
        dataio.load_dataset(str(tmp_path / "eth3d" / "x"))


def test_tum_reader_calibration_follows_the_path(tmp_path):
    from splatt3r_amd import dataio
    from splatt3r_amd.config import config
    from splatt3r_amd.intrinsics import remap_u8
    plain = dataio.write_synthetic_tum(tmp_path / "seq", 2, seed=1)
    named = dataio.write_synthetic_tum(tmp_path / "tum" / "rgbd_dataset_freiburg1_x", 2, seed=1)
    raw = dataio.TUMDataset(plain).read_img(1)
    assert config["use_calib"] is False
    for root in (plain, named):            # use_calib off: no calibration, today's bytes
        ds = dataio.TUMDataset(root)
        assert not ds.has_calib() and ds.camera_intrinsics is None and not ds.use_calibration
        assert np.array_equal(ds[1][1], raw.astype(np.float32) / 255.0)
    config["use_calib"] = True
    try:
        ds = dataio.load_dataset(str(named))
        assert isinstance(ds, dataio.TUMDataset) and ds.has_calib() and ds.use_calibration
        intr = ds.camera_intrinsics
        assert np.array_equal(intr.K_orig, K_of(CAMERAS["tum_fr1"][0]))
        assert np.array_equal(intr.distortion, CAMERAS["tum_fr1"][1])
        assert np.array_equal(intr.K, camera("tum_fr1", True)[2])
        assert np.array_equal(ds[1][1], remap_u8(raw, intr.mapx, intr.mapy).astype(np.float32) / 255.0)
        fr3 = dataio.TUMDataset(dataio.write_synthetic_tum(tmp_path / "rgbd_dataset_freiburg3_y", 1))
        assert np.array_equal(fr3.camera_intrinsics.distortion, np.zeros(4))
        assert fr3.camera_intrinsics.K_orig[0, 0] == 535.4
        ds = dataio.TUMDataset(plain)      # a path without freiburgN: none, today's bytes
        assert not ds.has_calib() and not ds.use_calibration
        assert np.array_equal(ds[1][1], raw.astype(np.float32) / 255.0)
    finally:
        config["use_calib"] = False


def test_abi_rejects_bad_arguments_before_any_device_work():
    """Status 1 with a message; the pointers are never dereferenced (they are
    not device memory here)."""
    from splatt3r_amd import _lib, ingest  # noqa: F401  (ingest registers s3u_* too)
    assert "s3u_remap" in _lib.SIGNATURES
    lib = _lib.lib()

    def call(src=0x10000, B=1, H=8, W=8, C=3, mapx=0x1000, mapy=0x2000, oh=8, ow=8, dst=0x20000):
        return lib.s3u_remap(src, B, H, W, C, mapx, mapy, oh, ow, dst, None)

    bad = ((dict(src=None), b"null"), (dict(mapx=None), b"null"), (dict(mapy=None), b"null"),
           (dict(dst=None), b"null"), (dict(C=2), b"C = 2"), (dict(C=0), b"C = 0"),
           (dict(C=4), b"C = 4"), (dict(B=0), b"non-positive"), (dict(H=0), b"non-positive"),
           (dict(W=-1), b"non-positive"), (dict(oh=0), b"non-positive"),
           (dict(ow=-5), b"non-positive"), (dict(W=40000), b"at most 32767"),
           (dict(dst=0x10000), b"overlaps"), (dict(dst=0x10000 + 191), b"overlaps"),
           (dict(dst=0x10000 - 191), b"overlaps"), (dict(B=2, dst=0x10000 + 383), b"overlaps"))
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


def test_python_validation_needs_no_gpu():
    intr = small_intrinsics("euroc")
    good = np.zeros((intr.H, intr.W, 3), np.uint8)
    for bad in (good.astype(np.float32), good[:, ::2], np.zeros((intr.H, intr.W, 2), np.uint8),
                np.zeros((intr.H,), np.uint8), torch.zeros(intr.H, intr.W, 3)):
        with pytest.raises(RuntimeError):
            intr.remap(bad, device="cuda")
    with pytest.raises(ValueError):
        intr.remap(np.zeros((intr.H + 1, intr.W, 3), np.uint8), device="cuda")
    with pytest.raises(RuntimeError, match="GPU only"):
        intr.remap(good, device="cpu")
    assert intr.remap(good).shape == good.shape              # host path
    assert intr.remap(good[..., 0].copy()).shape == (intr.H, intr.W)


def test_matches_cv2_where_it_is_installed():
    """Exact agreement of K_opt, both maps and the remapped bytes with cv2."""
    cv2 = pytest.importorskip("cv2")
    from splatt3r_amd.intrinsics import remap_u8
    for name in CAMERAS:
        for center in (True, False):
            K, D, K_opt, mapx, mapy, W, H = camera(name, center)
            want, _ = cv2.getOptimalNewCameraMatrix(K, np.array(D), (W, H), 0, (W, H),
                                                    centerPrincipalPoint=center)
            assert np.array_equal(K_opt, want)
            wx, wy = cv2.initUndistortRectifyMap(K, np.array(D), None, want, (W, H), cv2.CV_32FC1)
            assert np.array_equal(mapx, wx) and np.array_equal(mapy, wy)
            for c in (0, 3):
                img = np.array(noise_u8(H, W, c, 8))
                assert np.array_equal(remap_u8(img, mapx, mapy),
                                      cv2.remap(img, wx, wy, cv2.INTER_LINEAR))


# ------------------------------------------------------------------- GPU ---
def device_remap(src_u8, mapx, mapy, W, H):
    from splatt3r_amd.intrinsics import UndistortMap
    out, _ = UndistortMap(mapx, mapy, W, H).remap_device(src_u8)
    return out


def host_remap(frames, mapx, mapy):
    from splatt3r_amd.intrinsics import remap_u8
    return torch.from_numpy(np.stack([remap_u8(np.ascontiguousarray(f), mapx, mapy) for f in frames]))


@pytest.mark.gpu
def test_device_remap_edge_case_map():
    """53 x 37 x 3, B = 2: ties, the last row and column, negative
    coordinates, +-2^20 and random values, on a size that is no multiple of
    the four-pixel groups."""
    W, H = 53, 37
    mapx, mapy = edge_case_maps(W, H)
    frames = np.stack([noise_u8(H, W, 3, 20), noise_u8(H, W, 3, 21)])
    got = device_remap(frames, mapx, mapy, W, H)
    assert got.shape == (2, H, W, 3) and got.dtype == torch.uint8 and got.is_cuda
    assert torch.equal(got.cpu(), host_remap(frames, mapx, mapy))


@pytest.mark.gpu
def test_device_remap_output_size_differs_from_the_source():
    W, H = 53, 37
    rng = np.random.default_rng(12)
    mapx = rng.uniform(-2.0, W + 1.0, (29, 41)).astype(np.float32)
    mapy = rng.uniform(-2.0, H + 1.0, (29, 41)).astype(np.float32)
    mapx[0, :2], mapy[0, :2] = (0.0, W - 1), (0.0, H - 1)    # the first and the last source pixel
    frames = np.stack([noise_u8(H, W, 3, 20), noise_u8(H, W, 3, 21), noise_u8(H, W, 3, 22)])
    got = device_remap(frames, mapx, mapy, W, H)            # 29 * 41 * 3 odd: frames 1, 2 unaligned
    assert got.shape == (3, 29, 41, 3)
    assert torch.equal(got.cpu(), host_remap(frames, mapx, mapy))
    # unaligned maps and output (views one element into a buffer)
    from splatt3r_amd import _lib
    src = torch.from_numpy(frames).cuda()
    # ... and a source that starts at every byte alignment: the first and the
    # last pixel's dword runs would leave the buffer (the maps hit both)
    want = host_remap(frames, mapx, mapy)
    for c, frames_c in ((3, frames), (1, frames[..., :1])):
        want_c = want if c == 3 else host_remap(np.repeat(frames_c, 3, 3), mapx, mapy)
        for mis in (1, 2, 3):
            raw = torch.zeros(frames_c.size + 4, dtype=torch.uint8, device="cuda")
            raw[mis:mis + frames_c.size] = torch.from_numpy(np.ascontiguousarray(frames_c)).cuda().ravel()
            view = raw[mis:mis + frames_c.size].view(3, H, W, c)
            assert view.data_ptr() % 4 == mis
            assert torch.equal(device_remap(view, mapx, mapy, W, H).cpu(), want_c), (c, mis)
    mx = torch.zeros(29 * 41 + 1, device="cuda")
    my = torch.zeros(29 * 41 + 1, device="cuda")
    mx[1:], my[1:] = torch.from_numpy(mapx).cuda().ravel(), torch.from_numpy(mapy).cuda().ravel()
    buf = torch.zeros(3 * 29 * 41 * 3 + 2, dtype=torch.uint8, device="cuda")
    _lib.call("s3u_remap", src.data_ptr(), 3, H, W, 3, mx[1:].data_ptr(), my[1:].data_ptr(), 29, 41,
              buf[1:].data_ptr(), _lib.stream())
    assert torch.equal(buf[1:-1].view(3, 29, 41, 3), got)
    assert buf[0] == 0 and buf[-1] == 0


@pytest.mark.gpu
def test_device_remap_greyscale_equals_the_replicated_image():
    W, H = 53, 37
    mapx, mapy = edge_case_maps(W, H)
    grey = np.stack([noise_u8(H, W, 0, 30), noise_u8(H, W, 0, 31)])
    got = device_remap(grey[..., None].copy(), mapx, mapy, W, H)
    rgb = np.repeat(grey[..., None], 3, axis=3)
    assert got.shape == (2, H, W, 3)
    assert torch.equal(got, device_remap(rgb, mapx, mapy, W, H))
    assert torch.equal(got.cpu(), host_remap(rgb, mapx, mapy))
    one = device_remap(grey[0].copy(), mapx, mapy, W, H)    # [H,W]
    assert torch.equal(one[0], got[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_device_remap_radial_tangential_camera(name):
    """The camera at 1/8 scale (EuRoC 94 x 60, TUM fr1 80 x 60), maps from
    Intrinsics."""
    intr = small_intrinsics(name)
    img = noise_u8(intr.H, intr.W, 3, 40)
    got = intr.remap(img, device="cuda")
    assert got.shape == (intr.H, intr.W, 3) and got.is_cuda
    assert torch.equal(got.cpu(), torch.from_numpy(intr.remap(np.array(img))))
    assert torch.equal(intr.remap(torch.from_numpy(np.array(img)).cuda()), got)


@pytest.mark.gpu
def test_device_remap_batch_equals_single_launches():
    intr = small_intrinsics("euroc")
    frames = np.stack([noise_u8(intr.H, intr.W, 3, 50 + i) for i in range(5)])
    got = intr.remap(frames, device="cuda")
    assert got.shape == (5, intr.H, intr.W, 3)
    for i in range(5):
        assert torch.equal(got[i], intr.remap(frames[i].copy(), device="cuda"))
    assert torch.equal(got.cpu(), host_remap(frames, intr.mapx, intr.mapy))


@functools.lru_cache(maxsize=None)
def euroc_intrinsics():
    from splatt3r_amd.intrinsics import Intrinsics
    K, D, K_opt, mapx, mapy, W, H = camera("euroc", True)
    return Intrinsics(512, W, H, K.copy(), K_opt.copy(), np.array(D), mapx, mapy)


@pytest.mark.gpu
def test_resize_img_device_with_undistort_matches_the_host_path():
    """One 480 x 752 frame: remap + ingest on the device equal
    resize_img(remap_u8(raw) / 255, 512)."""
    from splatt3r_amd import ingest
    from splatt3r_amd.splatt3r_utils import resize_img
    intr = euroc_intrinsics()
    raw = noise_u8(480, 752, 3, 60)
    und = intr.remap(np.array(raw))
    want, want_tr = resize_img(und.astype(np.float32) / 255.0, 512, return_transformation=True)
    res, tr = ingest.resize_img_device(raw, 512, return_transformation=True, undistort=intr)
    assert torch.equal(res["img"].cpu(), want["img"])
    np.testing.assert_array_equal(res["unnormalized_img"].cpu().numpy(), want["unnormalized_img"])
    np.testing.assert_array_equal(res["true_shape"], want["true_shape"])
    assert tr == want_tr
    # the unit image create_frame keeps (uimg): the host's quotients
    assert torch.equal(ingest.unit_image(res["unnormalized_img"]).cpu(),
                       torch.from_numpy(want["unnormalized_img"].astype(np.float32) / 255.0))
    # greyscale in: the same as its three-channel copy
    g = ingest.resize_img_device(np.array(raw[..., 0]), 512, undistort=intr)
    r3 = ingest.resize_img_device(np.repeat(raw[..., :1], 3, 2), 512, undistort=intr)
    assert torch.equal(g["img"], r3["img"])
    assert torch.equal(g["unnormalized_img"], r3["unnormalized_img"])
    # the default leaves the plain ingest as it was
    plain = ingest.resize_img_device(raw, 512)
    assert torch.equal(plain["img"].cpu(),
                       resize_img(np.array(raw).astype(np.float32) / 255.0, 512)["img"])


@pytest.mark.gpu
def test_frame_loader_device_and_host_ingest_agree_on_euroc(tmp_path):
    from splatt3r_amd.dataio import EurocDataset, FrameLoader, write_synthetic_euroc
    ds = EurocDataset(write_synthetic_euroc(tmp_path / "euroc" / "MH_01", 3))
    out = {}
    for mode in ("device", "host"):
        loader = FrameLoader(ds, "cuda", workers=2, depth=3, ingest=mode)
        frames = []
        for lf in loader:
            img = lf.consume()
            torch.cuda.current_stream().synchronize()
            uimg = lf.uimg.cpu().numpy() if torch.is_tensor(lf.uimg) else np.asarray(lf.uimg)
            frames.append((img.cpu(), uimg, lf.true_shape.tolist(), lf.timestamp))
        loader.close()
        out[mode] = frames
    assert len(out["device"]) == len(out["host"]) == 3
    for d, h in zip(out["device"], out["host"]):
        assert torch.equal(d[0], h[0]) and d[0].shape == (1, 3, 320, 512)
        np.testing.assert_array_equal(d[1], h[1])
        assert d[2] == h[2] == [[320, 512]] and d[3] == h[3]
    # and the frames are the undistorted ones
    from splatt3r_amd.splatt3r_utils import resize_img
    want = resize_img(ds[0][1], 512)
    assert torch.equal(out["device"][0][0], want["img"])


@pytest.mark.gpu
def test_frontend_installs_k_frame_from_the_intrinsics(tmp_path):
    """Construction only: with use_calib on, `intrinsics=` (an Intrinsics or a
    dataset) supplies K_frame; an explicit K wins."""
    import types
    from splatt3r_amd.config import config
    from splatt3r_amd.slam import Frontend
    intr = euroc_intrinsics()
    want = torch.from_numpy(intr.K_frame).to("cuda", dtype=torch.float32)
    model = types.SimpleNamespace()
    config["use_calib"] = True
    try:
        fe = Frontend(model, device="cuda", render=False, intrinsics=intr)
        assert torch.equal(fe.keyframes.get_intrinsics(), want) and torch.equal(fe.K, want)
        ds = types.SimpleNamespace(camera_intrinsics=intr)
        fe = Frontend(model, device="cuda", render=False, intrinsics=ds)
        assert torch.equal(fe.keyframes.get_intrinsics(), want)
        K = torch.eye(3, device="cuda")
        fe = Frontend(model, device="cuda", render=False, K=K, intrinsics=intr)
        assert fe.keyframes.get_intrinsics() is K
        with pytest.raises(ValueError):
            Frontend(model, device="cuda", render=False)
        with pytest.raises(ValueError):
            Frontend(model, device="cuda", render=False,
                     intrinsics=types.SimpleNamespace(camera_intrinsics=None))
    finally:
        config["use_calib"] = False
