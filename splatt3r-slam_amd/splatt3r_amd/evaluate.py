"""Harness output formats: TUM trajectory, PLY point
cloud, keyframe PNGs — splatt3r_slam/evaluate.py.

Same function names, argument meaning and file bytes as the reference:

* `save_traj` (evaluate.py:23-44): one line per keyframe,
  `"{t} {x} {y} {z} {qx} {qy} {qz} {qw}"` with the Sim3 scale dropped
  (`as_SE3`, lietorch_utils.py:6-13) and each value formatted from its
  float32 the way the reference's f-string formats numpy float32 scalars.
* `save_ply` (evaluate.py:88-106): binary little-endian PLY, vertex element
  `x y z` float + `red green blue` uchar — the header plyfile writes for
  that structured dtype (plyfile is not installed here; the bytes are
  written directly).
* `save_reconstruction` (evaluate.py:47-71): world points `T_WC.act(X_canon)`
  of every keyframe, colours `uint8(uimg * 255)`, kept where the average
  confidence exceeds `c_conf_threshold`.
* `save_keyframes` (evaluate.py:74-85): `{t}.png` per keyframe (PIL instead
  of cv2; cv2's BGR swap followed by its BGR->RGB write is the identity).

Render quality has no counterpart in the reference's evaluate.py (its numbers
come from splatt3r_core/main.py log_metrics): `eval_renders`,
`eval_keyframe_renders` and `save_render_metrics` score rendered against
camera images on the device (splatt3r_amd/photometric.py), and
`eval_novel_view_renders` scores a keyframe against its neighbour's Gaussians
over the co-visibility mask (splatt3r_amd/loss_mask.py).

The Gaussian map itself leaves the process as a 3DGS splat file, which the
reference's evaluate.py has no function for either: `write_splat_ply`,
`read_splat_ply` and `save_gaussian_splats` (format and values: include/s3w.h
s3w_map_to_splats).

Geometry against ground truth has no counterpart either (the reference's
scripts call `evo_ape tum gt est -as` for the trajectory and score no
surface): `eval_reconstruction` (accuracy, completion, Chamfer distance,
F-score over exact nearest neighbours on the device, splatt3r_amd/nn.py,
include/s3k.h), `align_umeyama`, `read_traj`, `associate`, `eval_trajectory`
(host float64; the quantity evo reports, parity with evo unpinned: it is not
installed here) and `save_geometry_metrics` / `load_geometry_metrics`
(DESIGN.md §6s).

save_reconstruction's use_calib branch constrains points to their pixel
rays first (evaluate.py:55-59).  save_traj's `intrinsics` branch calls
`intrinsics.refine_pose_with_calibration(keyframe)` (evaluate.py:42), a
method the reference's Intrinsics class does not define
(dataloader.py:277-317): the reference raises AttributeError there, and so
does this one, with the same exception type.
"""
from __future__ import annotations

import pathlib
from typing import Optional

import numpy as np
import torch

from splatt3r_amd.config import config


def prepare_savedir(args, dataset):
    """evaluate.py:14-20: logs/[save_as]/ and the sequence name."""
    save_dir = pathlib.Path("logs")
    if args.save_as != "default":
        save_dir = save_dir / args.save_as
    save_dir.mkdir(exist_ok=True, parents=True)
    return save_dir, pathlib.Path(dataset.dataset_path).stem


def as_SE3_data(T_WC) -> np.ndarray:
    """lietorch_utils.py:6-13: Sim3 [t, q, s] -> SE3 [t, q] as float32 rows."""
    d = T_WC.data.detach().cpu() if hasattr(T_WC, "data") else torch.as_tensor(T_WC)
    if d.shape[-1] == 7:          # already an SE3 [t, q]
        return d.reshape(-1, 7).numpy().astype(np.float32)
    d = d.reshape(-1, 8)
    return torch.cat([d[:, :3], d[:, 3:7]], -1).numpy().astype(np.float32)


def traj_line(t, pose7: np.ndarray) -> str:
    x, y, z, qx, qy, qz, qw = np.asarray(pose7, np.float32).reshape(-1)
    return f"{t} {x} {y} {z} {qx} {qy} {qz} {qw}\n"


def save_traj(logdir, logfile, timestamps, frames, intrinsics: Optional[object] = None):
    if intrinsics is not None and not hasattr(intrinsics, "refine_pose_with_calibration"):
        raise AttributeError(
            "'Intrinsics' object has no attribute 'refine_pose_with_calibration' "
            "(the reference's save_traj calls a method its Intrinsics does not define, "
            "dataloader.py:277-317)")
    logdir = pathlib.Path(logdir)
    logdir.mkdir(exist_ok=True, parents=True)
    with open(logdir / logfile, "w") as f:
        for i in range(len(frames)):
            kf = frames[i]
            T = kf.T_WC if intrinsics is None else intrinsics.refine_pose_with_calibration(kf)
            f.write(traj_line(timestamps[kf.frame_id], as_SE3_data(T)[0]))


_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {n}\n"
               "property float x\nproperty float y\nproperty float z\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def save_ply(filename, points, colors):
    points = np.asarray(points)
    colors = np.asarray(colors).astype(np.uint8)
    pcd = np.empty(len(points), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                                       ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    pcd["x"], pcd["y"], pcd["z"] = points.T
    pcd["red"], pcd["green"], pcd["blue"] = colors.T
    with open(filename, "wb") as f:
        f.write(_PLY_HEADER.format(n=len(points)).encode("ascii"))
        f.write(pcd.tobytes())


def load_ply(filename):
    """Reader for the files save_ply writes (tests, tooling)."""
    with open(filename, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    n = int(raw[:end].decode().split("element vertex ")[1].split("\n")[0])
    pcd = np.frombuffer(raw[end:], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                                          ("red", "u1"), ("green", "u1"), ("blue", "u1")], count=n)
    pts = np.stack([pcd["x"], pcd["y"], pcd["z"]], -1)
    col = np.stack([pcd["red"], pcd["green"], pcd["blue"]], -1)
    return pts, col


def save_reconstruction(savedir, filename, keyframes, c_conf_threshold):
    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    pts, cols = [], []
    for i in range(len(keyframes)):
        kf = keyframes[i]
        if config.get("use_calib", False):
            from splatt3r_amd.geometry import constrain_points_to_ray
            kf.X_canon = constrain_points_to_ray(kf.img_shape.flatten()[:2], kf.X_canon[None],
                                                 kf.K).squeeze(0)
        pW = kf.T_WC.act(kf.X_canon).cpu().numpy().reshape(-1, 3)
        color = (kf.uimg.cpu().numpy() * 255).astype(np.uint8).reshape(-1, 3)
        valid = kf.get_average_conf().cpu().numpy().astype(np.float32).reshape(-1) > c_conf_threshold
        pts.append(pW[valid])
        cols.append(color[valid])
    save_ply(savedir / filename, np.concatenate(pts, 0), np.concatenate(cols, 0))


# ------------------------------------------------------- 3DGS splat .ply ----
# The file every 3DGS viewer and trainer reads (INRIA convention; the values
# are defined in include/s3w.h s3w_map_to_splats).  Attribute list and order
# as the reference's save_as_ply (splatt3r_core/utils/export.py) with the DC
# band only; its arithmetic is not reproduced (it writes U @ U for the
# rotation, scipy's x y z w order and post-sigmoid opacities).
SPLAT_PROPERTIES = ("x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity",
                    "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")
# what an import needs (the normals are written as 0 and never read)
SPLAT_REQUIRED = tuple(p for p in SPLAT_PROPERTIES if p not in ("nx", "ny", "nz"))
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2",
              "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4",
              "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8",
              "float64": "f8"}


def splat_ply_header(n: int) -> str:
    """The header plyfile writes for one vertex element of 17 float properties."""
    return ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {int(n)}\n"
            + "".join(f"property float {p}\n" for p in SPLAT_PROPERTIES) + "end_header\n")


def write_splat_ply(path, rows):
    """Write a [n, 17] float32 array (columns in SPLAT_PROPERTIES order) as a
    binary little-endian splat .ply: the header, then the rows as they are.
    Host only; one write of the body."""
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != len(SPLAT_PROPERTIES):
        raise ValueError(f"write_splat_ply: rows must be [n, {len(SPLAT_PROPERTIES)}], "
                         f"got {rows.shape}")
    body = np.ascontiguousarray(rows, dtype="<f4")
    with open(path, "wb") as f:
        f.write(splat_ply_header(len(body)).encode("ascii"))
        f.write(body.data)


def read_splat_ply(path) -> dict:
    """Read a 3DGS splat .ply into a dict of numpy arrays keyed by property
    name (every vertex property of the file, each [n]).

    Properties are found by name: any order, and extra ones (`f_rest_*` of a
    file trained elsewhere, anything else) are accepted.  Only the DC band is
    used on import; higher SH bands (`f_rest_*`) are returned here but ignored
    by SharedGaussians.load_ply.  Raises ValueError for an ascii or big-endian
    file, a missing or non-float required property (SPLAT_REQUIRED), and a
    body shorter than the header promises."""
    with open(path, "rb") as f:
        raw = f.read()
    if not raw.startswith(b"ply"):
        raise ValueError(f"{path}: not a PLY file")
    end = raw.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: PLY header has no end_header line")
    body_at = end + len(b"end_header\n")
    fmt, elements = None, []          # elements: [name, count, [(prop, dtype)]]
    for line in raw[:end].decode("ascii", errors="replace").split("\n")[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if tok[1] == "list":
                if elements[-1][0] == "vertex":
                    raise ValueError(f"{path}: list property in the vertex element")
                elements[-1][2] = None        # a variable-size element
            elif elements[-1][2] is not None:
                if tok[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unknown property type {tok[1]!r}")
                elements[-1][2].append((tok[2], "<" + _PLY_TYPES[tok[1]]))
    if fmt != "binary_little_endian":
        raise ValueError(f"{path}: only binary_little_endian PLY is read, file is {fmt}")
    offset, vertex = body_at, None
    for name, count, props in elements:
        if name == "vertex":
            vertex = (count, props)
            break
        if props is None:
            raise ValueError(f"{path}: a list element precedes the vertex element")
        offset += count * np.dtype(props).itemsize
    if vertex is None:
        raise ValueError(f"{path}: no vertex element")
    n, props = vertex
    types = dict(props)
    for p in SPLAT_REQUIRED:
        if p not in types:
            raise ValueError(f"{path}: missing property {p!r}")
        if types[p] != "<f4":
            raise ValueError(f"{path}: property {p!r} is not float")
    dt = np.dtype(props)
    if len(raw) - offset < n * dt.itemsize:
        raise ValueError(f"{path}: truncated body ({len(raw) - offset} bytes for {n} vertices "
                         f"of {dt.itemsize})")
    rec = np.frombuffer(raw, dtype=dt, count=n, offset=offset)
    return {name: np.ascontiguousarray(rec[name]) for name, _ in props}


def save_gaussian_splats(savedir, filename, gmap):
    """Write the Gaussian map as a splat .ply (SharedGaussians.save_ply) into
    savedir, created like save_reconstruction does.  Returns the number of
    Gaussians written, or None when there is no map or it is empty."""
    if gmap is None or gmap.n_gaussians == 0:
        return None
    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    return gmap.save_ply(savedir / filename)


# ------------------------------------------------------ triangle mesh .ply ----
def write_mesh_ply(path, verts, colors, faces):
    """Write a triangle mesh as a binary little-endian .ply: `vertex` with
    x y z float and red green blue uchar (colors in [0, 1], clamped, times 255
    rounded to nearest), `face` with vertex_indices as list uchar int.  Host
    arrays [nv, 3], [nv, 3], [nt, 3]; a mesh without triangles (or vertices)
    is a valid file."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    colors = np.asarray(colors, np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    if len(colors) != len(verts):
        raise ValueError(f"write_mesh_ply: {len(verts)} vertices but {len(colors)} colours")
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError("write_mesh_ply: a face index is out of range")
    vrec = np.empty(len(verts), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                                       ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    vrec["x"], vrec["y"], vrec["z"] = verts.T
    c8 = np.rint(np.clip(np.nan_to_num(colors), 0.0, 1.0) * 255.0).astype(np.uint8)
    vrec["red"], vrec["green"], vrec["blue"] = c8.T
    frec = np.empty(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = faces
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(verts)}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {len(faces)}\n"
              "property list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def read_mesh_ply(path):
    """Read a binary little-endian triangle-mesh .ply: (verts [nv, 3] float32,
    colors [nv, 3] uint8 or None, faces [nt, 3] int32).  Vertex properties are
    found by name (any order, extra ones skipped); the face element must
    follow the vertex element with one list property (`vertex_indices` or
    `vertex_index`) whose every entry has 3 indices.  Raises ValueError
    otherwise."""
    with open(path, "rb") as f:
        raw = f.read()
    if not raw.startswith(b"ply"):
        raise ValueError(f"{path}: not a PLY file")
    end = raw.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: PLY header has no end_header line")
    offset = end + len(b"end_header\n")
    fmt, elements = None, []          # [name, count, [(prop, dtype) | ("list", name, ct, it)]]
    for line in raw[:end].decode("ascii", errors="replace").split("\n")[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            types = tok[2:4] if tok[1] == "list" else tok[1:2]
            if any(t not in _PLY_TYPES for t in types):
                raise ValueError(f"{path}: unknown property type in {line!r}")
            if tok[1] == "list":
                elements[-1][2].append(("list", tok[4], "<" + _PLY_TYPES[tok[2]],
                                        "<" + _PLY_TYPES[tok[3]]))
            else:
                elements[-1][2].append((tok[2], "<" + _PLY_TYPES[tok[1]]))
    if fmt != "binary_little_endian":
        raise ValueError(f"{path}: only binary_little_endian PLY is read, file is {fmt}")
    names = [e[0] for e in elements]
    if names[:1] != ["vertex"]:
        raise ValueError(f"{path}: the first element must be vertex")
    _, nv, vprops = elements[0]
    if any(p[0] == "list" for p in vprops):
        raise ValueError(f"{path}: list property in the vertex element")
    vdt = np.dtype(vprops)
    for p in ("x", "y", "z"):
        if p not in vdt.names:
            raise ValueError(f"{path}: missing property {p!r}")
    if len(raw) - offset < nv * vdt.itemsize:
        raise ValueError(f"{path}: truncated vertex body")
    vrec = np.frombuffer(raw, dtype=vdt, count=nv, offset=offset)
    offset += nv * vdt.itemsize
    verts = np.stack([vrec[p].astype(np.float32) for p in ("x", "y", "z")], 1).reshape(-1, 3)
    colors = None
    if all(p in vdt.names for p in ("red", "green", "blue")):
        colors = np.stack([vrec[p].astype(np.uint8) for p in ("red", "green", "blue")],
                          1).reshape(-1, 3)
    faces = np.zeros((0, 3), np.int32)
    if len(elements) > 1:
        name, nt, fprops = elements[1]
        if name != "face" or len(fprops) != 1 or fprops[0][0] != "list" \
                or fprops[0][1] not in ("vertex_indices", "vertex_index"):
            raise ValueError(f"{path}: expected a face element with one vertex_indices list")
        fdt = np.dtype([("n", fprops[0][2]), ("v", fprops[0][3], (3,))])
        if len(raw) - offset < nt * fdt.itemsize:
            raise ValueError(f"{path}: truncated face body")
        frec = np.frombuffer(raw, dtype=fdt, count=nt, offset=offset)
        if nt and (frec["n"] != 3).any():
            raise ValueError(f"{path}: only triangles are read")
        faces = np.ascontiguousarray(frec["v"]).astype(np.int32).reshape(-1, 3)
    return verts, colors, faces


def save_mesh(savedir, filename, gmap, T_WC, K, H, W, voxel, **kw):
    """Extract the Gaussian map's surface (SharedGaussians.extract_mesh, which
    takes **kw) and write it as a triangle-mesh .ply into savedir, created
    like save_reconstruction does.  Returns (vertices, triangles) written, or
    None when there is no map, it is empty or there is no view."""
    if gmap is None:
        return None
    mesh = gmap.extract_mesh(T_WC, K, H, W, voxel, **kw)
    if mesh is None:
        return None
    verts, colors, faces = (t.cpu().numpy() for t in mesh)
    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    write_mesh_ply(savedir / filename, verts, colors, faces)
    return len(verts), len(faces)


def save_keyframes(savedir, timestamps, keyframes):
    from PIL import Image
    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    for i in range(len(keyframes)):
        kf = keyframes[i]
        t = timestamps[kf.frame_id]
        Image.fromarray((kf.uimg.cpu().numpy() * 255).astype(np.uint8)).save(savedir / f"{t}.png")


# ------------------------------------------------------- render quality ----
METRIC_NAMES = ("mse", "psnr", "ssim")


def eval_renders(renders, targets, masks=None):
    """Score rendered images against camera images on the device
    (photometric.image_metrics: the reference's log_metrics numbers,
    main.py:249-258).  renders, targets: [N, C, H, W] float32 in [0, 1];
    masks: [N, H, W] or None.  Returns (rows, means): one dict of mse, psnr,
    ssim, l1 per image and the dict of their means over the images."""
    from splatt3r_amd.photometric import image_metrics
    m = {k: v.cpu().tolist() for k, v in image_metrics(renders, targets, masks).items()}
    rows = [{k: m[k][i] for k in m} for i in range(renders.shape[0])]
    means = {k: float(np.mean(v)) if v else float("nan") for k, v in m.items()}
    return rows, means


def save_render_metrics(logdir, logfile, timestamps, rows):
    """One line `t mse psnr ssim` per image and a final `# mean mse psnr ssim`
    line (the means over the lines above)."""
    logdir = pathlib.Path(logdir)
    logdir.mkdir(exist_ok=True, parents=True)
    with open(logdir / logfile, "w") as f:
        for t, r in zip(timestamps, rows):
            f.write(" ".join([str(t)] + [repr(float(r[k])) for k in METRIC_NAMES]) + "\n")
        means = [float(np.mean([r[k] for r in rows])) if rows else float("nan")
                 for k in METRIC_NAMES]
        f.write(" ".join(["# mean"] + [repr(v) for v in means]) + "\n")


def load_render_metrics(path):
    """Reader for the files save_render_metrics writes: (timestamps as
    written, rows, means)."""
    ts, rows, means = [], [], None
    with open(path) as f:
        for line in f:
            p = line.split()
            if p[:2] == ["#", "mean"]:
                means = dict(zip(METRIC_NAMES, map(float, p[2:])))
            else:
                ts.append(p[0])
                rows.append(dict(zip(METRIC_NAMES, map(float, p[1:]))))
    return ts, rows, means


def keyframe_target(kf):
    """A keyframe's camera image as [1, 3, H, W] in [0, 1]: `uimg` ([H, W, 3])
    or, for frames made from an already normalised tensor (which carry no
    uimg), ImgNorm undone on `img`."""
    if kf.uimg is not None:
        return kf.uimg.to(kf.img.device, torch.float32).permute(2, 0, 1)[None]
    return kf.img.to(torch.float32) * 0.5 + 0.5


def eval_keyframe_renders(model, keyframes, K=None):
    """Render every keyframe at its own pose (splatt3r_render(model, kf, kf,
    K=K)) and score it against the keyframe's camera image.  Keyframes without
    Gaussian predictions are skipped and counted.  Returns a dict: `rows`
    (each with the keyframe's `frame_id`), `means`, `skipped`."""
    from splatt3r_amd.splatt3r_utils import splatt3r_render
    ids, renders, targets, skipped = [], [], [], 0
    for i in range(len(keyframes)):
        kf = keyframes[i]
        if kf.gaussian_pred is None or kf.gaussian_pred_cross is None:
            skipped += 1
            continue
        renders.append(splatt3r_render(model, kf, kf, K=K)[0])
        targets.append(keyframe_target(kf))
        ids.append(kf.frame_id)
    rows, means = [], {}
    if renders:
        rows, means = eval_renders(torch.cat(renders).contiguous(), torch.cat(targets).contiguous())
        for fid, r in zip(ids, rows):
            r["frame_id"] = fid
    return dict(rows=rows, means=means, skipped=skipped)


def _own_depth(model, kf, K, alpha_min):
    """A keyframe's rendered depth at its own pose, [1, 1, H, W]: depth / alpha
    (the blend pass returns sum z_i alpha_i T_i) where alpha >= alpha_min,
    else 0, which the loss mask's depth > 1e-6 condition drops."""
    from splatt3r_amd.splatt3r_utils import splatt3r_render
    _, depth, alpha = splatt3r_render(model, kf, kf, K=K, return_depth=True)
    return torch.where(alpha >= alpha_min, depth / alpha, torch.zeros_like(depth)).contiguous()


def eval_novel_view_renders(model, keyframes, K=None, gap=1, alpha_min=0.5):
    """Score every keyframe i against the render of keyframe j = i - gap's
    Gaussians from i's pose (splatt3r_render(model, kf_j, kf_j, K=K,
    target_T_WC=kf_i.T_WC)), over the co-visibility mask the reference takes
    its numbers over (loss_mask.calculate_in_frustum_mask; target view i,
    context view j, depths rendered at each keyframe's own pose, poses the
    4 x 4 (s R | t) of each T_WC, intrinsics the ones the render used).
    Keyframes without Gaussian predictions on either side are skipped and
    counted in `skipped`; pairs with an empty mask in `empty` (the reference
    asserts mask.sum() > 0).  Returns a dict: `rows` (mse, psnr, ssim, l1,
    `frame_id`, `source_id`, `mask_fraction`), `means`, `skipped`, `empty`."""
    from splatt3r_amd.loss_mask import calculate_in_frustum_mask
    from splatt3r_amd.photometric import image_metrics
    from splatt3r_amd.splatt3r_utils import (_estimate_default_intrinsics, _sim3_to_4x4,
                                             splatt3r_render)
    has_pred = lambda kf: kf.gaussian_pred is not None and kf.gaussian_pred_cross is not None
    rows, skipped, empty = [], 0, 0
    for i in range(gap, len(keyframes)):
        kf_i, kf_j = keyframes[i], keyframes[i - gap]
        if not (has_pred(kf_i) and has_pred(kf_j)):
            skipped += 1
            continue
        dev = kf_j.gaussian_pred["means"].device
        _, h, w, _ = kf_j.gaussian_pred["means"].shape
        K_use = (_estimate_default_intrinsics(h, w, dev) if K is None
                 else K.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3, 3)[0])
        K_use = K_use.reshape(1, 1, 3, 3).contiguous()
        render = splatt3r_render(model, kf_j, kf_j, K=K, target_T_WC=kf_i.T_WC)[0].contiguous()
        pose = lambda kf: _sim3_to_4x4(kf.T_WC).to(dev).reshape(1, 1, 4, 4).contiguous()
        mask = calculate_in_frustum_mask(_own_depth(model, kf_i, K, alpha_min), K_use, pose(kf_i),
                                         _own_depth(model, kf_j, K, alpha_min), K_use, pose(kf_j),
                                         as_float=True)[0]
        fraction = float(mask.mean())
        if fraction == 0.0:
            empty += 1
            continue
        m = image_metrics(render, keyframe_target(kf_i).contiguous(), mask)
        row = {k: float(v[0]) for k, v in m.items()}
        row.update(frame_id=kf_i.frame_id, source_id=kf_j.frame_id, mask_fraction=fraction)
        rows.append(row)
    means = {k: float(np.mean([r[k] for r in rows])) for k in ("mse", "psnr", "ssim", "l1")} \
        if rows else {}
    return dict(rows=rows, means=means, skipped=skipped, empty=empty)


# ------------------------------------------- geometry against ground truth ----
def align_umeyama(src, dst, with_scale=True):
    """(s, R, t) minimising sum |dst - (s R src + t)|^2 over similarities
    (Umeyama 1991, with the determinant correction: R is a rotation, never a
    reflection); s = 1 with with_scale=False.  src, dst: [n, 3], numpy
    float64 throughout.  Raises ValueError for fewer than 3 points, mismatched
    shapes, non-finite entries, or points whose cross-covariance has rank
    below 2 (coincident or collinear: the rotation is not determined)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    if src.ndim != 2 or src.shape[1] != 3 or src.shape != dst.shape:
        raise ValueError(f"align_umeyama: need two [n, 3] arrays, got {src.shape} and {dst.shape}")
    n = len(src)
    if n < 3:
        raise ValueError(f"align_umeyama: need at least 3 points, got {n}")
    if not (np.isfinite(src).all() and np.isfinite(dst).all()):
        raise ValueError("align_umeyama: non-finite point")
    mu_s, mu_d = src.mean(0), dst.mean(0)
    xs, xd = src - mu_s, dst - mu_d
    var_s = (xs ** 2).sum() / n
    U, D, Vt = np.linalg.svd(xd.T @ xs / n)
    if not (var_s > 0.0 and D[0] > 0.0 and D[1] > 1e-12 * D[0]):
        raise ValueError("align_umeyama: degenerate points (coincident or collinear)")
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        S[2] = -1.0
    R = (U * S) @ Vt
    s = float((D * S).sum() / var_s) if with_scale else 1.0
    return s, R, mu_d - s * (R @ mu_s)


def read_traj(path):
    """Reader for the TUM-format files save_traj writes (`t x y z qx qy qz qw`
    per line; `#` lines and empty lines skipped): (timestamps [n] float64,
    poses [n, 7] float64)."""
    ts, poses = [], []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            p = line.split()
            if not p or p[0].startswith("#"):
                continue
            if len(p) != 8:
                raise ValueError(f"{path}:{ln}: expected 8 columns, got {len(p)}")
            ts.append(float(p[0]))
            poses.append([float(v) for v in p[1:]])
    return np.asarray(ts, np.float64), np.asarray(poses, np.float64).reshape(-1, 7)


def associate(ts_a, ts_b, max_dt=0.02):
    """One-to-one pairing of two timestamp lists: every pair with
    |a - b| <= max_dt is a candidate, candidates are taken nearest first
    (ties: lower index in a, then in b) and a timestamp is used once.
    Returns (ia, ib) int64 index arrays ordered by ia.  max_dt's default is
    that of the TUM benchmark's associate.py as recalled, not a tuned value."""
    ts_a, ts_b = np.asarray(ts_a, np.float64).reshape(-1), np.asarray(ts_b, np.float64).reshape(-1)
    order = np.argsort(ts_b, kind="stable")
    sb = ts_b[order]
    cand = []
    for i, a in enumerate(ts_a):
        lo, hi = np.searchsorted(sb, a - max_dt, "left"), np.searchsorted(sb, a + max_dt, "right")
        for j in order[lo:hi]:
            d = abs(a - ts_b[j])
            if d <= max_dt:
                cand.append((d, i, int(j)))
    cand.sort()
    used_a, used_b, pairs = set(), set(), []
    for _, i, j in cand:
        if i not in used_a and j not in used_b:
            used_a.add(i)
            used_b.add(j)
            pairs.append((i, j))
    pairs.sort()
    ia = np.asarray([p[0] for p in pairs], np.int64)
    ib = np.asarray([p[1] for p in pairs], np.int64)
    return ia, ib


def _as_traj(x):
    if isinstance(x, (str, pathlib.Path)):
        return read_traj(x)
    ts, poses = x
    poses = np.asarray(poses, np.float64)
    return np.asarray(ts, np.float64).reshape(-1), poses.reshape(len(poses), -1)


def eval_trajectory(est, gt, with_scale=True, max_dt=0.02, align=True):
    """Absolute trajectory error of the positions: est and gt are each a
    TUM-format path or (timestamps [n], poses [n, >= 3]) with the position in
    the first three columns.  Poses are paired by `associate`, est is aligned
    to gt with `align_umeyama` (align=False: compared as given) and the error
    of a pair is |gt - (s R est + t)|.  Returns rmse, mean, median, std
    (population), min, max, n (pairs), scale, R, t: the quantity
    `evo_ape tum gt est -as` reports (-a without scale for with_scale=False);
    evo is not installed here, so parity with it is not pinned."""
    (ts_e, p_e), (ts_g, p_g) = _as_traj(est), _as_traj(gt)
    ia, ib = associate(ts_e, ts_g, max_dt)
    if len(ia) == 0:
        raise ValueError("eval_trajectory: no timestamps within max_dt of each other")
    src, dst = p_e[ia, :3], p_g[ib, :3]
    s, R, t = align_umeyama(src, dst, with_scale) if align else (1.0, np.eye(3), np.zeros(3))
    e = np.sqrt(((dst - (s * (src @ R.T) + t)) ** 2).sum(1))
    return dict(rmse=float(np.sqrt((e ** 2).mean())), mean=float(e.mean()),
                median=float(np.median(e)), std=float(e.std()), min=float(e.min()),
                max=float(e.max()), n=int(len(e)), scale=float(s), R=R, t=t)


def apply_transform(points, transform):
    """s R p + t of points [n, 3] (array or tensor) for transform = (s, R, t):
    each coordinate as s ((R_k0 x + R_k1 y) + R_k2 z) + t_k in numpy float64,
    rounded to float32 once.  Returns a float32 host array."""
    s, R, t = transform
    s, R, t = float(s), np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    p = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    p = p.reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.stack([s * ((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + t[k] for k in range(3)], 1)
    return out.astype(np.float32)


def _is_faces(a) -> bool:
    """a is an integer array or tensor of shape [F, 3] (the second entry of
    a (verts, faces) mesh, as against a list of two points)."""
    if torch.is_tensor(a):
        return a.dim() == 2 and a.shape[1] == 3 and not (a.is_floating_point() or a.is_complex())
    a = np.asarray(a)
    return a.ndim == 2 and a.shape[1] == 3 and a.dtype.kind in "iu"


def _as_cloud(x, samples, seed, device, transform, what):
    """x (an [n, 3] array or tensor, a (verts, faces) mesh or a .ply path) as
    a float32 device tensor [n, 3]: a mesh is sampled (nn.sample_mesh), its
    vertices transformed first."""
    from splatt3r_amd.nn import sample_mesh
    faces = None
    if isinstance(x, (str, pathlib.Path)):
        verts, _, faces = read_mesh_ply(x)
        if len(faces) == 0:
            faces = None
    elif isinstance(x, (tuple, list)) and len(x) == 2 and _is_faces(x[1]):
        verts, faces = x
    else:
        verts = x
    if transform is not None:
        verts = apply_transform(verts, transform)
    to_dev = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(
        np.ascontiguousarray(a))).to(device=device, dtype=dt)
    verts = to_dev(verts, torch.float32)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"eval_reconstruction: {what} must be [n, 3] points, a (verts, faces) "
                         f"mesh or a .ply path, got shape {tuple(verts.shape)}")
    if faces is None:
        return verts.contiguous()
    return sample_mesh(verts, to_dev(faces, torch.int32), samples, seed)[0]


def eval_reconstruction(rec, gt, threshold=0.05, samples=200_000, transform=None, seed=0,
                        max_dist=float("inf"), cell=None, device=None):
    """Score reconstructed geometry against ground truth with exact nearest
    neighbours on the device (splatt3r_amd.nn, include/s3k.h).  rec and gt
    are each an [n, 3] array or tensor, a (verts, faces) mesh, of which
    `samples` area-uniform points are drawn (seed: rec seed, gt seed + 1), or a
    .ply path (read_mesh_ply; points when it has no faces).  transform =
    (s, R, t) takes rec into gt's frame first (apply_transform: float64,
    rounded once; the vertices of a mesh).  Returns
      accuracy    mean distance from rec to the nearest gt point
      completion  mean distance from gt to the nearest rec point
      chamfer     (accuracy + completion) / 2
      precision   share of rec within threshold of gt
      recall      share of gt within threshold of rec (the completion ratio)
      fscore      2 P R / (P + R), 0 when both are 0
      n_rec, n_gt, threshold
    The means are over the points that found a neighbour within max_dist (NaN
    when none did); the shares are over all points.  threshold defaults to
    5 cm, the usual indoor convention; nobody has tuned it here.  One host
    read of ten numbers (and the sampler's check that a mesh has area)."""
    from splatt3r_amd.nn import dist_stats, nearest
    if device is None:
        parts = [t for x in (rec, gt) for t in (x if isinstance(x, (tuple, list)) else (x,))]
        device = next((t.device for t in parts if torch.is_tensor(t) and t.is_cuda),
                      torch.device("cuda"))
    threshold = float(threshold)
    p_rec = _as_cloud(rec, samples, seed, device, transform, "rec")
    p_gt = _as_cloud(gt, samples, seed + 1, device, None, "gt")
    d_rec = nearest(p_rec, p_gt, max_dist, cell=cell)[1]
    d_gt = nearest(p_gt, p_rec, max_dist, cell=cell)[1]
    st = torch.stack([dist_stats(d_rec, threshold), dist_stats(d_gt, threshold)]).cpu().numpy()
    n_rec, n_gt = p_rec.shape[0], p_gt.shape[0]
    mean = lambda s: float(s[1] / s[0]) if s[0] > 0 else float("nan")
    share = lambda s, n: float(s[3] / n) if n > 0 else float("nan")
    acc, comp = mean(st[0]), mean(st[1])
    P, R = share(st[0], n_rec), share(st[1], n_gt)
    return dict(accuracy=acc, completion=comp, chamfer=0.5 * (acc + comp), precision=P, recall=R,
                fscore=2.0 * P * R / (P + R) if P + R > 0 else 0.0, n_rec=n_rec, n_gt=n_gt,
                threshold=threshold)


def save_geometry_metrics(logdir, logfile, metrics):
    """Write the dict eval_reconstruction / Frontend.eval_geometry returns as
    one JSON line (arrays as nested lists)."""
    import json

    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, np.ndarray):
            return v.tolist()
        if isinstance(v, np.generic):
            return v.item()
        return v
    logdir = pathlib.Path(logdir)
    logdir.mkdir(exist_ok=True, parents=True)
    with open(logdir / logfile, "w") as f:
        f.write(json.dumps(plain(metrics)) + "\n")


def load_geometry_metrics(path):
    """Reader for the files save_geometry_metrics writes: the dict, with the
    trajectory's R and t as float64 arrays again."""
    import json
    with open(path) as f:
        m = json.loads(f.readline())
    tr = m.get("trajectory")
    for d in (m, tr) if isinstance(tr, dict) else (m,):
        for k in ("R", "t"):
            if k in d:
                d[k] = np.asarray(d[k], np.float64)
    return m


# ------------------------------------------------------- rendered depth ----
def eval_depth_renders(gmap, T_WC, K, targets, weights=None, align="global", alpha_min=0.5):
    """Score the map's rendered depth against target depth on the device
    (depth.depth_metrics: abs-rel, sq-rel, RMSE, RMSE-log, L1, delta < 1.25^k).
    gmap: a SharedGaussians; T_WC [V, 4, 4] camera-to-world (s R | t);
    targets, weights: [V, H, W] (weights or None), in each view's camera
    units.  align: None, "scale" (one least-squares scale per view) or
    "global" (one for all views; the default, as a monocular map's scale is
    free).  Returns one dict of depth.METRIC_NAMES per view (one host read),
    or None for an empty map."""
    from splatt3r_amd.depth import METRIC_NAMES, depth_metrics
    V, H, W = targets.shape
    out = gmap.render_depth_alpha(T_WC, K, H, W)
    if out is None:
        return None
    f = lambda t: None if t is None else t.to(gmap.device, torch.float32).contiguous()
    m = depth_metrics(out[0], out[1], f(targets), f(weights), align=align, alpha_min=alpha_min)
    host = torch.stack([m[k] for k in METRIC_NAMES]).cpu().tolist()
    return [{k: host[j][i] for j, k in enumerate(METRIC_NAMES)} for i in range(V)]


def save_depth_metrics(logdir, logfile, rows):
    """Write the rows eval_depth_renders / Frontend.eval_depth returns as one
    JSON line (a list of dicts; NaN as JSON's NaN literal)."""
    import json
    logdir = pathlib.Path(logdir)
    logdir.mkdir(exist_ok=True, parents=True)
    with open(logdir / logfile, "w") as f:
        f.write(json.dumps([{k: float(v) for k, v in r.items()} for r in rows]) + "\n")


def load_depth_metrics(path):
    """Reader for the files save_depth_metrics writes: the list of dicts."""
    import json
    with open(path) as f:
        return json.loads(f.readline())
