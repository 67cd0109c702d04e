"""Co-visibility loss mask on the device (include/s3c.h): the target-view
pixels whose 3-D point lands inside some context view's frustum, has valid
depth, and agrees with a context view's depth there to 0.1.

The reference computes it in splatt3r_core/utils/loss_mask.py and never calls
calculate_loss without it (main.py training_step, validation_step, test_step);
every number it reports is taken over this mask.  Here one HIP launch does the
whole projection / sampling chain per target pixel (csrc/loss_mask.hip), after
a tiny launch that inverts the intrinsics and poses in double; both are
stream-ordered, with no host sync and no solver library.

The result feeds photometric.photometric_loss / image_metrics / ssim /
calculate_loss and evaluate.eval_renders, which take float32 masks:
`as_float=True` returns that directly, with no cast launch.

Importing this module does not initialise the GPU; arguments are validated
before it is required.
"""
from __future__ import annotations

import torch

from splatt3r_amd import _abi, _lib

COND_FRUSTUM, COND_DEPTH, COND_MATCH = (
    _abi.constants[k] for k in ("S3C_COND_FRUSTUM", "S3C_COND_DEPTH", "S3C_COND_MATCH"))


def _check(depth_1, intrinsics_1, c2w_1, depth_2, intrinsics_2, c2w_2, fn):
    named = (("depth_1", depth_1), ("intrinsics_1", intrinsics_1), ("c2w_1", c2w_1),
             ("depth_2", depth_2), ("intrinsics_2", intrinsics_2), ("c2w_2", c2w_2))
    for name, t in named:
        if not torch.is_tensor(t):
            raise TypeError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{fn}: {name} must be float32, got {t.dtype}")
    if depth_1.dim() != 4:
        raise ValueError(f"{fn}: depth_1 must be [b, v1, h, w], got {tuple(depth_1.shape)}")
    b, v1, h, w = depth_1.shape
    if depth_2.dim() != 4 or depth_2.shape[0] != b or tuple(depth_2.shape[2:]) != (h, w):
        raise ValueError(f"{fn}: depth_2 must be [b, v2, h, w] = [{b}, v2, {h}, {w}], "
                         f"got {tuple(depth_2.shape)}")
    v2 = depth_2.shape[1]
    if min(b, v1, v2, h, w) < 1:
        raise ValueError(f"{fn}: depth_1 {tuple(depth_1.shape)} / depth_2 {tuple(depth_2.shape)} "
                         "have an empty dimension")
    for name, t, want in (("intrinsics_1", intrinsics_1, (b, v1, 3, 3)),
                          ("c2w_1", c2w_1, (b, v1, 4, 4)),
                          ("intrinsics_2", intrinsics_2, (b, v2, 3, 3)),
                          ("c2w_2", c2w_2, (b, v2, 4, 4))):
        if tuple(t.shape) != want:
            raise ValueError(f"{fn}: {name} must be {list(want)}, got {tuple(t.shape)}")
    tensors = [t for _, t in named]
    _lib.require_cuda(*tensors)
    for name, t in named[1:]:
        if t.device != depth_1.device:
            raise RuntimeError(f"{fn}: {name} is on {t.device}, depth_1 on {depth_1.device}; "
                               "all arguments must be on one device")
    return b, v1, v2, h, w


@torch.no_grad()
def calculate_in_frustum_mask(depth_1, intrinsics_1, c2w_1, depth_2, intrinsics_2, c2w_2, *,
                              as_float=False, return_conditions=False):
    """utils/loss_mask.py calculate_in_frustum_mask: which pixels of the first
    set of views have a directly corresponding pixel in any view of the second.

    depth_1 [b, v1, h, w], intrinsics_1 [b, v1, 3, 3], c2w_1 [b, v1, 4, 4];
    depth_2 [b, v2, h, w], intrinsics_2 [b, v2, 3, 3], c2w_2 [b, v2, 4, 4]; all
    float32 on one GPU.  Returns the mask [b, v1, h, w] as torch.bool, or with
    as_float as float32 0 / 1; with return_conditions also the uint8 map of
    COND_FRUSTUM (in some context view's frustum), COND_DEPTH (depth > 1e-6)
    and COND_MATCH (depth agrees with some context view's), whose AND the mask
    is.  The two `any` over the context views are separate, and there is no
    z > 0 test: both as in the reference (include/s3c.h)."""
    fn = "calculate_in_frustum_mask"
    b, v1, v2, h, w = _check(depth_1, intrinsics_1, c2w_1, depth_2, intrinsics_2, c2w_2, fn)
    dev = depth_1.device
    args = [t.detach().contiguous() for t in (depth_1, intrinsics_1, c2w_1, depth_2, intrinsics_2,
                                              c2w_2)]
    L = _lib.lib()
    with torch.cuda.device(dev):
        mask = torch.empty((b, v1, h, w), dtype=torch.bool, device=dev)
        mask_f = torch.empty((b, v1, h, w), dtype=torch.float32, device=dev) if as_float else None
        cond = torch.empty((b, v1, h, w), dtype=torch.uint8, device=dev) if return_conditions \
            else None
        ws = torch.empty(L.s3c_loss_mask_workspace_bytes(b, v1, v2), dtype=torch.uint8, device=dev)
        _lib.call("s3c_loss_mask", *[t.data_ptr() for t in args], b, v1, v2, h, w,
                  mask.data_ptr(), _lib.ptr(mask_f), _lib.ptr(cond), ws.data_ptr(),
                  _lib.stream(dev))
    out = mask_f if as_float else mask
    return (out, cond) if return_conditions else out


@torch.no_grad()
def calculate_loss_mask(batch, **kwargs):
    """utils/loss_mask.py calculate_loss_mask: the loss mask of the target
    views of a batch dict, batch['target' | 'context'][k]['depthmap' |
    'camera_intrinsics' | 'camera_pose'] ([b, h, w], [b, 3.., 3..], [b, 4, 4]);
    the views are stacked on dim 1 and the intrinsics cut to [..., :3, :3].
    Keyword arguments go to calculate_in_frustum_mask."""
    def stack(side, key):
        return torch.stack([view[key] for view in batch[side]], dim=1)
    return calculate_in_frustum_mask(
        stack("target", "depthmap"), stack("target", "camera_intrinsics")[..., :3, :3],
        stack("target", "camera_pose"),
        stack("context", "depthmap"), stack("context", "camera_intrinsics")[..., :3, :3],
        stack("context", "camera_pose"), **kwargs)
