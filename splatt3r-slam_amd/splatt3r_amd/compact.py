"""Map compaction (include/s3v.h): Gaussians whose centres fall in the same
voxel are replaced by their moment-matched merge, deterministically, in one
stream-ordered HIP pass (csrc/map_compact.hip: voxel keys, a stable 64-bit
radix sort, a segmented double-precision reduction).

  merge_gaussians   the pass on five field tensors, out of place
  SharedGaussians.compact (gaussian_map.py) runs it on the map in place

The reference has no counterpart: its map evicts its oldest half when full.
The voxel size is the caller's and nobody has tuned it.

Importing this module does not initialise the GPU.
"""
from __future__ import annotations

import ctypes
import math

import torch

from splatt3r_amd import _abi, _lib

S3vIn = _abi.structs["s3v_in"]      # include/s3v.h
S3vOut = _abi.structs["s3v_out"]


def check_grid(voxel, origin, fn: str):
    """(voxel, origin) as a float and a 3-tuple of floats; ValueError unless
    voxel > 0 and all four are finite."""
    voxel = float(voxel)
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError(f"{fn}: voxel must be > 0 and finite, got {voxel}")
    origin = tuple(float(v) for v in origin)
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
        raise ValueError(f"{fn}: origin must be three finite numbers, got {origin}")
    return voxel, origin


def launch_merge(fields, n_dev, n_max, voxel, origin, outs, first, group, tally, ws):
    """s3v_merge on already-checked device tensors.  fields, outs: the five
    tensors each; n_dev: device int64 [1] or None; tally: device int64 [2],
    (m, dropped)."""
    dev = fields[0].device
    c_in = S3vIn(*[t.data_ptr() for t in fields])
    c_out = S3vOut(*[t.data_ptr() for t in outs])
    org = (ctypes.c_double * 3)(*origin)
    with torch.cuda.device(dev):
        _lib.call("s3v_merge", ctypes.byref(c_in), None if n_dev is None else n_dev.data_ptr(),
                  int(n_max), org, voxel, ctypes.byref(c_out), first.data_ptr(),
                  group.data_ptr(), tally.data_ptr(), tally.data_ptr() + 8, ws.data_ptr(),
                  ws.numel(), _lib.stream(dev))


def workspace(n_max: int, device) -> torch.Tensor:
    """A uint8 device tensor of s3v_merge_workspace_bytes(n_max) bytes."""
    need = int(_lib.lib().s3v_merge_workspace_bytes(int(n_max)))
    return torch.empty(need, device=device, dtype=torch.uint8)


@torch.no_grad()
def merge_gaussians(means, cov_triu, colors, opacities, kf_id, voxel, origin=(0.0, 0.0, 0.0),
                    n=None):
    """Merge the Gaussians of every voxel of side `voxel` on the grid through
    `origin` (include/s3v.h states the definition in full): means [n_max, 3],
    cov_triu [n_max, 6], colors [n_max, 3], opacities [n_max] float32 and
    kf_id [n_max] int32 device tensors; n: a device int64 tensor of one entry,
    the number of leading rows that count (None: all).

    Returns (means, cov_triu, colors, opacities, kf_id, first, group, m,
    dropped): new device tensors sized to the input, of which the first m rows
    hold the merged Gaussians ordered by `first` (int64, the lowest input index
    of each group); group [n_max] int64 is the output row each input row went
    to, -1 for a row dropped because a field was not finite (entries at and
    past n are -1 too); m and dropped are device int64 scalars.  Nothing is
    read back to the host.  Bit-reproducible, and idempotent: merging the
    result again with the same voxel and origin returns it bit for bit."""
    fn = "merge_gaussians"
    voxel, origin = check_grid(voxel, origin, fn)
    if not torch.is_tensor(means) or means.dim() != 2 or means.shape[1] != 3:
        raise ValueError(f"{fn}: means must be [n, 3]")
    n_max = means.shape[0]
    want = ((means, (n_max, 3), torch.float32, "means"),
            (cov_triu, (n_max, 6), torch.float32, "cov_triu"),
            (colors, (n_max, 3), torch.float32, "colors"),
            (opacities, (n_max,), torch.float32, "opacities"),
            (kf_id, (n_max,), torch.int32, "kf_id"))
    for t, shape, dt, name in want:
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt:
            raise ValueError(f"{fn}: {name} must be a {dt} tensor of shape {list(shape)}")
    if n is not None and (not torch.is_tensor(n) or n.dtype != torch.int64 or n.numel() != 1):
        raise ValueError(f"{fn}: n must be an int64 tensor of one entry")
    fields = (means, cov_triu, colors, opacities, kf_id)
    _lib.require_cuda(*fields, n)
    dev = means.device
    fields = tuple(t.contiguous() for t in fields)
    outs = tuple(torch.empty_like(t) for t in fields)
    first = torch.empty(n_max, device=dev, dtype=torch.int64)
    group = torch.full((n_max,), -1, device=dev, dtype=torch.int64)
    tally = torch.zeros(2, device=dev, dtype=torch.int64)
    if n_max == 0:
        return (*outs, first, group, tally[0], tally[1])
    launch_merge(fields, n, n_max, voxel, origin, outs, first, group, tally,
                 workspace(n_max, dev))
    return (*outs, first, group, tally[0], tally[1])
