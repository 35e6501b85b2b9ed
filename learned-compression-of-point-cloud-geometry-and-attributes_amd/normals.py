"""Surface normals of a voxelised point cloud on the GPU (csrc/normals.hip).

Replaces open3d's ``estimate_normals`` (evaluate_view_dep.py:354-376).  The neighbourhood of a point is every
occupied voxel within ``radius`` voxels (Euclidean, the point itself included), found through the cloud's hashed-voxel table; the
normal is the unit eigenvector of the smallest eigenvalue of the neighbourhood's covariance, whose integer moments are exact.
Points with fewer than 3 neighbours, or whose neighbours all lie on one line, have no normal: (0, 0, 0).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .sparse import CoordMap

ORIENT_NONE, ORIENT_DIRECTION, ORIENT_CAMERA = 0, 1, 2


def _as_coords(cloud, device):
    """[N, 3+] voxelised cloud -> int32 [N, 4] coordinates of batch item 0 (the integer check of metrics._as_cloud)"""
    if not torch.is_tensor(cloud):
        cloud = torch.as_tensor(np.asarray(cloud))
    if cloud.dim() != 2 or cloud.shape[1] < 3:
        raise ValueError("a cloud is a [N, 3+] array: x, y, z first")
    xyz = cloud[:, :3].to(device)
    ixyz = torch.round(xyz.double()).to(torch.int32)
    if not torch.equal(ixyz.to(xyz.dtype), xyz):
        raise ValueError("normals run on voxelised clouds: coordinates must be integers")
    return torch.cat([torch.zeros((xyz.shape[0], 1), dtype=torch.int32, device=device), ixyz], dim=1).contiguous()


def estimate_normals(cloud, radius=3, direction=None, camera=None, coord_map=None, return_moments=False):
    """-> (normals float64 [N, 3], count int32 [N]) and, with ``return_moments``, moments int64 [N, 6].

    ``cloud``: an [N, 3+] voxelised cloud (tensor or array; a tensor on a GPU stays on it), or — with ``coord_map`` — the int32
    [N, 4] coordinate tensor (batch, x, y, z) that the map was built on.  ``radius``: 1 .. 8 voxels.  ``direction``: normals are
    flipped to n . direction >= 0; ``camera``: to n . (camera - p) >= 0, towards a camera position; neither: the sign is
    deterministic but unspecified.  ``count``: the number of neighbours of each point; ``moments``: the upper triangle (xx, xy, xz,
    yy, yz, zz) of count * sum(d d^T) - sum(d) sum(d)^T over the neighbour offsets d — count^2 times the covariance."""
    if direction is not None and camera is not None:
        raise ValueError("estimate_normals: give a direction or a camera position, not both")
    if coord_map is None:
        device = cloud.device if torch.is_tensor(cloud) and cloud.is_cuda else "cuda:0"
        coords = _as_coords(cloud, device)
        coord_map = CoordMap(coords, 1, nbatch=1)
    else:
        coords = cloud
        if not (torch.is_tensor(coords) and coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 4):
            raise ValueError("estimate_normals: with a coord_map the cloud is its int32 [N, 4] coordinate tensor")
        if coords.device != coord_map.device:
            raise ValueError("estimate_normals: coordinates and coord_map are on different devices")
        coords = coords.contiguous()
    mode, vec = ORIENT_NONE, None
    if direction is not None:
        mode, vec = ORIENT_DIRECTION, direction
    elif camera is not None:
        mode, vec = ORIENT_CAMERA, camera
    orient = None
    if vec is not None:
        vec = [float(v) for v in (vec.tolist() if hasattr(vec, "tolist") else vec)]
        if len(vec) != 3:
            raise ValueError("estimate_normals: direction / camera are 3 numbers")
        orient = (ctypes.c_double * 3)(*vec)
    n, dev = int(coords.shape[0]), coords.device
    normals = torch.empty((n, 3), dtype=torch.float64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    moments = torch.empty((n, 6), dtype=torch.int64, device=dev) if return_moments else None
    with torch.cuda.device(dev):
        keys, vals, cap = coord_map.table()
        check(_lib.lib().pcc_estimate_normals(ptr(coords), n, ptr(keys), ptr(vals), cap, coord_map.stride, int(radius), mode,
                                              None if orient is None else ctypes.addressof(orient), ptr(normals), ptr(count), ptr(moments),
                                              _lib.stream()))
    return (normals, count, moments) if return_moments else (normals, count)
