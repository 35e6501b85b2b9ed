"""The training augmentations of the reference (configs/Ours.yaml:29-35; data/transform.py:107-130, 425-494) as device
operators on a collated batch: ``ColorJitter`` (torchvision's transform, all four ranges 0.3) and ``RandomRotate``
(rotate about the block centre, round to the voxel grid, drop duplicate voxels).

Both run in libpcc_hip.so (csrc/augment.hip) for the whole batch at once: the jitter is
three launches, the rotation one coordinate-set construction plus a row gather for the colours.  The random draws stay on
the host (a ``numpy.random.Generator`` per ``TrainAugment``); a few dozen bytes per batch travel to the device.

One deliberate difference from the reference: its ``RandomRotate.transform`` computes ``first_occurrence_indices`` as the
inverse map of a ``unique`` over an inverse map — which is that inverse map again — so it returns N rows gathered from the
first U and removes nothing, although its docstring says "round them to integers, and remove duplicates".  Here the first
occurrence of a voxel wins and later ones are dropped ("Training augmentation").
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .sparse import _host_count, _read_count, _require_cuda, _set_buffers, gather_rows

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3          # operation codes of ``order`` (torchvision's fn_idx)


def rotation_matrices(phi, theta):
    """float32 [B,9]: R_y(theta) @ R_x(phi) per item, row-major (RandomRotate.rotation_matrix_3d, data/transform.py:477-494).
    The sines and cosines are taken in float64 and the closed-form product is rounded to float32 once."""
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    theta = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    if phi.shape != theta.shape or phi.ndim != 1:
        raise ValueError("phi and theta must be vectors of one length")
    cp, sp, ct, st = np.cos(phi), np.sin(phi), np.cos(theta), np.sin(theta)
    zero = np.zeros_like(cp)
    R = np.stack([ct, st * sp, st * cp,
                  zero, cp, -sp,
                  -st, ct * sp, ct * cp], axis=1)
    return np.ascontiguousarray(R, dtype=np.float32)


IDENTITY = np.eye(3, dtype=np.float32).reshape(9)


def _to_device(a, dtype, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)


def random_rotate(C, F, matrices, block_size):
    """(C', F') of a collated device batch (C int32 [n,4], F float32 [n,c]) with item b rotated by matrices[b] (float32 [B,9],
    numpy or tensor) about block_size / 2, rounded to the grid, and only the first row of every (batch, x, y, z) kept
    (pcc_augment_rotate; the arithmetic is specified in include/pcc_hip.h).  F' = F[source row] through pcc_gather_rows.
    Raises ValueError (CoordinateRangeError) when a result is not finite or leaves the coordinate range."""
    C2, src, _ = _rotate(C, matrices, block_size)
    return C2, gather_rows(F.contiguous(), src)


def _rotate(C, matrices, block_size):
    """-> (out_coords [m,4], out_src [m], table of the output set)"""
    _require_cuda(C)
    assert C.dtype == torch.int32 and C.dim() == 2 and C.shape[1] == 4
    C = C.contiguous()
    dev = C.device
    rot = _to_device(matrices, torch.float32, dev).reshape(-1, 9)
    nbatch, n = rot.shape[0], C.shape[0]
    keys, vals, cap, scratch = _set_buffers(n, dev)
    out = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)
    src = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    count, word = _host_count()
    check(_lib.lib().pcc_augment_rotate(ptr(C), n, ptr(rot), nbatch, float(block_size) / 2.0, ptr(keys), ptr(vals), cap, ptr(scratch),
                                        ptr(out), ptr(src), ptr(count), _lib.stream()))
    m = _read_count(word, dev)
    return out[:m], src[:m], (keys, vals, cap)


BATCH_SLOTS = _lib.PCC.BATCH_LIMIT + 1                      # every index the voxel key can hold


def _offsets_of(C, nbatch=None):
    """int64 [nbatch+1] row offsets of the items of a collated batch (rows of one item are contiguous, items ascending), and
    the per-item counts as a host list — ONE transfer from the device: without ``nbatch`` every possible batch index is
    counted (4 KB) and the item count is read off the last one that has rows"""
    slots = BATCH_SLOTS if nbatch is None else int(nbatch)
    counts = torch.empty(slots, dtype=torch.int32, device=C.device)
    check(_lib.lib().pcc_count_per_batch(ptr(C), C.shape[0], slots, ptr(counts), _lib.stream()))
    counts = counts.cpu().numpy()
    if nbatch is None:
        used = np.flatnonzero(counts)
        counts = counts[:int(used[-1]) + 1 if used.size else 0]
    if int(counts.sum()) != C.shape[0]:
        raise ValueError(f"batch indices outside 0..{slots - 1} in a collated batch")
    offsets = np.zeros(counts.shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    return offsets, [int(v) for v in counts]


def _upload(device, *arrays):
    """several small host arrays to the device in ONE copy: -> a tensor view per array (segments 8-byte aligned)"""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    starts, total = [], 0
    for a in arrays:
        starts.append(total)
        total += (a.nbytes + 7) // 8 * 8
    buf = np.zeros(max(total, 8), dtype=np.uint8)
    for a, st in zip(arrays, starts):
        buf[st:st + a.nbytes] = a.reshape(-1).view(np.uint8)
    dbuf = torch.from_numpy(buf).to(device)
    return [dbuf[st:st + a.nbytes].view(torch.from_numpy(a).dtype).reshape(a.shape) for a, st in zip(arrays, starts)]


def _jitter_launch(F, offsets_d, params_d, order_d):
    n, nbatch = F.shape[0], params_d.shape[0]
    out = torch.empty_like(F)
    L = _lib.lib()
    nbytes = L.pcc_color_jitter_scratch_bytes(n, nbatch)
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=F.device)
    check(L.pcc_color_jitter(ptr(F), n, ptr(offsets_d), nbatch, ptr(params_d), ptr(order_d), ptr(out), ptr(scratch), nbytes,
                             _lib.stream()))
    return out


def color_jitter(C, F, params, order, offsets=None):
    """F' (float32 [n,3]) of torchvision's ColorJitter applied per batch item: params float32 [B,4] = (brightness, contrast,
    saturation, hue) factors, order int32 [B,4] = the permutation of (BRIGHTNESS, CONTRAST, SATURATION, HUE) in which item b
    applies them (pcc_color_jitter; formulas in include/pcc_hip.h).  Items are the contiguous runs of C[:, 0]; ``offsets``
    (int64 [B+1], host) may be given when the caller knows them."""
    _require_cuda(F)
    if F.dim() != 2 or F.shape[1] != 3:
        raise ValueError(f"colours of shape {tuple(F.shape)}: need [n, 3]")
    F = F.to(torch.float32).contiguous()
    dev = F.device
    params_h = params.cpu().numpy() if isinstance(params, torch.Tensor) else np.asarray(params)
    order_h = order.cpu().numpy() if isinstance(order, torch.Tensor) else np.asarray(order)
    params_h = np.ascontiguousarray(params_h, dtype=np.float32).reshape(-1, 4)
    order_h = np.ascontiguousarray(order_h, dtype=np.int32).reshape(-1, 4)
    nbatch = params_h.shape[0]
    if order_h.shape[0] != nbatch or not np.array_equal(np.sort(order_h, axis=1), np.tile(np.arange(4, dtype=np.int32), (nbatch, 1))):
        raise ValueError("order must hold one permutation of 0..3 per item")
    n = F.shape[0]
    out = torch.empty_like(F)
    if n == 0 or nbatch == 0:
        return out
    if offsets is None:
        offsets, _ = _offsets_of(C.contiguous(), nbatch)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if offsets.shape != (nbatch + 1,) or offsets[0] != 0 or offsets[-1] != n or np.any(np.diff(offsets) < 0):
        raise ValueError(f"offsets {offsets.tolist()} do not partition {n} rows into {nbatch} items")
    return _jitter_launch(F, *_upload(dev, offsets, params_h, order_h))


class TrainAugment:
    """ColorJitter, then RandomRotate, on a collated device batch: ``(C', F') = aug(C, F)`` — the order of the
    configuration's sorted transform keys (configs/Ours.yaml:29-35).

    Random draws come from a host ``numpy.random.Generator`` seeded with ``seed`` that the object owns.  Per call, for item
    0, 1, ... of the batch in turn, EVERY item draws the same six things in this order, whether or not the gate below lets it
    rotate (so the stream depends on the batch's item count only):

      1. ``rng.permutation(4)``                     the order of (brightness, contrast, saturation, hue)
      2. ``rng.uniform(1 - b, 1 + b)``              brightness factor
      3. ``rng.uniform(1 - c, 1 + c)``              contrast factor
      4. ``rng.uniform(1 - s, 1 + s)``              saturation factor
      5. ``rng.uniform(-h, h)``                     hue shift
      6. ``rng.uniform(0, 2 pi)`` twice             phi (roll), then theta (pitch)

    The same seed and the same sequence of batch shapes therefore give the same output bytes.  The reference's gate is kept:
    an item with at most ``min_rotate_points`` points is not rotated (data/transform.py:470 tests the cube's point count) —
    it gets the identity matrix, under which integer coordinates pass through the rotation's arithmetic unchanged."""

    def __init__(self, block_size=128, seed=0, min_rotate_points=1000, brightness=0.3, contrast=0.3, saturation=0.3, hue=0.3):
        self.block_size = block_size
        self.min_rotate_points = int(min_rotate_points)
        self.ranges = (float(brightness), float(contrast), float(saturation), float(hue))
        self.rng = np.random.default_rng(seed)

    def draw(self, counts):
        """host draws for items of ``counts`` points -> (params float32 [B,4], order int32 [B,4], matrices float32 [B,9])"""
        B = len(counts)
        b, c, s, h = self.ranges
        params = np.empty((B, 4), dtype=np.float32)
        order = np.empty((B, 4), dtype=np.int32)
        phi, theta = np.empty(B), np.empty(B)
        for i in range(B):
            order[i] = self.rng.permutation(4)
            params[i, 0] = self.rng.uniform(1.0 - b, 1.0 + b)
            params[i, 1] = self.rng.uniform(1.0 - c, 1.0 + c)
            params[i, 2] = self.rng.uniform(1.0 - s, 1.0 + s)
            params[i, 3] = self.rng.uniform(-h, h)
            phi[i] = self.rng.uniform(0.0, 2.0 * math.pi)
            theta[i] = self.rng.uniform(0.0, 2.0 * math.pi)
        matrices = rotation_matrices(phi, theta) if B else np.empty((0, 9), dtype=np.float32)
        for i, cnt in enumerate(counts):
            if cnt <= self.min_rotate_points:
                matrices[i] = IDENTITY
        return params, order, matrices

    def __call__(self, C, F):
        """One read from the device (the per-item counts, which the gate needs on the host, and with them the item count), one
        copy to it (offsets, factors, orders and matrices together), and the rotation's row count."""
        _require_cuda(C)
        C = C.contiguous()
        if C.shape[0] == 0:
            return C, F
        if F.dim() != 2 or F.shape[1] != 3:
            raise ValueError(f"colours of shape {tuple(F.shape)}: need [n, 3]")
        offsets, counts = _offsets_of(C)
        params, order, matrices = self.draw(counts)
        offsets_d, params_d, order_d, matrices_d = _upload(C.device, offsets, params, order, matrices)
        F = _jitter_launch(F.to(torch.float32).contiguous(), offsets_d, params_d, order_d)
        return random_rotate(C, F, matrices_d, self.block_size)
