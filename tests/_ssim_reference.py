"""Dense CPU restatement of the ColorSSIM loss (reference loss.py:197-453), the yardstick of tests/test_color_ssim.py.

It shares no code with the package: both clouds are scattered into a small dense grid, the window sums are a dense
``conv3d`` (missing voxels hold zeros, so they add nothing: the sparse operator's semantics), and the formula is written
out again.  Runs in float64 or float32; the float32 run measures how far float32 arithmetic alone moves the result, which
is what the HIP path is held to.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F


def window_1d(size, sigma=1.5):
    """float32, normalised in float32 (loss.py:229-230)"""
    g = torch.tensor([math.exp(-((i - size // 2) ** 2) / (2.0 * sigma * sigma)) for i in range(size)], dtype=torch.float32)
    return g / g.sum()


def window_3d(size):
    """[size, size, size] float32 by float32 outer products (loss.py:248-251); entry [a, b, c] = g[a] * (g[b] * g[c])"""
    g = window_1d(size)
    plane = g[:, None] * g[None, :]
    return (g[:, None] * plane.reshape(1, -1)).reshape(size, size, size)


def window_sums_dense(grid, window):
    """grid [B, C, X, Y, Z], window [s, s, s] indexed [ix, iy, iz] -> sums over the window centred on every voxel:
    out[b, c, x, y, z] = sum window[ix, iy, iz] * grid[b, c, x + ix - h, y + iy - h, z + iz - h]"""
    B, C = grid.shape[:2]
    s = window.shape[0]
    out = F.conv3d(grid.reshape(B * C, 1, *grid.shape[2:]), window.to(grid.dtype).reshape(1, 1, s, s, s), padding=s // 2)
    return out.reshape(B, C, *grid.shape[2:])


def window_sums_loops(grid, window):
    """the same sums by a plain loop over voxels and offsets (the self-check of window_sums_dense); grid [X, Y, Z] numpy"""
    X, Y, Z = grid.shape
    s = window.shape[0]
    h = s // 2
    out = np.zeros_like(grid)
    for x in range(X):
        for y in range(Y):
            for z in range(Z):
                acc = 0.0
                for ix in range(s):
                    for iy in range(s):
                        for iz in range(s):
                            a, b, c = x + ix - h, y + iy - h, z + iz - h
                            if 0 <= a < X and 0 <= b < Y and 0 <= c < Z:
                                acc += window[ix, iy, iz] * grid[a, b, c]
                out[x, y, z] = acc
    return out


YUV = [[0.2126, 0.7152, 0.00722],             # the reference's matrix, loss.py:270-274 (third entry sic)
       [-0.1146, -0.3854, 0.5],
       [0.5, -0.4542, 0.0458]]


def _to_yuv(rgb):
    m = torch.tensor(YUV, dtype=rgb.dtype)
    out = rgb @ m.t()
    return out + torch.tensor([0.0, 0.5, 0.5], dtype=rgb.dtype)


def ssim_reference(gt_c, gt_f, pr_c, pr_f, q_f, window_size, yuv, dtype, grid):
    """gt_c / pr_c int [n, 4] (b, x, y, z) inside [0, grid)^3, gt_f / pr_f [n, 3], q_f [n_gt, 2] on gt's voxels.
    -> dict(coords = union voxels [U, 4] in (b, x, y, z) order, map [U, 3], loss, grad = d loss / d pr_f), numpy float64"""
    gt_c, pr_c = torch.as_tensor(gt_c).long(), torch.as_tensor(pr_c).long()
    gt_f = torch.as_tensor(gt_f).to(dtype)
    pr_f = torch.as_tensor(pr_f).to(dtype).clone().requires_grad_(True)
    q = torch.as_tensor(q_f).to(dtype)[:, 1]
    B = int(max(gt_c[:, 0].max(), pr_c[:, 0].max())) + 1
    G = grid
    x_col, y_col = gt_f, pr_f
    if yuv:
        x_col, y_col = _to_yuv(gt_f), _to_yuv(pr_f)

    def dense(c, f):
        d = torch.zeros((B, f.shape[1], G, G, G), dtype=dtype)
        return d.index_put((c[:, 0, None], torch.arange(f.shape[1])[None, :], c[:, 1, None], c[:, 2, None], c[:, 3, None]), f)

    ox = dense(gt_c, torch.ones((gt_c.shape[0], 1), dtype=dtype))
    oy = dense(pr_c, torch.ones((pr_c.shape[0], 1), dtype=dtype))
    oxy = ox * oy
    X, Y = dense(gt_c, x_col), dense(pr_c, y_col)
    Xm, Ym = X * oxy, Y * oxy
    maps = torch.cat([ox, oy, oxy, X, Y, X * X, Y * Y, Xm, Ym, Xm * Xm, Ym * Ym, Xm * Ym], dim=1)
    S = window_sums_dense(maps, window_3d(window_size))
    Nx, Ny, Nxy = S[:, 0:1], S[:, 1:2], S[:, 2:3]
    sx, sy, sxx, syy = S[:, 3:6], S[:, 6:9], S[:, 9:12], S[:, 12:15]
    mx, my, mxx, myy, mxy = S[:, 15:18], S[:, 18:21], S[:, 21:24], S[:, 24:27], S[:, 27:30]
    zero = torch.zeros((), dtype=dtype)
    inv = lambda n: torch.where(n > 0, 1 / n, zero)
    pos = lambda v: torch.where(v > 0, v, zero)
    inx, iny, inxy = inv(Nx), inv(Ny), inv(Nxy)
    mu_x, mu_y, mu_xm, mu_ym = inx * sx, iny * sy, inxy * mx, inxy * my
    vx, vy = pos(inx * sxx - mu_x ** 2), pos(iny * syy - mu_y ** 2)
    vxm, vym = pos(inxy * mxx - mu_xm ** 2), pos(inxy * myy - mu_ym ** 2)
    cov = inxy * mxy - mu_xm * mu_ym
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    C3 = C2 / 2
    lum = (2 * mu_x * mu_y + C1) / (mu_x ** 2 + mu_y ** 2 + C1)
    lig = (2 * torch.sqrt(vx) * torch.sqrt(vy) + C2) / (vx + vy + C2)
    stru = (cov + C3) / (torch.sqrt(vxm) * torch.sqrt(vym) + C3)
    qd = dense(gt_c, q[:, None])
    val = (1 - lum * stru * lig) / 2 * qd
    if yuv:
        val = val * torch.tensor([0.75, 0.125, 0.125], dtype=dtype).reshape(1, 3, 1, 1, 1)
    union = torch.nonzero((ox + oy)[:, 0] > 0)                       # (b, x, y, z) ascending
    m = val[union[:, 0], :, union[:, 1], union[:, 2], union[:, 3]]   # [U, 3]
    loss = m.mean()
    (grad,) = torch.autograd.grad(loss, pr_f)
    return {"coords": union.numpy(), "map": m.detach().double().numpy(), "loss": float(loss.detach().double()),
            "grad": grad.double().numpy()}


GRID = 22


def shell_case(seed, batch_index=0):
    """The well-conditioned input: gt = the voxels of a 22^3 grid at distance 6.6 < r < 8.6 from the grid's centre; prediction =
    gt with every voxel of gt's 3^3 dilation flipped with probability 0.08; colours from one uniform field, the prediction's
    with 0.1 N(0, 1) added and clamped; q-map uniform on gt.  -> gt_c, gt_f, pr_c, pr_f, q_f (numpy)"""
    rng = np.random.default_rng(seed)
    ax = np.arange(GRID) - (GRID - 1) / 2.0
    r = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    gt = (r > 6.6) & (r < 8.6)
    pad = np.pad(gt, 1)
    dil = np.zeros_like(gt)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                dil |= pad[dx:dx + GRID, dy:dy + GRID, dz:dz + GRID]
    pred = gt ^ (dil & (rng.random(gt.shape) < 0.08))
    field = rng.random(gt.shape + (3,))
    noisy = np.clip(field + 0.1 * rng.standard_normal(field.shape), 0.0, 1.0)

    def rows(occ):
        c = np.argwhere(occ)
        return np.concatenate([np.full((c.shape[0], 1), batch_index), c], axis=1).astype(np.int32), c

    gt_c, gi = rows(gt)
    pr_c, pi = rows(pred)
    gt_f = field[gi[:, 0], gi[:, 1], gi[:, 2]].astype(np.float32)
    pr_f = noisy[pi[:, 0], pi[:, 1], pi[:, 2]].astype(np.float32)
    q_f = rng.random((gt_c.shape[0], 2)).astype(np.float32)
    return gt_c, gt_f, pr_c, pr_f, q_f


def batched_case(seeds):
    parts = [shell_case(s, b) for b, s in enumerate(seeds)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(5))


@functools.lru_cache(maxsize=None)
def case_and_references(seeds, window_size, yuv):
    """(case, float64 reference, float32 reference, e_s, e_g, e_L) of a seeded case, computed once per session"""
    case = batched_case(seeds)
    r64 = ssim_reference(*case, window_size, yuv, torch.float64, GRID)
    r32 = ssim_reference(*case, window_size, yuv, torch.float32, GRID)
    e_s = np.linalg.norm(r32["map"] - r64["map"]) / np.linalg.norm(r64["map"])
    e_g = np.linalg.norm(r32["grad"] - r64["grad"]) / np.linalg.norm(r64["grad"])
    e_L = abs(r32["loss"] - r64["loss"]) / abs(r64["loss"])
    return case, r64, r32, float(e_s), float(e_g), float(e_L)
