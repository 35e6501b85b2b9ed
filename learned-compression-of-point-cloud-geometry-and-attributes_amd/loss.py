"""Training losses (mirror of /root/reference/loss.py:7-453: ``Loss``, ``BPPLoss``, ``ColorLoss``,
``FocalLoss``, ``Multiscale_FocalLoss``, ``ColorSSIM``), on this package's SparseTensor.

Elementwise arithmetic on per-point vectors is plain torch (autograd); the sparse pieces run on the
HIP coordinate kernels: the reference's ``torch.isin`` on packed coordinates becomes a voxel-hash
lookup, ``MinkowskiAvgPooling`` (loss.py:154-155) an average over the kernel map's existing neighbours,
the ``MinkowskiChannelwiseConvolution`` of ColorSSIM (loss.py:204-206) the HIP window convolution of
csrc/chconv.hip — the SSIM formula itself stays torch, in the reference's operation order.
"""
import functools
import math

import torch
import torch.nn.functional as F

from .sparse import CoordMap, MinkowskiChannelwiseConvolution, SparseTensor, gather_rows


def avg_pool(x, out_map, kernel_size=3):
    """ME.MinkowskiAvgPooling(kernel_size, stride = out stride / in stride): mean of the inputs that exist
    in the kernel window of every output voxel (zero where there is none)."""
    nbr, _, _ = x.map.kernel_map(out_map, kernel_size)
    valid = nbr >= 0
    sel = x.F.index_select(0, nbr.clamp(min=0).reshape(-1).long()).reshape(nbr.shape[0], nbr.shape[1], -1)
    sel = sel * valid.unsqueeze(2).to(sel.dtype)
    cnt = valid.sum(dim=1, keepdim=True).clamp(min=1).to(sel.dtype)
    return SparseTensor(sel.sum(dim=1) / cnt, coordinate_map=out_map)


class BPPLoss:
    def __init__(self, config):
        self.weight = config["weight"]
        self.identifier = config["id"]
        self.key = config["key"]

    def __call__(self, gt, pred):
        loss = 0.0
        num_points = gt.C.shape[0]
        for likelihood in pred["likelihoods"][self.key]:
            loss = loss + torch.log(likelihood).sum() / (-math.log(2) * num_points)
        return loss.mean() * self.weight


class ColorLoss:
    def __init__(self, config):
        self.identifier = config["id"]
        self.loss_func = torch.nn.L1Loss(reduction="none") if config["loss"] == "L1" else torch.nn.MSELoss(reduction="none")

    def __call__(self, gt, pred):
        pred_colors = pred["prediction"].features_at_coordinates(gt.C.float())
        color_loss = self.loss_func(gt.F, pred_colors)
        color_loss = color_loss * pred["q_map"].features_at_coordinates(gt.C.float())[:, 1].unsqueeze(1)
        return color_loss.mean()


def _focal(logits, overlapping, alpha, gamma):
    p_z = torch.sigmoid(logits)
    pt_z = torch.where(overlapping, p_z, 1 - p_z)
    alpha_z = torch.where(overlapping, torch.full_like(p_z, alpha), torch.full_like(p_z, 1 - alpha))
    pt_z = torch.clip(pt_z, 1e-2, 1)
    return -alpha_z * (1 - pt_z) ** gamma * torch.log(pt_z)


class FocalLoss:
    def __init__(self, config):
        self.identifier = config["id"]
        self.alpha, self.gamma = config["alpha"], config["gamma"]

    def __call__(self, gt, pred):
        prediction = pred["prediction"]
        overlapping = gt.map.lookup(prediction.C) >= 0
        return _focal(prediction.F[:, 0] + 0.5, overlapping, self.alpha, self.gamma).mean() * pred["lambdas"][0][0]


class Multiscale_FocalLoss:
    def __init__(self, config):
        self.identifier = config["id"]
        self.alpha, self.gamma = config["alpha"], config["gamma"]

    def __call__(self, gt, pred):
        predictions = list(reversed(pred["occ_predictions"]))      # finest scale first (loss.py:160-161)
        points = list(reversed(pred["points"]))
        q_map = pred["q_map"]
        loss = 0.0
        for prediction, coords in zip(predictions, points):
            overlapping = coords.map.lookup(prediction.C) >= 0
            focal = _focal(prediction.F[:, 0], overlapping, self.alpha, self.gamma)
            q_avgs = avg_pool(q_map, prediction.map, 3)             # pooled onto the candidates
            q_map = avg_pool(q_map, q_map.map.down(), 3)            # next scale
            loss = loss + (focal * q_avgs.F[:, 0]).mean()
        return loss


def gaussian_window_3d(window_size, sigma=1.5):
    """loss.py:213-253: the 1-D Gaussian normalised in float32, then outer products in float32 -> [window_size^3, 1]"""
    gauss = torch.tensor([math.exp(-(i - window_size // 2) ** 2 / float(2 * sigma ** 2)) for i in range(window_size)],
                         dtype=torch.float32)
    w1 = (gauss / gauss.sum()).unsqueeze(1)                              # [w, 1]
    w2 = w1.mm(w1.t())                                                   # [w, w]
    w3 = w1.mm(w2.reshape(1, -1))                                        # [w, w * w]
    return w3.reshape(-1, 1).float().contiguous()


def rgb_to_yuv(rgb):
    """loss.py:255-283 as written ("BT.709").  The Y row's third coefficient 0.00722 is the reference's value (BT.709's is
    0.0722): kept, because the loss a reference config trains with is this one."""
    m = torch.tensor([[0.2126, 0.7152, 0.00722],
                      [-0.1146, -0.3854, 0.5],
                      [0.5, -0.4542, 0.0458]], dtype=rgb.dtype, device=rgb.device)
    yuv = torch.einsum("ij,nj->ni", m, rgb)
    return yuv + torch.tensor([0.0, 0.5, 0.5], dtype=rgb.dtype, device=rgb.device)


@functools.lru_cache(maxsize=16)
def _window_sum(window_size, device):
    """loss.py:204-206: the channelwise convolution with the Gaussian window as its frozen [K, 1] kernel"""
    conv = MinkowskiChannelwiseConvolution(in_channels=30, kernel_size=window_size, stride=1, dimension=3)
    conv.kernel = torch.nn.Parameter(gaussian_window_3d(window_size).to(device), requires_grad=False)
    return conv


def _union_map(a, b, stride=1):
    """loss.py:308: the union of two coordinate lists as one CoordMap (rows in packed-key order)"""
    c = torch.cat([a, b], 0).long()
    key = (c[:, 0] << 54) | ((c[:, 1] + (1 << 17)) << 36) | ((c[:, 2] + (1 << 17)) << 18) | (c[:, 3] + (1 << 17))
    u = torch.unique(key)
    m18 = (1 << 18) - 1
    coords = torch.stack([(u >> 54) & 0x3FF, ((u >> 36) & m18) - (1 << 17), ((u >> 18) & m18) - (1 << 17), (u & m18) - (1 << 17)], 1)
    return CoordMap(coords.to(torch.int32).contiguous(), stride)


def color_ssim_map(gt, prediction, q_map, window_size, yuv):
    """The per-voxel ColorSSIM term on the union of ground-truth and predicted voxels (loss.py:285-363, 391-453) ->
    (union coordinates [U, 4], ssim [U, 3]); ``ColorSSIM`` is its mean.  Differentiable with respect to ``prediction.F``."""
    C1, C2 = 0.01 ** 2, 0.03 ** 2                                        # loss.py:208-210
    C3 = C2 / 2
    gt_f, pred_f = gt.F, prediction.F
    if yuv:                                                              # loss.py:295-297
        gt_f, pred_f = rgb_to_yuv(gt_f), rgb_to_yuv(pred_f)
    union = _union_map(gt.C, prediction.C, gt.map.stride)              # loss.py:308
    U = union.coords

    # loss.py:396-413: occupancies and colours on the union (absent = 0), masked to the intersection
    gt_idx, pred_idx = gt.map.lookup(U), prediction.map.lookup(U)
    gt_occ = (gt_idx >= 0).to(torch.float32).unsqueeze(1)
    pred_occ = (pred_idx >= 0).to(torch.float32).unsqueeze(1)
    shared_occ = pred_occ * gt_occ
    pred_u = gather_rows(pred_f, pred_idx) * pred_occ
    gt_u = gather_rows(gt_f, gt_idx) * gt_occ
    pred_m = pred_u * shared_occ
    gt_m = gt_u * shared_occ
    pred_gt_m = pred_m * gt_m

    # loss.py:416-437: the 30 maps (two zero columns keep a row one 128-byte line), one window sum for all of them
    feats = torch.cat([gt_occ, pred_occ, shared_occ,                     # 0 1 2
                       gt_u, pred_u, gt_u.pow(2), pred_u.pow(2),         # 3:6 6:9 9:12 12:15
                       gt_m, pred_m, gt_m.pow(2), pred_m.pow(2),         # 15:18 18:21 21:24 24:27
                       pred_gt_m,                                        # 27:30
                       torch.zeros((U.shape[0], 2), dtype=torch.float32, device=U.device)], dim=1)
    R = _window_sum(int(window_size), U.device)(SparseTensor(feats, coordinate_map=union)).F
    N_x, N_y, N_xy = R[:, 0:1], R[:, 1:2], R[:, 2:3]                     # loss.py:439-452
    sum_x, sum_y, sum_x_sq, sum_y_sq = R[:, 3:6], R[:, 6:9], R[:, 9:12], R[:, 12:15]
    m_sum_x, m_sum_y, m_sum_x_sq, m_sum_y_sq, m_sum_xy = R[:, 15:18], R[:, 18:21], R[:, 21:24], R[:, 24:27], R[:, 27:30]

    # loss.py:313-315
    N_x_inv = torch.where(N_x > 0.0, 1 / N_x, 0)
    N_y_inv = torch.where(N_y > 0.0, 1 / N_y, 0)
    N_xy_inv = torch.where(N_xy > 0.0, 1 / N_xy, 0)
    # loss.py:322-325
    mu_x = N_x_inv * sum_x
    mu_y = N_y_inv * sum_y
    mu_x_masked = N_xy_inv * m_sum_x
    mu_y_masked = N_xy_inv * m_sum_y
    # loss.py:332-341
    sigma_x_sq = N_x_inv * sum_x_sq - mu_x.pow(2)
    sigma_y_sq = N_y_inv * sum_y_sq - mu_y.pow(2)
    sigma_x_sq_masked = N_xy_inv * m_sum_x_sq - mu_x_masked.pow(2)
    sigma_y_sq_masked = N_xy_inv * m_sum_y_sq - mu_y_masked.pow(2)
    sigma_x_sq = torch.where(sigma_x_sq > 0.0, sigma_x_sq, 0)
    sigma_y_sq = torch.where(sigma_y_sq > 0.0, sigma_y_sq, 0)
    sigma_x_sq_masked = torch.where(sigma_x_sq_masked > 0.0, sigma_x_sq_masked, 0)
    sigma_y_sq_masked = torch.where(sigma_y_sq_masked > 0.0, sigma_y_sq_masked, 0)
    # loss.py:343-350
    sigma_x = torch.sqrt(sigma_x_sq)
    sigma_y = torch.sqrt(sigma_y_sq)
    sigma_x_masked = torch.sqrt(sigma_x_sq_masked)
    sigma_y_masked = torch.sqrt(sigma_y_sq_masked)
    sigma_xy = N_xy_inv * m_sum_xy - mu_x_masked * mu_y_masked
    # loss.py:353-358
    luminance = (2 * mu_x * mu_y + C1) / (mu_x.pow(2) + mu_y.pow(2) + C1)
    lightness = (2 * sigma_x * sigma_y + C2) / (sigma_x_sq + sigma_y_sq + C2)
    structure = (sigma_xy + C3) / (sigma_x_masked * sigma_y_masked + C3)
    ssim = luminance * structure * lightness
    # loss.py:359-361
    ssim = ((1 - ssim) / 2) * q_map.features_at_coordinates(U)[:, 1].unsqueeze(1)
    if yuv:
        ssim = ssim * torch.tensor([[0.75, 0.125, 0.125]], dtype=ssim.dtype, device=ssim.device)
    return U, ssim


class ColorSSIM:
    """loss.py:197-363: mean over the union voxels and the three channels of (1 - SSIM) / 2, weighted by the q-map"""

    def __init__(self, config):
        self.identifier = config["id"]
        self.window_size = config["window_size"]
        self.yuv = config["yuv"]

    def __call__(self, gt, pred):
        return color_ssim_map(gt, pred["prediction"], pred["q_map"], self.window_size, self.yuv)[1].mean()


class Loss:
    """loss.py:7-64: sum of the configured losses -> (total, {id: value})."""
    TYPES = {"BPPLoss": BPPLoss, "ColorLoss": ColorLoss, "FocalLoss": FocalLoss, "Multiscale_FocalLoss": Multiscale_FocalLoss,
             "ColorSSIM": ColorSSIM}

    def __init__(self, config):
        self.losses = {}
        for ident, setting in config.items():
            setting = dict(setting, id=ident)
            cls = self.TYPES.get(setting["type"])
            if cls is None:
                print("Not found {}".format(setting["type"]))
                continue
            self.losses[ident] = cls(setting)

    def __call__(self, gt, pred):
        total, parts = 0, {}
        for loss in self.losses.values():
            item = loss(gt, pred)
            parts[loss.identifier] = item
            total = total + item
        return total, parts


OURS_LOSS = {            # configs/Ours.yaml:58-73
    "Multiscale_FocalLoss": {"type": "Multiscale_FocalLoss", "alpha": 0.5, "gamma": 2.0},
    "ColorLoss": {"type": "ColorLoss", "loss": "L2"},
    "bpp-y": {"type": "BPPLoss", "key": "y", "weight": 1.0},
    "bpp-z": {"type": "BPPLoss", "key": "z", "weight": 1.0},
}
