"""The ColorSSIM loss (pcc_amd.loss.ColorSSIM / color_ssim_map, reference loss.py:197-453) against the dense float64
restatement of tests/_ssim_reference.py.

The yardstick is the restatement's OWN float32 error (e_s on the per-voxel map, e_g on the gradient with respect to the
predicted colours, e_L on the loss), never the code under test: the HIP path must lie within 4 e + 1e-6 of float64.  The
inputs are chosen where the formula is well conditioned (a thick shell with 8 % flipped voxels), and that is asserted:
e_s <= 1e-4, e_g <= 1e-5.  Scattered clouds are NOT held to a tolerance: at isolated voxels a variance is cancellation noise
that sqrt amplifies (loss.py:332-346), and the restatement's own float32 gradient is then off by percents.
"""
import numpy as np
import pytest
import torch

import _ssim_reference as ref

DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------
# no GPU needed
# ---------------------------------------------------------------------------------------------
def test_dispatcher_knows_color_ssim(pcc):
    from pcc_amd.loss import ColorSSIM, Loss
    losses = Loss({"ssim": {"type": "ColorSSIM", "window_size": 5, "yuv": False}}).losses
    assert list(losses) == ["ssim"] and isinstance(losses["ssim"], ColorSSIM)
    assert losses["ssim"].identifier == "ssim" and losses["ssim"].window_size == 5 and losses["ssim"].yuv is False


def test_library_exports_the_window_convolution(pcc):
    from pcc_amd import _lib
    assert hasattr(pcc.lib(), "pcc_chconv") and "pcc_chconv" in _lib.SIGNATURES
    assert pcc.MinkowskiChannelwiseConvolution is not None


def test_reference_window_sums_check_themselves():
    """conv3d window sums of the restatement against a plain loop over voxels and offsets, 12^3, float64"""
    grid = np.random.default_rng(0).random((12, 12, 12))
    grid[np.random.default_rng(1).random(grid.shape) < 0.5] = 0.0
    w = ref.window_3d(5).double()
    dense = ref.window_sums_dense(torch.from_numpy(grid)[None, None], w)[0, 0].numpy()
    assert np.abs(dense - ref.window_sums_loops(grid, w.numpy())).max() <= 1e-12


def test_window_is_the_reference_construction(pcc):
    """the package's window: float32, the 1-D Gaussian normalised, outer products — equal to the restatement's, bit for bit"""
    from pcc_amd.loss import gaussian_window_3d
    for size in (3, 5, 7, 11):
        w = gaussian_window_3d(size)
        assert w.dtype == torch.float32 and tuple(w.shape) == (size ** 3, 1)
        assert torch.equal(w.reshape(size, size, size), ref.window_3d(size))
        assert abs(float(w.double().sum()) - 1.0) < 1e-6


# ---------------------------------------------------------------------------------------------
# GPU: the HIP path against float64
# ---------------------------------------------------------------------------------------------
def _tensors(pcc, case):
    gt_c, gt_f, pr_c, pr_f, q_f = case
    t = lambda a: torch.from_numpy(a).to(DEV)
    gt = pcc.SparseTensor(coordinates=t(gt_c), features=t(gt_f), device=DEV)
    pred_f = t(pr_f).requires_grad_(True)
    pred = pcc.SparseTensor(pred_f, coordinate_map=pcc.CoordMap(t(pr_c), 1))
    q = pcc.SparseTensor(t(q_f), coordinate_map=gt.map)
    return gt, pred, pred_f, q


def _by_coordinate(coords, values):
    order = np.lexsort((coords[:, 3], coords[:, 2], coords[:, 1], coords[:, 0]))
    return coords[order], values[order]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _hip(pcc, case, window, yuv):
    """-> (union coordinates and map in (b, x, y, z) order, loss, gradient), float64 numpy"""
    from pcc_amd.loss import color_ssim_map
    gt, pred, pred_f, q = _tensors(pcc, case)
    coords, m = color_ssim_map(gt, pred, q, window, yuv)
    assert m.shape == (coords.shape[0], 3)
    loss = m.mean()
    (grad,) = torch.autograd.grad(loss, pred_f)
    c, v = _by_coordinate(coords.cpu().numpy(), m.detach().double().cpu().numpy())
    return c, v, float(loss.detach().double()), grad.double().cpu().numpy()


CASES = [((seed,), window, yuv) for window in (3, 5, 7, 9) for yuv in (False, True) for seed in (1, 2)] + [((3, 4), 5, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("seeds,window,yuv", CASES)
def test_map_loss_and_gradient_against_float64(pcc, seeds, window, yuv):
    case, r64, r32, e_s, e_g, e_L = ref.case_and_references(seeds, window, yuv)
    # conditions on the INPUT: float32 arithmetic alone (the restatement in float32) stays this close to float64
    assert e_s <= 1e-4 and e_g <= 1e-5, (e_s, e_g)
    coords, m, loss, grad = _hip(pcc, case, window, yuv)
    assert np.array_equal(coords, r64["coords"])
    d_s, d_g, d_L = _rel(m, r64["map"]), _rel(grad, r64["grad"]), abs(loss - r64["loss"]) / abs(r64["loss"])
    print(f"seeds {seeds} window {window} yuv {yuv}: map {d_s:.2e} (e_s {e_s:.2e})  grad {d_g:.2e} (e_g {e_g:.2e})  "
          f"loss {d_L:.2e} (e_L {e_L:.2e})")
    assert d_s <= 4 * e_s + 1e-6
    assert d_g <= 4 * e_g + 1e-6
    assert d_L <= 4 * e_L + 1e-6
    # the class is the mean of the map
    from pcc_amd.loss import ColorSSIM
    gt, pred, _, q = _tensors(pcc, case)
    value = ColorSSIM({"id": "ssim", "window_size": window, "yuv": yuv})(gt, {"prediction": pred, "q_map": q})
    assert float(value.detach().double()) == loss


@pytest.mark.gpu
def test_batch_items_equal_the_clouds_alone(pcc):
    """windows never cross batch items: the map of a batch of two, item by item, against each cloud's own float64 map"""
    window, yuv = 5, False
    case, _, _, _, _, _ = ref.case_and_references((3, 4), window, yuv)
    coords, m, _, _ = _hip(pcc, case, window, yuv)
    for b, seed in enumerate((3, 4)):
        _, alone64, _, e_s, _, _ = ref.case_and_references((seed,), window, yuv)
        sel = coords[:, 0] == b
        assert np.array_equal(coords[sel][:, 1:], alone64["coords"][:, 1:])
        assert _rel(m[sel], alone64["map"]) <= 4 * e_s + 1e-6
        alone_c, alone_m, _, _ = _hip(pcc, ref.shell_case(seed), window, yuv)
        assert np.array_equal(alone_m, m[sel])              # and the HIP path alone gives the same bits


@pytest.mark.gpu
def test_scattered_cloud_is_finite(pcc):
    """30 % random voxels, window 3: ill-conditioned by construction of the formula, so only finiteness is asserted"""
    rng = np.random.default_rng(7)
    occ = np.argwhere(rng.random((16, 16, 16)) < 0.3)
    pocc = np.argwhere(rng.random((16, 16, 16)) < 0.3)
    rows = lambda c: np.concatenate([np.zeros((c.shape[0], 1)), c], axis=1).astype(np.int32)
    case = (rows(occ), rng.random((occ.shape[0], 3)).astype(np.float32), rows(pocc), rng.random((pocc.shape[0], 3)).astype(np.float32),
            rng.random((occ.shape[0], 2)).astype(np.float32))
    _, m, loss, grad = _hip(pcc, case, 3, False)
    assert np.isfinite(loss) and np.isfinite(grad).all() and np.isfinite(m).all()


@pytest.mark.gpu
def test_dispatcher_and_training_step(pcc):
    """Loss(OURS_LOSS + ColorSSIM) on the 32^3 synthetic frame, model in train mode: total = sum of the parts, the SSIM part
    finite and bounded, backward() leaves finite gradients everywhere and a non-zero one on the last colour layer.

    The bound.  An element of the map is (1 - SSIM) / 2 times the weight, times 0.75 / 0.125 / 0.125 with yuv, and SSIM lies
    in [-1, 1] (luminance and structure in [-1, 1], lightness in (0, 1]), so with weights in [0, 1] the part lies in [0, 1].
    The weight is column 1 of what the model hands on as "q_map", and that is its third argument (model.py:89 of the
    reference: the lambda map).  So the part is held to [0, 1] with the q-map itself (0.7 here) in that place; with the lambda
    map of tests/test_train_model.py (2^(7 q) + 99 = 128.9 here), which a training step uses, the same reasoning gives
    [0, max lambda / 3], 1/3 being the mean of the yuv factors.  (Measured on the MI355X: 9.88 with the lambda map.)"""
    from pcc_amd import synthetic as syn
    from pcc_amd.loss import OURS_LOSS, Loss
    model = syn.make_model(seed=0, device=DEV)
    pts = syn.sphere_shell(**syn.CONFIG1)
    qc, qf = syn.uniform_qmap(pts[:, :3], 0.3, 0.7)
    lam = np.stack([2 ** (qf[:, 0] * 6) + 24, 2 ** (qf[:, 1] * 7) + 99], axis=1).astype(np.float32)
    model.train()
    inp = pcc.SparseTensor(coordinates=torch.from_numpy(qc).to(DEV), features=torch.from_numpy(pts[:, 3:]).to(DEV), device=DEV)
    Q = pcc.SparseTensor(torch.from_numpy(qf).to(DEV), coordinate_map=inp.map)
    Lam = pcc.SparseTensor(torch.from_numpy(lam).to(DEV), coordinate_map=inp.map)
    loss_fn = Loss(dict(OURS_LOSS, ssim={"type": "ColorSSIM", "window_size": 5, "yuv": True}))
    assert "ssim" in loss_fn.losses
    total, parts = loss_fn(inp, model(inp, Q, Lam))
    assert set(parts) == set(OURS_LOSS) | {"ssim"}
    summed = sum(float(v.detach().double()) for v in parts.values())
    assert abs(float(total.detach().double()) - summed) <= 1e-5 * abs(summed)
    ssim = float(parts["ssim"].detach())
    with torch.no_grad():                                   # the same step weighted by the q-map itself: weights in [0, 1]
        unit = float(loss_fn(inp, model(inp, Q, Q))[1]["ssim"])
    print(f"SSIM part: {unit:.6f} weighted by the q-map, {ssim:.6f} weighted by the lambda map (max {lam[:, 1].max():.3f})")
    assert np.isfinite(unit) and 0.0 <= unit <= 1.0
    assert np.isfinite(ssim) and 0.0 <= ssim <= float(lam[:, 1].max()) / 3
    total.backward()
    seen = 0
    for name, p in model.named_parameters():
        if p.grad is not None:
            seen += 1
            assert bool(torch.isfinite(p.grad).all()), name
    assert seen > 100
    last = model.g_s.post_conv[4].kernel.grad
    assert last is not None and float(last.abs().max()) > 0.0
    # the SSIM term alone reaches the colour layer too
    model.zero_grad()
    out = model(inp, Q, Lam)
    Loss({"ssim": {"type": "ColorSSIM", "window_size": 5, "yuv": False}})(inp, out)[0].backward()
    last = model.g_s.post_conv[4].kernel.grad
    assert last is not None and bool(torch.isfinite(last).all()) and float(last.abs().max()) > 0.0
