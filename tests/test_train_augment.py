"""pcc_amd.augment.TrainAugment on a collated batch of two small cubes, one below and one above the 1000-point rotation gate:
seeded bytes, unique output voxels, the gate, and one training step on the augmented batch."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK = 32


@functools.lru_cache(maxsize=None)
def batch():
    from pcc_amd import synthetic as syn
    from pcc_amd.utils import sparse_collate
    small = syn.sphere_shell(grid=32, radius=7.0, half_width=0.6)
    big = syn.sphere_shell(**syn.CONFIG1)
    assert 100 < small.shape[0] <= 1000 < big.shape[0]
    C, F = sparse_collate([torch.from_numpy(small[:, :3]), torch.from_numpy(big[:, :3])],
                          [torch.from_numpy(small[:, 3:6]), torch.from_numpy(big[:, 3:6])])
    return C, F, small.shape[0]


def augmented(seed):
    from pcc_amd.augment import TrainAugment
    C, F, _ = batch()
    aug = TrainAugment(block_size=BLOCK, seed=seed)
    C2, F2 = aug(C.to(DEV), F.to(DEV))
    return C2, F2


def test_same_seed_same_bytes_other_seed_other_output(pcc):
    a, b, c = augmented(7), augmented(7), augmented(8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert a[0].shape != c[0].shape or not torch.equal(a[0], c[0])
    n_small = batch()[2]
    assert not torch.equal(a[1][:n_small], c[1][:n_small])                   # the jitter differs too
    # a second call of ONE object goes on in its stream of draws
    from pcc_amd.augment import TrainAugment
    C, F, _ = batch()
    aug = TrainAugment(block_size=BLOCK, seed=7)
    first = aug(C.to(DEV), F.to(DEV))
    second = aug(C.to(DEV), F.to(DEV))
    assert torch.equal(first[0], a[0]) and not torch.equal(first[1][:n_small], second[1][:n_small])


def test_output_is_unique_gated_and_in_range(pcc):
    C, F, n_small = batch()
    C2, F2 = augmented(11)
    assert C2.dtype == torch.int32 and F2.dtype == torch.float32 and C2.shape[0] == F2.shape[0] and F2.shape[1] == 3
    cm = pcc.CoordMap(C2)
    cm.count_duplicates()
    cm.table()
    assert cm.duplicates() == 0
    # the small cube is not rotated: its coordinates are unchanged, its colours are jittered
    assert torch.equal(C2[:n_small].cpu(), C[:n_small])
    assert not torch.equal(F2[:n_small].cpu(), F[:n_small])
    # the big cube is: rows stay grouped by item, duplicates were dropped, colours stay in [0, 1]
    assert bool((C2[n_small:, 0] == 1).all()) and C2.shape[0] <= C.shape[0]
    assert not torch.equal(C2[n_small:n_small + 200].cpu(), C[n_small:n_small + 200])
    assert float(F2.min()) >= 0.0 and float(F2.max()) <= 1.0
    # with the gate above both cubes nothing moves
    from pcc_amd.augment import TrainAugment
    C3, _ = TrainAugment(block_size=BLOCK, seed=11, min_rotate_points=10 ** 6)(C.to(DEV), F.to(DEV))
    assert torch.equal(C3.cpu(), C)


def test_draws_follow_the_documented_order(pcc):
    from pcc_amd.augment import TrainAugment, rotation_matrices
    aug = TrainAugment(block_size=BLOCK, seed=3)
    params, order, matrices = aug.draw([500, 5000])
    rng = np.random.default_rng(3)
    for i in range(2):
        assert np.array_equal(order[i], rng.permutation(4))
        want = [rng.uniform(0.7, 1.3), rng.uniform(0.7, 1.3), rng.uniform(0.7, 1.3), rng.uniform(-0.3, 0.3)]
        assert np.array_equal(params[i], np.asarray(want, dtype=np.float32))
        phi, theta = rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        want_m = np.eye(3, dtype=np.float32).reshape(9) if i == 0 else rotation_matrices([phi], [theta])[0]
        assert np.array_equal(matrices[i], want_m)


def test_training_step_on_the_augmented_batch(pcc):
    from pcc_amd import synthetic as syn
    from pcc_amd.loss import OURS_LOSS, Loss
    from pcc_amd.q_map import Q_Map
    C2, F2 = augmented(5)
    model = syn.make_model(seed=0, device=DEV)
    model.train()
    inp = pcc.SparseTensor(coordinates=C2, features=F2, device=DEV)
    qgen = Q_Map({"mode": "exponential", "lambda_A_max": 12800, "lambda_A_min": 100, "lambda_G_max": 1600, "lambda_G_min": 25})
    Q, Lam = qgen(inp)
    total, _ = Loss(OURS_LOSS)(inp, model(inp, Q, Lam))
    total.backward()
    assert bool(torch.isfinite(total.detach()))
    grads = [p.grad for n, p in model.named_parameters() if not n.endswith(".quantiles")]
    assert sum(g is not None for g in grads) > 50
    assert all(bool(torch.isfinite(g).all()) for g in grads if g is not None)
    assert any(float(g.abs().max()) > 0 for g in grads if g is not None)
