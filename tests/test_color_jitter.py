"""pcc_color_jitter (csrc/augment.hip): within JITTER_TOL of the float64 restatement of torchvision's ColorJitter
(tests/_augment_reference.py: the tolerance is measured there, float32 restatement against float64, never against the kernel),
bitwise reproducible, and an item's bytes do not depend on the batch around it."""
import functools

import numpy as np
import pytest
import torch

import _augment_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_abi(pcc, rgb, offsets, params, order):
    from pcc_amd._lib import check, ptr, stream
    L = pcc.lib()
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    n, nbatch = rgb.shape[0], len(offsets) - 1
    F = torch.from_numpy(rgb).to(DEV)
    off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(DEV)
    par = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32)).to(DEV)
    ordr = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(DEV)
    nbytes = L.pcc_color_jitter_scratch_bytes(n, nbatch)
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=DEV)
    out = torch.full((max(n, 1), 3), -5.0, dtype=torch.float32, device=DEV)
    check(L.pcc_color_jitter(ptr(F), n, ptr(off), nbatch, ptr(par), ptr(ordr), ptr(out), ptr(scratch), nbytes, stream()))
    return out[:n].cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(name):
    return ref.jitter_reference(*ref.jitter_cases()[name], np.float64)


def test_chunk_size_is_the_one_the_cases_straddle(pcc):
    assert pcc.lib().pcc_color_jitter_chunk() == ref.JITTER_CHUNK
    for k in (1, 2):
        assert {k * ref.JITTER_CHUNK - 1, k * ref.JITTER_CHUNK, k * ref.JITTER_CHUNK + 1} <= set(ref.ITEM_SIZES)


@pytest.mark.parametrize("name", ["sizes", "empty", "orders", "extremes", "large"])
def test_within_measured_tolerance_of_float64(pcc, name):
    rgb, off, par, order = ref.jitter_cases()[name]
    got = run_abi(pcc, rgb, off, par, order)
    want = reference(name)
    err = np.abs(got.astype(np.float64) - want)
    print(f"{name}: n={rgb.shape[0]} items={len(off) - 1} max |gpu - float64| = {err.max():.3e} (tolerance {ref.JITTER_TOL:.3e})")
    assert got.min() >= 0.0 and got.max() <= 1.0
    assert err.max() <= ref.JITTER_TOL, (np.unravel_index(err.argmax(), err.shape), err.max())
    again = run_abi(pcc, rgb, off, par, order)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))          # two runs: the same bytes


@pytest.mark.parametrize("name", ["sizes", "empty", "extremes", "large"])
def test_item_alone_equals_item_in_batch(pcc, name):
    rgb, off, par, order = ref.jitter_cases()[name]
    batch = run_abi(pcc, rgb, off, par, order)
    for i in range(len(off) - 1):
        lo, hi = int(off[i]), int(off[i + 1])
        if hi == lo:
            continue
        alone = run_abi(pcc, rgb[lo:hi], [0, hi - lo], par[i:i + 1], order[i:i + 1])
        assert np.array_equal(alone.view(np.uint32), batch[lo:hi].view(np.uint32)), (name, i)


def test_special_colours_under_every_single_op(pcc):
    """gray points, black, primaries and ties of the maximum through hue shifts that wrap in both directions, alone"""
    sp = ref.special_colours()
    shifts = (-0.3, 0.3, -0.05, 0.05, 0.0)
    off = np.arange(len(shifts) + 1, dtype=np.int64) * sp.shape[0]
    rgb = np.tile(sp, (len(shifts), 1))
    par = np.array([(1.0, 1.0, 1.0, f) for f in shifts], dtype=np.float32)
    order = np.tile(np.array([[3, 0, 1, 2]], dtype=np.int32), (len(shifts), 1))
    got = run_abi(pcc, rgb, off, par, order)
    want = ref.jitter_reference(rgb, off, par, order, np.float64)
    # contrast with factor 1 is the identity whatever the mean, so this is the hue operation alone
    assert np.abs(got - want).max() <= ref.JITTER_TOL
    gray = sp[:, 0] == sp[:, 1]
    gray &= sp[:, 1] == sp[:, 2]
    for k in range(len(shifts)):
        assert np.array_equal(got[k * sp.shape[0]:(k + 1) * sp.shape[0]][gray], sp[gray])      # cr = 0: unchanged, exactly


def test_python_color_jitter_finds_the_items(pcc):
    from pcc_amd import augment
    rgb, off, par, order = ref.jitter_cases()["empty"]
    b = np.repeat(np.arange(len(off) - 1), np.diff(off))
    C = np.zeros((rgb.shape[0], 4), dtype=np.int32)
    C[:, 0] = b
    got = augment.color_jitter(torch.from_numpy(C).to(DEV), torch.from_numpy(rgb).to(DEV), par, order)
    assert np.array_equal(got.cpu().numpy(), run_abi(pcc, rgb, off, par, order))
    with pytest.raises(ValueError):
        augment.color_jitter(torch.from_numpy(C).to(DEV), torch.from_numpy(rgb).to(DEV), par, np.zeros_like(order))
