"""The ROW ORDER of the coordinate manager's sets (csrc/first_rows.h through coords.hip's unique_coords): unique candidates in
order of first appearance, the lowest candidate index wins.  The set tests of test_hip_parity.py compare sets; here the
output rows are held to equality, in order, with a numpy restatement of the rule, for the seven-launch form and for the
one-workgroup form (pcc_small_paths bit 2) alike, and the returned table must index the rows.

Candidate order (include/pcc_hip.h): stride map — floor(c / 2 ts) 2 ts, row by row; children of kernel 3 — candidate 27 p + k;
children of kernel 2 — candidate k n + p; offsets kernel_offsets(ks) ts / 2.

Cases: the table's shift (log2 of the output set's stride) is 1 and 4 for the stride maps of strides 1 and 8, and 0 and 2
for the children of strides 2 and 8 (a child set needs an even parent stride, so 2 stands where the stride maps have 1: its
output stride 1 is the shift of 0).  Candidate counts of 1 (one parent), just below / at / just above 1,024 (one scan tile),
at 8,192 (the largest one-workgroup set) and just above it; kernel 3 takes the nearest multiples of 27.
"""
import numpy as np
import pytest
import torch

from oracle import coords as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_M = 8192                       # csrc/coords.hip UNIQUE_SMALL_M


def voxels(n, side, ts, seed):
    """n distinct random voxels (two batch items) of a side^3 cube around the origin, scaled by ts, in random order"""
    rng = np.random.default_rng(seed)
    cell = rng.permutation(2 * side ** 3)[:n]
    b, cell = cell // side ** 3, cell % side ** 3
    xyz = np.stack([cell % side, (cell // side) % side, cell // side ** 2], axis=1) - side // 2
    return np.concatenate([b[:, None], xyz * ts], axis=1).astype(np.int32)


def first_rows(cand):
    _, first = np.unique(oc.pack(cand), return_index=True)
    return cand[np.sort(first)]


def stride_candidates(c, ts):
    return np.concatenate([c[:, :1], np.floor_divide(c[:, 1:], 2 * ts) * (2 * ts)], axis=1).astype(np.int32)


def children_candidates(c, ts, ks):
    offs = oc.kernel_offsets(ks) * ts // 2
    K = offs.shape[0]
    if ks == 3:                                                      # candidate 27 p + k
        b, xyz = np.repeat(c[:, 0], K), c[:, None, 1:] + offs[None]
    else:                                                            # candidate k n + p
        b, xyz = np.tile(c[:, 0], K), c[None, :, 1:] + offs[:, None]
    return np.concatenate([b[:, None], xyz.reshape(-1, 3)], axis=1).astype(np.int32)


def check_both_forms(pcc, build, cand, collide):
    from pcc_amd import sparse as sp
    m = cand.shape[0]
    want = first_rows(cand)
    if collide:
        assert want.shape[0] < m, "the case was meant to hold duplicates"
    else:
        assert want.shape[0] == m
    was = sp.set_small_paths(-1)
    try:
        for small in ((True, False) if m <= SMALL_M else (False,)):
            sp.set_small_paths((was | 4) if small else (was & ~4))
            out = build()
            got = out.coords.cpu().numpy()
            print(f"m={m} small={small} n_out={got.shape[0]} want={want.shape[0]}")
            assert got.shape == want.shape and (got == want).all(), f"one-workgroup form: {small}"
            assert (out.lookup(out.coords).cpu().numpy() == np.arange(got.shape[0])).all()
    finally:
        sp.set_small_paths(was)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 8192, 8193])
@pytest.mark.parametrize("ts", [1, 8])
def test_stride_map_rows_in_order_of_first_appearance(pcc, ts, n):
    """distinct voxels of a 32^3 cube (negative halves included: a true floor division): 8 of them share a parent"""
    c = voxels(n, 32, ts, seed=n)
    d = torch.as_tensor(c).to(DEV)
    check_both_forms(pcc, lambda: pcc.CoordMap(d, ts).down(), stride_candidates(c, ts), collide=n > 1)


@pytest.mark.parametrize("n", [1, 37, 38, 303, 304])                # 27, 999, 1,026, 8,181 and 8,208 candidates
@pytest.mark.parametrize("ts", [2, 8])
def test_children_of_kernel_3_rows_in_order_of_first_appearance(pcc, ts, n):
    """parents from an 8^3 block of the stride grid: neighbours share the children between them"""
    c = voxels(n, 8, ts, seed=100 + n)
    d = torch.as_tensor(c).to(DEV)
    check_both_forms(pcc, lambda: pcc.CoordMap(d, ts).up(3), children_candidates(c, ts, 3), collide=n > 1)


@pytest.mark.parametrize("n", [1, 127, 128, 129, 1024, 1025])       # 8, 1,016, 1,024, 1,032, 8,192 and 8,200 candidates
@pytest.mark.parametrize("ts", [2, 8])
def test_children_of_kernel_2_rows_in_candidate_order(pcc, ts, n):
    """the 8 children of distinct parents never collide: the order alone is checked (offset-major: candidate k n + p)"""
    c = voxels(n, 32, ts, seed=200 + n)
    d = torch.as_tensor(c).to(DEV)
    check_both_forms(pcc, lambda: pcc.CoordMap(d, ts).up(2), children_candidates(c, ts, 2), collide=False)
