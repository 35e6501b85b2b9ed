"""pcc_scaled_cells and pcc_scaled_transfer (csrc/rescale.hip) through pcc_amd.rescale on the GPU: every output EQUAL to the numpy
restatement (tests/_scaled_reference.py), on Morton-sorted rows (long runs: the in-wave fold), shuffled rows (the no-fold branch)
and one cell shared by several waves; the association cross-checked against metrics.nearest_neighbours; batch items kept apart;
bitwise reproducibility; the errors."""
import numpy as np
import pytest
import torch

import _scaled_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 63, 64, 65, 255, 256, 257, 2855)
SCALES = ((1, 8), (1, 2), (3, 4), (5, 7), (1, 1))
CHANNELS = (0, 1, 3, 16)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def check_against(want, coords, attr, scale, channels=CHANNELS):
    """every output of the two entry points and of quantize_coords against the restatement ``want`` (made with all of ``attr``'s
    channels), for each channel count"""
    from pcc_amd import rescale
    num, den = scale
    C = dev(coords, torch.int32)
    for c in channels:
        A = dev(attr[:, :c], torch.float32) if c else None
        cells, first, npts, sums, row, table = rescale.scaled_cells(C, A, num, den)
        assert np.array_equal(cells.cpu().numpy(), want["cells"]) and cells.dtype == torch.int32
        assert np.array_equal(first.cpu().numpy(), want["first"]) and np.array_equal(row.cpu().numpy(), want["row"])
        assert np.array_equal(npts.cpu().numpy(), want["own_npts"])
        if c:
            assert sums.dtype == torch.int64 and np.array_equal(sums.cpu().numpy(), want["own_sums"][:, :c])
        else:
            assert sums is None
        q = rescale.quantize_coords(C, A, scale, "nearest")
        assert (q.num, q.den) == scale
        assert np.array_equal(q.cells.cpu().numpy(), want["cells"]) and np.array_equal(q.positions.cpu().numpy(), want["positions"])
        assert np.array_equal(q.first.cpu().numpy(), want["first"]) and np.array_equal(q.row.cpu().numpy(), want["row"])
        assert q.nearest.dtype == torch.int32 and np.array_equal(q.nearest.cpu().numpy(), want["nearest"])
        assert q.d2.dtype == torch.int64 and np.array_equal(q.d2.cpu().numpy(), want["d2"])
        assert np.array_equal(q.counts.cpu().numpy(), want["counts"])
        if c:
            assert np.array_equal(q.sums.cpu().numpy(), want["sums"][:, :c])
            assert q.features.dtype == torch.float32 and np.array_equal(q.features.cpu().numpy(), want["features"][:, :c])
            own = rescale.quantize_coords(C, A, scale, "cell")
            assert own.nearest is None and own.d2 is None and np.array_equal(own.counts.cpu().numpy(), want["own_npts"])
            assert np.array_equal(own.features.cpu().numpy(), want["own_features"][:, :c])
        else:
            assert q.sums is None and q.features is None


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: "%d_%d" % s)
@pytest.mark.parametrize("n", SIZES)
def test_outputs_equal_the_restatement(pcc, n, scale):
    p = ref.shell()[:n]
    assert len(p) == n
    attr = ref.colours(n, 16, 21)
    for name, order in (("morton", ref.morton_order(p)), ("shuffled", np.arange(n))):
        coords = ref.with_batch(p[order])
        want = ref.quantize_reference(coords, attr[order], *scale)
        if n >= 255:
            runs = int((want["nearest"][1:] == want["nearest"][:-1]).sum())
            print(f"n {n} scale {scale[0]}/{scale[1]} {name}: {len(want['cells'])} cells, {runs} neighbouring rows share a destination, "
                  f"{want['empty'].size} cells no point chose")
            if scale == (1, 8):                            # sorted rows have runs to fold; shuffled rows have next to none
                assert runs > n // 5 if name == "morton" else runs < n // 50
        check_against(want, coords, attr[order], scale)


def test_one_cell_shared_across_waves(pcc):
    p = ref.one_cell_points(300)
    coords, attr = ref.with_batch(p), ref.colours(300, 3, 5)
    want = ref.quantize_reference(coords, attr, 1, 8)
    assert want["cells"].tolist() == [[0, -3, 2, 1]] and want["counts"].tolist() == [300] and not want["nearest"].any()
    check_against(want, coords, attr, (1, 8), channels=(0, 3))
    # and next to a second, sparsely filled cell: rows of two destinations alternate
    both = np.concatenate([p, ref.one_cell_points(40, cell=(-2, 2, 1), seed=6)])
    both = both[np.random.default_rng(1).permutation(340)]
    coords, attr = ref.with_batch(both), ref.colours(340, 3, 6)
    check_against(ref.quantize_reference(coords, attr, 1, 8), coords, attr, (1, 8), channels=(3,))


@pytest.mark.parametrize("scale", ((1, 8), (1, 4), (1, 2), (3, 4), (5, 7), (15, 16)), ids=lambda s: "%d_%d" % s)
def test_association_agrees_with_the_metric_search(pcc, scale):
    """the same association the parent's way: the source into a CoordMap of the reconstructed positions"""
    from pcc_amd import CoordMap, rescale
    from pcc_amd.metrics import nearest_neighbours
    C = dev(ref.with_batch(ref.shell()), torch.int32)
    q = rescale.quantize_coords(C, None, scale)
    recon = torch.cat([q.cells[:, :1], q.positions], dim=1).contiguous()
    idx, d2, _, _ = nearest_neighbours(C, CoordMap(recon, 1))
    assert torch.equal(idx, q.nearest) and torch.equal(d2, q.d2)
    want = ref.shell_reference(*scale)
    assert np.array_equal(q.nearest.cpu().numpy(), want["nearest"]) and np.array_equal(q.d2.cpu().numpy(), want["d2"])


def test_batch_items_neither_merge_nor_associate_across(pcc):
    p = ref.shell()
    a, b = p[:500], p[:500] + np.array([1, 0, 0])            # item 1: the same surface one voxel on, so most cells are shared
    coords = np.concatenate([ref.with_batch(a, 0), ref.with_batch(b, 1)])
    coords = coords[np.random.default_rng(3).permutation(1000)]
    attr = ref.colours(1000, 3, 9)
    for scale in ((1, 4), (1, 2), (3, 4)):
        want = ref.quantize_reference(coords, attr, *scale)
        cells = want["cells"]
        shared = set(map(tuple, cells[cells[:, 0] == 0][:, 1:].tolist())) & set(map(tuple, cells[cells[:, 0] == 1][:, 1:].tolist()))
        assert len(shared) > 50
        assert np.array_equal(cells[want["nearest"], 0], coords[:, 0])          # the restatement never crosses items
        check_against(want, coords, attr, scale, channels=(3,))
        # each item alone gives its own part of the joint result
        for item in (0, 1):
            rows = coords[:, 0] == item
            alone = ref.quantize_reference(coords[rows], attr[rows], *scale)
            assert np.array_equal(alone["cells"], cells[cells[:, 0] == item])
            assert np.array_equal(alone["d2"], want["d2"][rows])
            assert np.array_equal(alone["features"], want["features"][cells[:, 0] == item])


def test_two_runs_give_equal_bytes(pcc):
    from pcc_amd import rescale
    p = ref.shell()
    C = dev(ref.with_batch(p[ref.morton_order(p)]), torch.int32)
    A = dev(ref.colours(len(p), 3, 2), torch.float32)
    for scale in ((1, 8), (3, 4)):
        first = rescale.quantize_coords(C, A, scale)
        again = rescale.quantize_coords(C, A, scale)
        for name in ("cells", "positions", "row", "first", "counts", "sums", "features", "nearest", "d2"):
            x, y = getattr(first, name), getattr(again, name)
            assert x.dtype == y.dtype and bytes(x.cpu().numpy().tobytes()) == bytes(y.cpu().numpy().tobytes()), name


def test_quantize_takes_a_cloud(pcc):
    from pcc_amd import rescale
    p = ref.shell()[:700]
    attr = ref.colours(700, 3, 12)
    x = torch.from_numpy(np.concatenate([p.astype(np.float32), attr], axis=1)).to(DEV)
    want = ref.quantize_reference(ref.with_batch(p), attr, 3, 4)
    for scale in (0.75, (3, 4), (6, 8)):
        q = rescale.quantize(x, scale)
        assert np.array_equal(q.cells.cpu().numpy(), want["cells"]) and np.array_equal(q.features.cpu().numpy(), want["features"])
        assert np.array_equal(q.nearest.cpu().numpy(), want["nearest"]) and (q.num, q.den) == (3, 4)
    own = rescale.quantize(x, 0.75, transfer="cell")
    assert np.array_equal(own.features.cpu().numpy(), want["own_features"]) and own.nearest is None
    geometry = rescale.quantize(x[:, :3], 0.75)
    assert geometry.features is None and np.array_equal(geometry.d2.cpu().numpy(), want["d2"])
    empty = rescale.quantize(x[:0], 0.5)
    assert tuple(empty.cells.shape) == (0, 4) and tuple(empty.features.shape) == (0, 3) and tuple(empty.nearest.shape) == (0,)
    with pytest.raises(ValueError):
        rescale.quantize(x, 0.75, transfer="blend")
    with pytest.raises(ValueError):
        rescale.quantize(x, 0.3)
    with pytest.raises(RuntimeError):
        rescale.quantize(x.cpu(), 0.5)


def test_errors(pcc):
    from pcc_amd import rescale
    p = ref.shell()[:300]
    attr = ref.colours(300, 3, 1)
    C = dev(ref.with_batch(p), torch.int32)
    for bad in (1.5, float("nan"), float("-inf"), -1.0000001):
        a = attr.copy()
        a[171, 1] = bad
        for transfer in ("nearest", "cell"):
            with pytest.raises(ValueError):
                rescale.quantize_coords(C, dev(a, torch.float32), (1, 2), transfer)
    a = attr.copy()
    a[171, 1] = -1.0                                          # the range's edge is inside it
    rescale.quantize_coords(C, dev(a, torch.float32), (1, 2))
    # the extent is checked on the host: a source coordinate, or a position it maps to, beyond the limit
    limit = rescale.COORD_LIMIT
    for xyz, scale, ok in (((limit, 0, 0), (1, 1), True), ((limit + 1, 0, 0), (1, 1), False), ((0, -limit - 1, 0), (1, 8), False),
                           ((0, 0, limit), (1, 8), True), ((0, 0, limit), (2, 3), False), ((0, 0, -limit), (2, 3), True)):
        c = ref.with_batch(np.concatenate([p, [xyz]]))
        if ok:
            q = rescale.quantize_coords(dev(c, torch.int32), None, scale)
            want = ref.quantize_reference(c, None, *scale)
            assert np.array_equal(q.positions.cpu().numpy(), want["positions"]) and np.array_equal(q.d2.cpu().numpy(), want["d2"])
        else:
            with pytest.raises(ValueError):
                rescale.quantize_coords(dev(c, torch.int32), None, scale)
    with pytest.raises(ValueError):
        rescale.quantize_coords(dev(ref.with_batch(p, 1023), torch.int32), None, (1, 2))
    with pytest.raises(ValueError):
        rescale.quantize_coords(C, dev(ref.colours(300, 17, 1), torch.float32), (1, 2))
    with pytest.raises(ValueError):
        rescale.quantize_coords(C.long(), None, (1, 2))
