"""pcc_surface_variation and pcc_pcqm_features (csrc/pcqm.hip) against the numpy restatement (tests/_pcqm_reference.py).

The kernels are fed numpy-made attribute planes and associations, so they alone are judged.  Bounds:

* kappa: 1e-12 absolute.  kappa is a ratio of eigenvalues of an exactly known integer matrix; the kernel's Jacobi and numpy's
  eigvalsh each carry O(10^2) float64 round-offs relative to the largest eigenvalue (the argument of tests/test_normals.py), and
  kappa <= 1/3: 1.1e-16 * 1e2 with two orders to spare.  Validity is an integer predicate and must be equal.
* statistics: a sum of `count` rounded products of magnitude sum w|x| is off by at most count * 2^-53 * sum w|x| on either side,
  hence count * 2^-52 * sum w|x| between two evaluations: the bound of sum w (x = 1) and of the means (x the attribute: a
  float64 mean cannot be held tighter than its own half ulp, whatever is added up).  Second moments likewise with sum w x^2, x
  the values shifted by the centre's attribute — what the kernel adds, and a magnitude that does not grow with the attribute's
  (cross terms: sqrt(sum w u^2 * sum w v^2), which bounds sum w |u v|).  The statistics are judged against the restatement
  evaluated in numpy.longdouble: in float64 the two-pass form subtracts a rounded mean of the attribute's full magnitude from
  every value, an error of its own that exceeds the shifted sums' bound where the weights are small (h = 1: 46 times, and a
  variance that is exactly 0 comes out as 1e-34); the bound carries the longdouble evaluation's error, count * 2^-63 * the
  unshifted sums, beside the kernel's.  The float64 comparison is printed, not asserted.
* features from the kernel's own statistics: add, multiply, divide and sqrt are correctly rounded and the build does not
  contract them (-ffp-contract=off), so numpy repeats the kernel's operations: 4 ulp of 1.0, absolute.
* features end to end: e = the largest float64-versus-longdouble difference of the restatement on the input; the kernel stays
  within 8 e of the float64 restatement (one-pass shifted sums round differently from two-pass ones, and sqrt near a small
  variance amplifies both alike).
* pooled sums: n * 2^-53 * sum |f| against math.fsum."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import _pcqm_reference as ref

DEV = "cuda:0"
ULP = 2.0 ** -52
EPS_LD = float(np.finfo(np.longdouble).eps)
CONSTS = (1.0, 1.0, 0.002, 0.1)


# ---- the C ABI's argument checks: no GPU ------------------------------------------------------------------------------------

def test_argument_checks_of_the_c_abi(pcc):
    """every refusal happens before a launch and names its argument (runs without a GPU; fails where the symbols are missing)"""
    L = pcc.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data                                           # stands in for every required pointer: nothing is launched
    consts = (ctypes.c_double * 4)(*CONSTS)
    c = ctypes.addressof(consts)

    for R in (0, 9):
        assert L.pcc_surface_variation(p, 1, p, p, 1024, 1, R, p, None) < 0
        assert b"radius" in L.pcc_last_error()
    assert L.pcc_surface_variation(p, 1, p, p, 1000, 1, 3, p, None) < 0
    assert b"cap" in L.pcc_last_error()
    assert L.pcc_surface_variation(p, 1, p, p, 1024, 1, 3, None, None) < 0
    assert b"kappa" in L.pcc_last_error()
    assert L.pcc_surface_variation(None, 1, p, p, 1024, 1, 3, p, None) < 0
    assert b"coords" in L.pcc_last_error()
    assert L.pcc_surface_variation(None, 0, None, None, 1024, 1, 3, p, None) == 0

    def call(n_r=1, n_d=1, cap_r=1024, cap_d=1024, h=3, coords_r=p, nn=p, attrs_r=p, w=p, constants=c, stats=p, features=p, sums=None,
             scratch=None, scratch_bytes=0):
        return L.pcc_pcqm_features(coords_r, n_r, p, p, cap_r, p, n_d, p, p, cap_d, 1, nn, attrs_r, p, w, h, constants, stats, features, sums,
                                   scratch, scratch_bytes, None)

    for h in (0, 9):
        assert call(h=h) < 0
        assert b" h " in L.pcc_last_error()
    assert call(cap_r=1000) < 0
    assert b"cap_r" in L.pcc_last_error()
    assert call(cap_d=24) < 0
    assert b"cap_d" in L.pcc_last_error()
    assert call(stats=None, features=None, sums=None) < 0
    assert b"outputs" in L.pcc_last_error()
    assert call(constants=None) < 0
    assert b"constants" in L.pcc_last_error()
    assert call(coords_r=None) < 0
    assert b"coords_r" in L.pcc_last_error()
    for name in ("nn", "attrs_r", "w"):
        assert call(**{name: None}) < 0
        assert name.encode() in L.pcc_last_error()
    assert call(n_d=0) < 0
    assert b"n_d" in L.pcc_last_error()
    assert L.pcc_pcqm_scratch_bytes(1000) >= 8 * 8 * ((1000 + 255) // 256)
    assert L.pcc_pcqm_scratch_bytes(-1) == 0
    assert call(n_r=1000, sums=p, scratch=None) < 0
    assert b"scratch" in L.pcc_last_error()
    assert call(n_r=1000, sums=p, scratch=p, scratch_bytes=L.pcc_pcqm_scratch_bytes(1000) - 1) < 0
    assert b"scratch" in L.pcc_last_error()
    assert call(n_r=0, n_d=0) == 0                                 # nothing to do (sums, which a launch zeroes, not asked for)


# ---- GPU --------------------------------------------------------------------------------------------------------------------

def _coords(xyz, batch=None):
    b = np.zeros(len(xyz), np.int64) if batch is None else batch
    return torch.from_numpy(np.concatenate([b[:, None], np.asarray(xyz, np.int64)], axis=1).astype(np.int32)).to(DEV)


@functools.lru_cache(maxsize=None)
def inputs(noise=12):
    """the shell pair as numpy: integer coordinates, attribute planes at radius 1 and the association"""
    R, D = ref.shell_pair(noise)
    r_xyz, d_xyz = R[:, :3].astype(np.int64), D[:, :3].astype(np.int64)
    return r_xyz, ref.attributes(R, 1), d_xyz, ref.attributes(D, 1), ref.nearest(r_xyz, d_xyz)


def run_features(r_xyz, ar, d_xyz, ad, nn, h, w=None, batch_r=None, batch_d=None, consts=CONSTS):
    """-> (stats, features, sums) as numpy"""
    from pcc_amd import CoordMap
    from pcc_amd.pcqm import pcqm_features
    cr, cd = _coords(r_xyz, batch_r), _coords(d_xyz, batch_d)
    nb = 1 if batch_r is None else int(batch_r.max()) + 1
    stats, features, sums = pcqm_features(cr, CoordMap(cr, 1, nbatch=nb), torch.from_numpy(ar).to(DEV), cd, CoordMap(cd, 1, nbatch=nb),
                                          torch.from_numpy(ad).to(DEV), torch.from_numpy(nn.astype(np.int32)).to(DEV), h, weight_table=w,
                                          k_L=consts[0], k_kappa=consts[1], c_chroma=consts[2], c_hue=consts[3], want_stats=True)
    assert stats.dtype == features.dtype == sums.dtype == torch.float64
    return stats.cpu().numpy(), features.cpu().numpy(), sums.cpu().numpy()


@functools.lru_cache(maxsize=None)
def gpu(h):
    return run_features(*inputs(), h)


@functools.lru_cache(maxsize=None)
def restated(h, dtype=np.float64):
    r_xyz, ar, d_xyz, ad, nn = inputs()
    return ref.stats(r_xyz, ar, d_xyz, ad, nn, h, ref.gaussian_weights(h), dtype=dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 2, 4, 8])
def test_surface_variation_matches_eigvalsh(pcc, radius):
    from pcc_amd.pcqm import surface_variation
    xyz = inputs()[0]
    want, valid = ref.surface_variation(xyz, radius)
    got = surface_variation(_coords(xyz), radius).cpu().numpy()
    assert got.dtype == np.float64 and valid.any()
    assert not got[~valid].any()
    assert (got >= 0).all() and (got <= 1 / 3 + 1e-12).all()
    err = np.abs(got - want).max()
    print("kappa r=%d: %d valid of %d, max |kappa - eigvalsh| %.3g, kappa max %.4f" % (radius, valid.sum(), len(xyz), err, got.max()))
    assert err <= 1e-12


@pytest.mark.gpu
def test_surface_variation_validity_equals_the_reference(pcc):
    """a sparse random cloud has isolated, paired and collinear neighbourhoods: kappa is 0 exactly there"""
    from pcc_amd.pcqm import surface_variation
    xyz = ref.nref.random_cloud()
    want, valid = ref.surface_variation(xyz, 2)
    got = surface_variation(_coords(xyz), 2).cpu().numpy()
    assert (~valid).any() and valid.any()
    assert not got[~valid].any()
    assert np.array_equal(got > 1e-9, want > 1e-9) and (got[valid] > 1e-9).any()      # integer moments: l0 is 0 or far from it
    assert np.abs(got - want).max() <= 1e-12


@functools.lru_cache(maxsize=None)
def _bounds(h):
    """per row and statistic: count * 2^-52 * (sum w |x|, or sum w x^2 of the shifted values), plus the longdouble
    restatement's own error, count * eps(longdouble) * the same sums over the attributes as they are (it does not shift)"""
    r_xyz, ar, d_xyz, ad, nn = inputs()
    w_k = ref.gaussian_weights(h)
    rows_r, d2 = ref.neighbour_rows(r_xyz, r_xyz, h)
    rows_d, _ = ref.neighbour_rows(d_xyz[nn], d_xyz, h)
    w = w_k[d2]
    wr, wd = np.where(rows_r >= 0, w[None, :], 0.0), np.where(rows_d >= 0, w[None, :], 0.0)
    cnt_r, cnt_d = (rows_r >= 0).sum(1), (rows_d >= 0).sum(1)
    at_r, at_d = np.maximum(rows_r, 0), np.maximum(rows_d, 0)
    bound = np.empty((len(r_xyz), ref.N_STATS))
    bound[:, 0], bound[:, 1] = cnt_r * ULP * wr.sum(1), cnt_d * ULP * wd.sum(1)
    second = {}
    for ch in range(5):
        xr, xd = ar[:, ch][at_r], ad[:, ch][at_d]
        bound[:, 2 + ch], bound[:, 7 + ch] = cnt_r * ULP * (wr * np.abs(xr)).sum(1), cnt_d * ULP * (wd * np.abs(xd)).sum(1)
        if ch in (0, 4):
            u, v = xr - ar[:, ch][:, None], xd - ad[nn, ch][:, None]
            y = ad[:, ch][nn][at_r]
            paired = y - ad[nn, ch][:, None]
            second[ch] = ((wr * u * u).sum(1), (wd * v * v).sum(1), (wr * paired * paired).sum(1),
                          (wr * xr * xr).sum(1), (wd * xd * xd).sum(1), (wr * y * y).sum(1))
            # the restatement centres the paired values on the D-side mean nu: its factors have magnitude |y| + |nu|, and
            # sum w (|y| + |nu|)^2 <= 2 (sum w y^2 + nu^2 sum w)
            nu = (wd * xd).sum(1) / wd.sum(1)
            second[ch] = second[ch][:5] + (2.0 * (second[ch][5] + nu * nu * wr.sum(1)),)
    for at, ch in ((12, 0), (15, 4)):
        uu, vv, pp, xx, dd, yy = second[ch]
        bound[:, at], bound[:, at + 1], bound[:, at + 2] = cnt_r * ULP * uu, cnt_d * ULP * vv, cnt_r * ULP * np.sqrt(uu * pp)
        bound[:, at] += cnt_r * EPS_LD * xx
        bound[:, at + 1] += cnt_d * EPS_LD * dd
        bound[:, at + 2] += cnt_r * EPS_LD * np.sqrt(xx * yy)
    return bound


@pytest.mark.gpu
@pytest.mark.parametrize("h", [1, 2, 3, 8])
def test_statistics_match_the_restatement(pcc, h):
    assert EPS_LD < ULP / 1000, "numpy.longdouble is no wider than float64 on this host: the kernel's rounding cannot be told from the restatement's"
    stats = gpu(h)[0]
    want = restated(h, np.longdouble)
    assert stats.shape == want.shape == (len(inputs()[0]), 18) and np.isfinite(stats).all()
    worst = _ratio_to_bound(stats, want, _bounds(h)).max(0)
    print("h=%d: largest |stats - restatement| / bound per column: %s" % (h, " ".join("%.3f" % r for r in worst)))
    assert worst.max() <= 1.0
    # the float64 restatement, for the record: its own two-pass rounding (a mean of magnitude |x| subtracted from every value)
    # is what the longdouble evaluation takes out of the comparison
    loose = _ratio_to_bound(stats, restated(h), _bounds(h)).max(0)
    print("h=%d: the same against the float64 restatement (not asserted): %s" % (h, " ".join("%.3g" % r for r in loose)))


def _ratio_to_bound(stats, want, bound):
    diff = np.abs(stats.astype(np.longdouble) - want).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("h", [1, 2, 3, 8])
def test_features_follow_from_the_kernels_own_statistics(pcc, h):
    stats, features, _ = gpu(h)
    want = ref.features(stats, *CONSTS)
    err = np.abs(features - want).max()
    print("h=%d: max |features - formulas(stats)| = %.3g (%.2f ulp of 1.0)" % (h, err, err / ULP))
    assert features.shape == (len(stats), 8)
    assert err <= 4 * ULP


@pytest.mark.gpu
@pytest.mark.parametrize("h", [2, 3])
def test_features_match_the_restatement_end_to_end(pcc, h):
    features = gpu(h)[1]
    f64 = ref.features(restated(h), *CONSTS)
    f80 = ref.features(restated(h, np.longdouble), *CONSTS)
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("numpy.longdouble is no wider than float64 on this host: the restatement's own error cannot be measured")
    e = float(np.abs(f64.astype(np.longdouble) - f80).max())
    got = float(np.abs(features - f64).max())
    print("h=%d: restatement float64 vs longdouble e = %.3g, kernel vs float64 restatement %.3g (%.2f e)" % (h, e, got, got / e))
    assert e > 0
    assert got <= 8 * e


@pytest.mark.gpu
@pytest.mark.parametrize("h", [2, 8])
def test_pooled_sums(pcc, h):
    _, features, sums = gpu(h)
    n = len(features)
    for i in range(8):
        want = math.fsum(features[:, i])
        assert abs(sums[i] - want) <= n * 2.0 ** -53 * math.fsum(np.abs(features[:, i])), (i, sums[i], want)
    assert (sums > 0).all()


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal(pcc):
    again = run_features(*inputs(), 3)
    for a, b in zip(gpu(3), again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_identical_clouds_score_exactly_zero(pcc):
    from pcc_amd import pcqm_voxel
    R, _ = ref.shell_pair()
    x = torch.from_numpy(R).to(DEV)
    for kw in ({}, {"radius": 2, "neighbourhood": 3}):
        out = pcqm_voxel(x, x.clone(), return_features=True, **kw)
        assert out["pcqm_voxel"] == 0.0
        assert all(out["pcqm_f%d" % i] == 0.0 for i in range(1, 9))
        assert out["features"].shape == (len(R), 8) and not out["features"].any()
    assert (out["radius"], out["neighbourhood"]) == (2, 3)


@pytest.mark.gpu
def test_centre_only_weight_table(pcc):
    """w = 1 at d2 = 0 and 0 elsewhere: every mean is the centre's own attribute, every variance and cross term 0"""
    r_xyz, ar, d_xyz, ad, nn = inputs()
    w = np.zeros(10)
    w[0] = 1.0
    stats, features, _ = run_features(r_xyz, ar, d_xyz, ad, nn, 3, w=w)
    assert not features[:, [1, 2, 6, 7]].any()
    a, b = ar[:, 0], ad[nn, 0]
    assert np.array_equal(features[:, 0], np.abs(a - b) / (np.maximum(a, b) + 1.0))
    assert np.array_equal(stats[:, 2:7], ar) and np.array_equal(stats[:, 7:12], ad[nn])
    assert (stats[:, :2] == 1.0).all() and not stats[:, 12:].any()


@pytest.mark.gpu
def test_batch_items_do_not_leak(pcc):
    """a second batch item, the pair shifted by one voxel, leaves the first item's rows bitwise unchanged"""
    r_xyz, ar, d_xyz, ad, nn = inputs()
    n_r, n_d = len(r_xyz), len(d_xyz)
    both_r, both_d = np.concatenate([r_xyz, r_xyz + [1, 0, 0]]), np.concatenate([d_xyz, d_xyz + [1, 0, 0]])
    batch_r = np.concatenate([np.zeros(n_r, np.int64), np.ones(n_r, np.int64)])
    batch_d = np.concatenate([np.zeros(n_d, np.int64), np.ones(n_d, np.int64)])
    stats, features, _ = run_features(both_r, np.concatenate([ar, ar]), both_d, np.concatenate([ad, ad]), np.concatenate([nn, nn + n_d]), 3,
                                      batch_r=batch_r, batch_d=batch_d)
    one_stats, one_features, _ = gpu(3)
    assert stats[:n_r].tobytes() == one_stats.tobytes() and features[:n_r].tobytes() == one_features.tobytes()
    assert stats[n_r:].tobytes() == one_stats.tobytes()


@pytest.mark.gpu
def test_no_rows_zeroes_the_sums(pcc):
    from pcc_amd._lib import ptr
    L = pcc.lib()
    sums = torch.full((8,), 7.0, dtype=torch.float64, device=DEV)
    scratch = torch.empty(64, dtype=torch.uint8, device=DEV)
    consts = (ctypes.c_double * 4)(*CONSTS)
    rc = L.pcc_pcqm_features(None, 0, None, None, 1024, None, 0, None, None, 1024, 1, None, None, None, None, 3, ctypes.addressof(consts), None,
                             None, ptr(sums), ptr(scratch), 64, pcc._lib.stream())
    assert rc == 0
    assert not sums.cpu().numpy().any()


@pytest.mark.gpu
@pytest.mark.parametrize("h", [0, 9])
def test_neighbourhood_out_of_range_raises(pcc, h):
    from pcc_amd._lib import PccError
    with pytest.raises(PccError, match=" h "):
        run_features(*inputs(), h)
