"""pcc_chconv (csrc/chconv.hip), per launch, through the C-ABI: the channelwise window convolution and its adjoint.

The operator is linear, so it is held to EQUALITY with a float64 numpy evaluation on operand families whose sums are exact
in any order (small integer features, dyadic windows), for both flips, over every window size, the channel counts and row
counts at which the kernel's lane mapping changes, and geometries that exercise absent neighbours, the key range, tensor
strides and batch items.  An asymmetric window catches a wrong flip or axis order.  On the loss's own Gaussian window the
result lies within the bound of any-order fp32 summation of rounded products.
"""
import functools

import numpy as np
import pytest
import torch

DEV = "cuda:0"
COORD_LIMIT = 130000


# ---------------------------------------------------------------------------------------------
# geometries: name -> (coords int32 [n, 4] in shuffled row order, tensor stride)
# ---------------------------------------------------------------------------------------------
def _rows(xyz, b=0):
    xyz = np.asarray(xyz).reshape(-1, 3)
    return np.concatenate([np.full((xyz.shape[0], 1), b), xyz], axis=1).astype(np.int32)


def _block(n, origin=(0, 0, 0)):
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    return g + np.asarray(origin)


def _scatter(grid, frac, rng):
    g = _block(grid)
    return g[rng.random(g.shape[0]) < frac]


@functools.lru_cache(maxsize=None)
def geometry(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    ts = 1
    if name == "block14":                                    # full 11^3 windows in the middle
        c = _rows(_block(14))
    elif name == "shell":                                    # thickness 2, about 5 k rows
        g = _block(24)
        c = _rows(g[((g < 2) | (g >= 22)).any(axis=1)])
    elif name.startswith("line_z"):                          # line_z63 / 64 / 65 / 257
        n = int(name[6:])
        c = _rows(np.stack([np.full(n, 3), np.full(n, -2), np.arange(n)], 1))
    elif name == "line_x":
        c = _rows(np.stack([np.arange(257), np.full(257, 5), np.full(257, 7)], 1))
    elif name == "plane_z":
        g = _block(20)
        c = _rows(g[g[:, 2] == 9])
    elif name == "scattered":                                # 2 % of 40^3: mostly empty windows
        c = _rows(_scatter(40, 0.02, rng))
    elif name == "negative":
        c = _rows(np.concatenate([_block(6, (-50, -60, -70)), _scatter(16, 0.2, rng) - 20]))
        c = np.unique(c, axis=0)
    elif name == "far":                                      # window 11 at the edge of the key range: probes past it are absent
        c = _rows([(COORD_LIMIT, 0, 0), (COORD_LIMIT - 2, 0, 1), (COORD_LIMIT - 4, 1, 0), (-COORD_LIMIT, 0, 0), (-COORD_LIMIT + 3, 0, 0),
                   (0, COORD_LIMIT, -COORD_LIMIT), (1, COORD_LIMIT - 1, -COORD_LIMIT + 2)])
    elif name == "far512":
        # stride 512: the probe at +5 steps from +-COORD_LIMIT leaves the key's 18-bit field, and the voxel its WRAPPED key
        # would name (130000 + 2560 - 2^18 = -129584) is in the set: a probe that wraps instead of being absent finds it
        a = 2 ** 18 - COORD_LIMIT - 5 * 512
        c = _rows([(COORD_LIMIT, 0, 0), (-a, 0, 0), (0, -COORD_LIMIT, 0), (0, a, 0), (0, 0, COORD_LIMIT), (0, 0, -a)])
        ts = 512
    elif name == "stride2":
        c = _rows(_scatter(12, 0.3, rng) * 2 - 6)
        ts = 2
    elif name == "two_items":                                # identical coordinates in two batch items
        g = _scatter(10, 0.3, rng)
        c = np.concatenate([_rows(g, 0), _rows(g, 1)])
    elif name == "single":
        c = _rows([(4, -4, 4)])
    elif name == "big":                                      # about 40 k rows
        c = _rows(_scatter(44, 0.5, rng))
    else:
        raise KeyError(name)
    return c[rng.permutation(c.shape[0])].copy(), ts


# ---------------------------------------------------------------------------------------------
# float64 reference: sorted keys, one searchsorted per offset
# ---------------------------------------------------------------------------------------------
_R = 1 << 19


def _key(c):
    c = c.astype(np.int64)
    return ((c[:, 0] * _R + (c[:, 1] + _R // 2)) * _R + (c[:, 2] + _R // 2)) * _R + (c[:, 3] + _R // 2)


def reference(coords, x, w, ksize, ts, flip):
    """-> (y float64 [n, c], present neighbours per row, sum |w x| per element)"""
    n, c = x.shape
    keys = _key(coords)
    order = np.argsort(keys)
    skeys = keys[order]
    assert np.all(np.diff(skeys) > 0), "duplicate coordinates in a test geometry"
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    y, mag, cnt = np.zeros((n, c)), np.zeros((n, c)), np.zeros(n, dtype=np.int64)
    h, K = ksize // 2, ksize ** 3
    for k in range(K):
        d = np.array([0, k % ksize - h, (k // ksize) % ksize - h, k // (ksize * ksize) - h]) * ts
        q = coords.astype(np.int64) + d
        ok = (np.abs(q[:, 1:]) <= COORD_LIMIT).all(axis=1)
        qk = _key(q)
        pos = np.minimum(np.searchsorted(skeys, qk), n - 1)
        ok &= skeys[pos] == qk
        src = order[pos[ok]]
        wk = w64[K - 1 - k if flip else k]                    # [1] or [c]: broadcasts
        y[ok] += wk * x64[src]
        mag[ok] += np.abs(wk * x64[src])
        cnt[ok] += 1
    return y, cnt, mag


def dyadic_window(ksize, channels):
    """w[k, ch] = 2^-(((3 ix + 5 iy + 7 iz) mod 4) + ch mod 3): asymmetric under reversal and under any swap of axes"""
    k = np.arange(ksize ** 3)
    ix, iy, iz = k % ksize, (k // ksize) % ksize, k // (ksize * ksize)
    e = (3 * ix + 5 * iy + 7 * iz) % 4
    return (2.0 ** -(e[:, None] + (np.arange(channels) % 3)[None, :])).astype(np.float32)


def exact_case(geom, ksize, c, per_channel, seed=0):
    coords, ts = geometry(geom)
    rng = np.random.default_rng(seed + 17 * ksize + c)
    x = rng.integers(-3, 4, (coords.shape[0], c)).astype(np.float32)
    w = dyadic_window(ksize, c if per_channel else 1)
    return coords, ts, x, w


def launch(pcc, cmap, x, w, ksize, flip, y=None):
    L = pcc.lib()
    keys, vals, cap = cmap.table()
    n, c = x.shape
    if y is None:
        y = torch.full((n, c), float("nan"), dtype=torch.float32, device=DEV)
    rc = L.pcc_chconv(x.data_ptr(), n, c, cmap.coords.data_ptr(), keys.data_ptr(), vals.data_ptr(), cap, cmap.stride, ksize,
                      w.data_ptr(), w.shape[1], flip, y.data_ptr(), None)
    assert rc == 0, L.pcc_last_error()
    return y


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# (geometry, window, channels, per-channel window): every window size, channel count, w_channels and row count of the family
EXACT = [
    ("block14", 11, 32, False), ("block14", 11, 32, True), ("block14", 9, 30, True), ("block14", 7, 3, False),
    ("shell", 5, 32, True), ("shell", 11, 1, False), ("shell", 3, 30, False),
    ("line_z63", 7, 32, False), ("line_z64", 5, 3, True), ("line_z65", 11, 30, True), ("line_z257", 9, 1, True),
    ("line_x", 11, 32, True), ("plane_z", 9, 32, False), ("scattered", 11, 30, False), ("scattered", 3, 1, False),
    ("negative", 7, 32, True), ("far", 11, 32, False), ("far", 11, 3, True), ("far512", 11, 32, True),
    ("stride2", 5, 32, True), ("stride2", 3, 30, False),
    ("two_items", 7, 32, False), ("single", 11, 32, True), ("single", 1, 1, False), ("block14", 1, 32, True),
    ("big", 3, 30, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("geom,ksize,c,per_channel", EXACT)
def test_exact_family_equals_float64_for_both_flips(pcc, geom, ksize, c, per_channel):
    coords, ts, x, w = exact_case(geom, ksize, c, per_channel)
    cmap = pcc.CoordMap(dev(coords), ts)
    xd, wd = dev(x), dev(w)
    for flip in (0, 1):
        want, cnt, _ = reference(coords, x, w, ksize, ts, flip)
        # exactness: |products| <= 3 on a grid of 2^-5, so every partial sum is an integer below 2^24 in grid units
        assert int(cnt.max()) * 3 * 32 < 2 ** 24
        got = launch(pcc, cmap, xd, wd, ksize, flip).cpu().numpy().astype(np.float64)
        assert np.array_equal(got, want), (geom, ksize, c, per_channel, flip, float(np.abs(got - want).max()))
    if geom == "far512":
        assert cnt.max() == 1                                # every voxel is alone: the wrapped aliases are not neighbours
    if geom == "block14" and ksize == 11:
        assert cnt.max() == 11 ** 3


@pytest.mark.gpu
def test_batch_items_do_not_mix(pcc):
    """identical coordinates in two batch items: each item's result is that of the item alone"""
    coords, ts, x, w = exact_case("two_items", 5, 32, True)
    got = launch(pcc, pcc.CoordMap(dev(coords), ts), dev(x), dev(w), 5, 0).cpu().numpy()
    for b in (0, 1):
        sel = coords[:, 0] == b
        alone = coords[sel].copy()
        alone[:, 0] = 0
        want, _, _ = reference(alone, x[sel], w, 5, ts, 0)
        assert np.array_equal(got[sel].astype(np.float64), want)


@pytest.mark.gpu
@pytest.mark.parametrize("geom,ksize,c", [("shell", 7, 32), ("scattered", 11, 30), ("stride2", 5, 3)])
def test_adjoint_identity_is_exact(pcc, geom, ksize, c):
    coords, ts, x, w = exact_case(geom, ksize, c, True)
    dy = np.random.default_rng(5).integers(-3, 4, x.shape).astype(np.float32)
    cmap = pcc.CoordMap(dev(coords), ts)
    fwd = launch(pcc, cmap, dev(x), dev(w), ksize, 0).cpu().numpy().astype(np.float64)
    adj = launch(pcc, cmap, dev(dy), dev(w), ksize, 1).cpu().numpy().astype(np.float64)
    assert float((dy.astype(np.float64) * fwd).sum()) == float((adj * x.astype(np.float64)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("ksize", [3, 5, 7, 9, 11])
@pytest.mark.parametrize("geom", ["block14", "scattered"])
def test_gaussian_window_within_the_summation_bound(pcc, geom, ksize):
    """the loss's own window on uniform random features: any-order fp32 summation of n rounded products is within
    (n + 2) 2^-24 sum |w x| of the exact sum to first order (n - 1 adds, one product rounding, one for the slack of the
    first-order bound); 1.01 covers the higher-order terms"""
    from pcc_amd.loss import gaussian_window_3d
    coords, ts = geometry(geom)
    x = np.random.default_rng(ksize).random((coords.shape[0], 32)).astype(np.float32)
    w = gaussian_window_3d(ksize).numpy()
    assert w.shape == (ksize ** 3, 1) and w.dtype == np.float32
    cmap = pcc.CoordMap(dev(coords), ts)
    for flip in (0, 1):
        want, cnt, mag = reference(coords, x, w, ksize, ts, flip)
        got = launch(pcc, cmap, dev(x), dev(w), ksize, flip).cpu().numpy().astype(np.float64)
        bound = 1.01 * (cnt[:, None] + 2) * 2.0 ** -24 * mag
        worst = float((np.abs(got - want) / bound).max())
        print(f"{geom} window {ksize} flip {flip}: worst error / bound = {worst:.3f}")
        assert np.all(np.abs(got - want) <= bound), worst


@pytest.mark.gpu
def test_two_launches_are_bit_equal(pcc):
    coords, ts = geometry("shell")
    x = np.random.default_rng(1).standard_normal((coords.shape[0], 32)).astype(np.float32)
    w = np.random.default_rng(2).standard_normal((7 ** 3, 32)).astype(np.float32)
    cmap = pcc.CoordMap(dev(coords), ts)
    a = launch(pcc, cmap, dev(x), dev(w), 7, 0)
    b = launch(pcc, cmap, dev(x), dev(w), 7, 0)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.gpu
def test_refusals_touch_nothing(pcc):
    L = pcc.lib()
    coords, ts, x, w = exact_case("plane_z", 3, 3, True)
    cmap = pcc.CoordMap(dev(coords), ts)
    keys, vals, cap = cmap.table()
    n = coords.shape[0]
    xd, w3 = dev(x), dev(w)
    x33 = torch.zeros((n, 33), dtype=torch.float32, device=DEV)
    w_big = torch.ones((13 ** 3, 33), dtype=torch.float32, device=DEV)
    guard = 64
    buf = torch.full((n * 33 + 2 * guard,), -77.0, dtype=torch.float32, device=DEV)
    y = buf[guard:]
    ARG, UNSUPPORTED = -1, -3

    def call(x_=xd, c=3, ksize=3, w_=w3, wc=3, flip=0, y_=y, cap_=cap, n_=n, ts_=ts):
        return L.pcc_chconv(None if x_ is None else x_.data_ptr(), n_, c, cmap.coords.data_ptr(), keys.data_ptr(), vals.data_ptr(),
                            cap_, ts_, ksize, None if w_ is None else w_.data_ptr(), wc, flip, None if y_ is None else y_.data_ptr(), None)

    refused = [
        (dict(ksize=2), UNSUPPORTED), (dict(ksize=4), UNSUPPORTED), (dict(ksize=0), UNSUPPORTED), (dict(ksize=-3), UNSUPPORTED),
        (dict(ksize=13, w_=w_big), UNSUPPORTED), (dict(c=33, x_=x33, w_=w_big, wc=33), UNSUPPORTED), (dict(c=0), UNSUPPORTED),
        (dict(wc=2), ARG), (dict(wc=0), ARG), (dict(x_=None), ARG), (dict(w_=None), ARG), (dict(y_=None), ARG), (dict(flip=2), ARG),
        (dict(cap_=cap - 1), ARG), (dict(n_=-1), ARG), (dict(ts_=0), ARG),
    ]
    for kwargs, code in refused:
        rc = call(**kwargs)
        assert rc == code, (kwargs.keys(), rc)
        assert b"pcc_chconv" in L.pcc_last_error()
    torch.cuda.synchronize()
    assert bool((buf == -77.0).all())
    assert call(n_=0) == 0 and call(n_=0, x_=None, y_=None) == 0         # nothing to do: success, nothing launched
    torch.cuda.synchronize()
    assert bool((buf == -77.0).all())
    assert call() == 0                                                   # the same arguments, unrefused, do write
    torch.cuda.synchronize()
    assert bool((buf[:guard] == -77.0).all()) and bool((buf[guard + n * 3:] == -77.0).all()) and bool((y[:n * 3] != -77.0).any())


@pytest.mark.gpu
def test_python_class_forward_backward_and_broadcast(pcc):
    coords, ts, x, w = exact_case("shell", 5, 30, True)
    dy = np.random.default_rng(9).integers(-3, 4, x.shape).astype(np.float32)
    cmap = pcc.CoordMap(dev(coords), ts)
    conv = pcc.MinkowskiChannelwiseConvolution(in_channels=30, kernel_size=5, stride=1, dimension=3)
    assert tuple(conv.kernel.shape) == (125, 30)
    conv.kernel = torch.nn.Parameter(dev(w), requires_grad=False)
    xt = dev(x).requires_grad_(True)
    out = conv(pcc.SparseTensor(xt, coordinate_map=cmap))
    assert out.map is cmap
    (gx,) = torch.autograd.grad(out.F, xt, dev(dy))
    want, _, _ = reference(coords, x, w, 5, ts, 0)
    want_g, _, _ = reference(coords, dy, w, 5, ts, 1)
    assert np.array_equal(out.F.detach().cpu().numpy().astype(np.float64), want)
    assert np.array_equal(gx.cpu().numpy().astype(np.float64), want_g)
    # [K, 1] broadcasts over the channels: the same bits as the [K, C] kernel with repeated columns
    w1 = dyadic_window(5, 1) * np.float32(0.3)
    xr = dev(np.random.default_rng(3).standard_normal(x.shape).astype(np.float32))
    with torch.no_grad():
        conv.kernel = torch.nn.Parameter(dev(w1), requires_grad=False)
        a = conv(pcc.SparseTensor(xr, coordinate_map=cmap)).F
        conv.kernel = torch.nn.Parameter(dev(np.repeat(w1, 30, axis=1)), requires_grad=False)
        b = conv(pcc.SparseTensor(xr, coordinate_map=cmap)).F
    assert torch.equal(a, b)
    # a kernel that wants a gradient is refused while autograd tracks (the kernel gradient is not built)
    conv.kernel = torch.nn.Parameter(dev(w1), requires_grad=True)
    with pytest.raises(NotImplementedError):
        conv(pcc.SparseTensor(xr, coordinate_map=cmap))


def test_python_class_refuses_what_is_not_built(pcc):
    for kwargs in (dict(stride=2), dict(dilation=2), dict(bias=True), dict(kernel_size=4), dict(kernel_size=13)):
        with pytest.raises(NotImplementedError):
            pcc.MinkowskiChannelwiseConvolution(**{"in_channels": 30, "kernel_size": 5, **kwargs})
    conv = pcc.MinkowskiChannelwiseConvolution(in_channels=30, kernel_size=5)
    assert tuple(conv.kernel.shape) == (125, 30) and isinstance(conv.kernel, torch.nn.Parameter)


def test_reference_evaluation_checks_itself():
    """the float64 yardstick against a direct double loop on a tiny set (no GPU)"""
    coords, ts = geometry("stride2")
    coords = coords[:40]
    x = np.random.default_rng(0).integers(-3, 4, (coords.shape[0], 2)).astype(np.float32)
    w = dyadic_window(3, 2)
    for flip in (0, 1):
        y, cnt, _ = reference(coords, x, w, 3, ts, flip)
        want = np.zeros_like(y)
        present = np.zeros(coords.shape[0], dtype=int)
        for i, ci in enumerate(coords):
            for j, cj in enumerate(coords):
                d = (cj[1:] - ci[1:]) // ts
                if cj[0] == ci[0] and np.all(np.abs(d) <= 1):
                    k = (d[0] + 1) + 3 * (d[1] + 1) + 9 * (d[2] + 1)
                    want[i] += w[26 - k if flip else k].astype(np.float64) * x[j]
                    present[i] += 1
        assert np.array_equal(y, want) and np.array_equal(cnt, present)
