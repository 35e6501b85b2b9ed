"""pcc_raht_plan / pcc_raht_transform (csrc/raht.hip) through the C-ABI, every output buffer pre-filled with a sentinel, against the
numpy restatement (tests/_raht_reference.py, itself checked against the recursive definition on the CPU).  The plan is integer
work and EQUAL to numpy; the coefficients are float64 with the operation order fixed by include/pcc_hip.h and are held to
1e-12 * max|a| * sqrt(N): four correctly rounded operations per step and at most 51 steps on values bounded by max|a| * sqrt(N)
give at most 4 * 51 * 2^-53 = 2.3e-14 of that magnitude, so the bound carries about 40x margin.  Cases: one point, two siblings,
two points that first meet at the top step, the full 2^3 cube, 92 random voxels at depth 3, the 32^3 sphere shell (2.5 k rows: more
than one workgroup and more than one wave per step), 4,000 random voxels at depth 10, 300 voxels at depth 17 with a negative
origin, and a dense 8^3 block without and with two more voxels (a first step of exactly 256 and of 257 rows: the size up to which
the steps at the top share one launch); input rows are shuffled in every case."""
import functools

import numpy as np
import pytest
import torch

import _raht_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7
PLAN_ARRAYS = ("perm", "step", "left", "w0", "w1", "step_rows")
CASES = sorted(ref.cases())


def run_plan(pcc, coords, origin, depth):
    """-> dict of numpy arrays like the restatement's, and the device tensors"""
    from pcc_amd._lib import check, ptr, stream
    L = pcc.lib()
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    n = coords.shape[0]
    c4 = np.concatenate([np.full((n, 1), 5, np.int64), coords], axis=1).astype(np.int32)      # (a batch column that is ignored)
    C = torch.from_numpy(c4).to(DEV)
    dev = {k: torch.full((n + 3,), SENTINEL, dtype=torch.int32, device=DEV) for k in PLAN_ARRAYS}
    offsets = torch.full((3 * depth + 1 + 3,), SENTINEL, dtype=torch.int32, device=DEV)
    status = torch.full((2 + 3,), SENTINEL, dtype=torch.int32, device=DEV)
    nbytes = L.pcc_raht_scratch_bytes(n)
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    o = np.ascontiguousarray(origin, dtype=np.int32)
    check(L.pcc_raht_plan(ptr(C), n, ptr(o), depth, *(ptr(dev[k]) for k in PLAN_ARRAYS), ptr(offsets), ptr(status), ptr(scratch), nbytes,
                          stream()))
    torch.cuda.synchronize()
    # nothing is written behind the arrays
    for k in PLAN_ARRAYS:
        assert bool((dev[k][n:] == SENTINEL).all()), k
    assert bool((offsets[3 * depth + 1:] == SENTINEL).all()) and bool((status[2:] == SENTINEL).all())
    out = {k: dev[k][:n].cpu().numpy() for k in PLAN_ARRAYS}
    out["step_offsets"] = offsets[:3 * depth + 1].cpu().numpy()
    out["status"] = status[:2].cpu().numpy()
    return out, dev


def run_transform(pcc, dev, offsets_host, depth, values, inverse):
    """values [N,C] float64 numpy -> transformed copy; the rows behind the values stay sentinel"""
    from pcc_amd._lib import check, ptr, stream
    n, c = values.shape
    V = torch.full((n + 2, c), float(SENTINEL), dtype=torch.float64, device=DEV)
    V[:n] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(DEV)
    check(pcc.lib().pcc_raht_transform(ptr(V), n, c, ptr(dev["left"]), ptr(dev["w0"]), ptr(dev["w1"]), ptr(dev["step_rows"]),
                                       ptr(np.ascontiguousarray(offsets_host, dtype=np.int32)), depth, inverse, stream()))
    torch.cuda.synchronize()
    assert bool((V[n:] == float(SENTINEL)).all())
    return V[:n].cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference_plan(name):
    coords, origin, depth = ref.cases()[name]
    return ref.plan(coords, origin, depth)


@functools.lru_cache(maxsize=None)
def gpu_plan(name):
    import pcc_amd
    coords, origin, depth = ref.cases()[name]
    want = reference_plan(name)
    o = ref.default_origin_depth(coords)[0] if origin is None else origin
    return run_plan(pcc_amd, coords, o, want["depth"])


@pytest.mark.parametrize("name", CASES)
def test_plan_equals_numpy(pcc, name):
    want = reference_plan(name)
    got, _ = gpu_plan(name)
    assert got["status"].tolist() == [0, 0]
    for k in PLAN_ARRAYS + ("step_offsets",):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("c", (1, 3, 16))
@pytest.mark.parametrize("name", CASES)
def test_transform_against_numpy(pcc, name, c):
    coords, _, _ = ref.cases()[name]
    want = reference_plan(name)
    got, dev = gpu_plan(name)
    n, depth = coords.shape[0], want["depth"]
    a = ref.attributes(n, c, seed=20 + c) * 2.0 - 0.5
    tol = 1e-12 * np.abs(a).max() * np.sqrt(n)
    co_ref = ref.forward(want, a)
    co = run_transform(pcc, dev, got["step_offsets"], depth, a[want["perm"]], 0)
    err = np.abs(co - co_ref).max()
    print(f"{name} C={c}: forward max error {err:.3e} (bound {tol:.3e}), bit-equal {np.array_equal(co, co_ref)}")
    assert err <= tol
    back_ref = ref.inverse(want, co_ref)
    back = run_transform(pcc, dev, got["step_offsets"], depth, co_ref, 1)
    err = np.abs(back - back_ref).max()
    print(f"{name} C={c}: inverse max error {err:.3e}, bit-equal {np.array_equal(back, back_ref)}")
    assert err <= tol
    # two runs: the same bytes
    assert np.array_equal(run_transform(pcc, dev, got["step_offsets"], depth, a[want["perm"]], 0).view(np.uint64), co.view(np.uint64))
    assert np.array_equal(run_transform(pcc, dev, got["step_offsets"], depth, co_ref, 1).view(np.uint64), back.view(np.uint64))


def test_two_plans_are_identical(pcc):
    coords, origin, depth = ref.cases()["shell32"]
    want = reference_plan("shell32")
    o = ref.default_origin_depth(coords)[0]
    a, _ = run_plan(pcc, coords, o, want["depth"])
    b, _ = run_plan(pcc, coords, o, want["depth"])
    for k in PLAN_ARRAYS + ("step_offsets", "status"):
        assert np.array_equal(a[k], b[k]), k


def test_status_reports_duplicates_and_rows_outside(pcc):
    coords = ref.random_voxels(500, 5, 9)
    bad = coords.copy()
    bad[17] = bad[400]                      # one voxel twice
    bad[33] = (32, 0, 0)                    # outside on the high side
    bad[250] = (3, -1, 3)                   # and on the low side
    bad[251] = (2 ** 31 - 1, 0, 0)          # a difference that would wrap in 32 bits with the origin below
    want = ref.plan(bad, (0, 0, 0), 5)
    got, _ = run_plan(pcc, bad, (0, 0, 0), 5)
    assert want["status"].tolist() == [3, 3]           # the three outside rows share key 0: two of them repeat it
    for k in PLAN_ARRAYS + ("step_offsets", "status"):
        assert np.array_equal(got[k], want[k]), k
    got, _ = run_plan(pcc, np.array([[-5, 2 ** 31 - 1, 0], [0, 0, 0]]), (-2 ** 31, 0, 0), 3)
    assert got["status"].tolist() == [2, 1]
    # the Python layer turns either into a ValueError
    from pcc_amd import raht
    for rows, kw in ((bad[[17, 400, 1]], {}), (coords[:50], dict(origin=(1, 0, 0), depth=5)), (coords[:50], dict(depth=2))):
        with pytest.raises(ValueError):
            raht.plan(torch.from_numpy(rows).to(DEV), **kw)
    assert raht.plan(torch.from_numpy(coords).to(DEV)).n == 500


def test_argument_errors(pcc):
    from pcc_amd._lib import PCC, ptr, stream
    L = pcc.lib()
    _, dev = gpu_plan("cube")
    offsets = reference_plan("cube")["step_offsets"]
    V = torch.zeros((8, 17), dtype=torch.float64, device=DEV)
    args = (ptr(dev["left"]), ptr(dev["w0"]), ptr(dev["w1"]), ptr(dev["step_rows"]), ptr(offsets))
    for c in (0, 17):
        assert L.pcc_raht_transform(ptr(V), 8, c, *args, 1, 0, stream()) == PCC.ERR_ARG
        assert b"channels" in L.pcc_last_error()
    assert L.pcc_raht_transform(ptr(V), 8, 3, *args, 1, 2, stream()) == PCC.ERR_ARG
    assert L.pcc_raht_transform(ptr(V), 8, 3, *args, 18, 0, stream()) == PCC.ERR_ARG
    assert L.pcc_raht_transform(ptr(V), 0, 3, *args, 1, 0, stream()) == PCC.ERR_ARG
    assert L.pcc_raht_transform(None, 8, 3, *args, 1, 0, stream()) == PCC.ERR_ARG
    wrong = np.array([0, 4, 3, 7], dtype=np.int32)                      # offsets that do not ascend
    assert L.pcc_raht_transform(ptr(V), 8, 3, *args[:4], ptr(wrong), 1, 0, stream()) == PCC.ERR_ARG
    wrong = np.array([0, 4, 6, 9], dtype=np.int32)                      # or run past the rows
    assert L.pcc_raht_transform(ptr(V), 8, 3, *args[:4], ptr(wrong), 1, 0, stream()) == PCC.ERR_ARG
    assert bool((V == 0).all())
    C = torch.zeros((8, 4), dtype=torch.int32, device=DEV)
    o = np.zeros(3, dtype=np.int32)
    buf = [torch.zeros(8, dtype=torch.int32, device=DEV) for _ in range(8)]
    nbytes = L.pcc_raht_scratch_bytes(8)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    plan_args = lambda n, depth, nb: (ptr(C), n, ptr(o), depth, *(ptr(b) for b in buf), ptr(scratch), nb, stream())
    assert L.pcc_raht_plan(*plan_args(8, 18, nbytes)) == PCC.ERR_ARG and b"depth" in L.pcc_last_error()
    assert L.pcc_raht_plan(*plan_args(0, 1, nbytes)) == PCC.ERR_ARG
    assert L.pcc_raht_plan(*plan_args(8, 1, nbytes - 1)) == PCC.ERR_ARG and b"scratch" in L.pcc_last_error()


def test_python_layer_round_trip(pcc):
    """raht.forward / inverse / encode_attributes / decode_attributes on the shell: the coefficients of the restatement, the
    input back in Morton order, and a stream whose symbols the decoder returns"""
    from pcc_amd import raht
    coords, _, _ = ref.cases()["shell32"]
    want = reference_plan("shell32")
    p = raht.plan(torch.from_numpy(coords).to(DEV))
    assert (p.n, p.depth, p.origin) == (coords.shape[0], want["depth"], tuple(ref.default_origin_depth(coords)[0].tolist()))
    assert np.array_equal(p.step_offsets, want["step_offsets"])
    a = ref.smooth_colours(coords)
    tol = 1e-12 * np.abs(a).max() * np.sqrt(p.n)
    co = raht.forward(p, a)
    assert co.dtype == torch.float64 and np.abs(co.cpu().numpy() - ref.forward(want, a)).max() <= tol
    assert np.abs(raht.inverse(p, co).cpu().numpy() - a[want["perm"]]).max() <= 1e-12
    data, sym = raht.encode_attributes(p, a, 4 / 255, return_symbols=True)
    back, qstep = raht.decode_symbols(p, data)
    assert qstep == 4 / 255 and np.array_equal(back, sym)
    rec = raht.decode_attributes(p, data).cpu().numpy()
    assert ((rec - a[want["perm"]]) ** 2).mean() <= (4 / 255) ** 2 / 4 * (1 + 1e-9)
    with pytest.raises(ValueError):
        raht.decode_attributes(p, data, channels=1)
    with pytest.raises(ValueError):
        raht.encode_attributes(p, a[:-1], 4 / 255)
