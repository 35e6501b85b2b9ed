"""rate_control.compress_to_target on the GPU: the seeded q-responsive model (the FiLM gain tools/rd_sweep.py uses) and the
4,904-point shell, searched between q = (0, 0) and q = (1, 1).

Precondition, checked on the CPU with the kernel-order oracle for this gain (synthetic.FILM_GAIN_Q_RESPONSIVE = 1.0): the two
ends code at different lengths — y + z = 6392 + 92 = 6,484 bytes at t = 0 (q = (0, 0)) and 2908 + 92 = 3,000 bytes at t = 1
(q = (1, 1)); seeded weights spend LESS at higher q, which the search does not mind."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def setup(pcc):
    syn = pcc.synthetic
    model = syn.make_model(0, DEV, film_gain=syn.FILM_GAIN_Q_RESPONSIVE)
    model.update()
    pts = syn.sphere_shell(**syn.CONFIG1)
    x = torch.from_numpy(pts).to(DEV)
    ends = []
    for q in ((0.0, 0.0), (1.0, 1.0)):
        qc, qf = syn.uniform_qmap(pts[:, :3], *q)
        Q = pcc.SparseTensor(coordinates=torch.from_numpy(qc).to(DEV), features=torch.from_numpy(qf).to(DEV), device=DEV)
        ends.append(model.estimate_bits(x, Q)["bytes"][1])
    return model, pts, x, ends


def _canonical(rec):
    rec = rec.cpu().numpy()
    order = np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))
    return rec[order]


def test_the_two_ends_differ(setup):
    model, pts, x, ends = setup
    assert ends[0] != ends[1], ends
    assert abs(ends[0] - 6484) <= 8 and abs(ends[1] - 3000) <= 8, ends      # the oracle's lengths, each within its interval's width


@pytest.mark.parametrize("fraction", [0.25, 0.5, 0.75])
def test_targets_between_the_ends_are_met(pcc, setup, fraction):
    from pcc_amd.rate_control import compress_to_target
    model, pts, x, ends = setup
    target = int(min(ends) + fraction * (max(ends) - min(ends)))
    out = compress_to_target(model, x, target_bytes=target)
    print(f"target {target}: t {out['t']} q {out['q']} estimate {out['estimate']} bytes {out['bytes']} probes {len(out['log'])}")
    assert out["reached"] and out["target_bytes"] == target
    assert out["bytes"] == len(out["strings"][0][0]) + len(out["strings"][1][0]) <= out["estimate"] <= target
    assert len(out["log"]) <= 2 + 8 and out["log"][0][0] == 0.0 and out["log"][1][0] == 1.0
    fits = [(e, -t) for t, e in out["log"] if e <= target]
    assert (out["estimate"], -out["t"]) == max(fits)                        # the best probe of the log, ties to the smaller t
    assert out["q"] == (out["t"], out["t"])                                 # q_lo + t (q_hi - q_lo) on the default ends
    # the strings decode, and equal a plain compress + decompress at the returned (q_g, q_a): byte for byte, voxel for voxel
    rec = model.decompress(coordinates=out["coordinates"], strings=out["strings"], shape=out["shape"], k=out["k"])
    qc, qf = pcc.synthetic.uniform_qmap(pts[:, :3], *out["q"])
    Q = pcc.SparseTensor(coordinates=torch.from_numpy(qc).to(DEV), features=torch.from_numpy(qf).to(DEV), device=DEV)
    strings, shape, k, coords = model.compress(x, Q)
    assert strings == out["strings"] and shape == out["shape"] and k == out["k"] and torch.equal(coords, out["coordinates"])
    plain = model.decompress(coordinates=coords, strings=strings, shape=shape, k=k)
    assert rec.shape[1] == 6 and np.array_equal(_canonical(rec), _canonical(plain))


def test_target_below_both_ends(setup):
    from pcc_amd.rate_control import compress_to_target
    model, pts, x, ends = setup
    out = compress_to_target(model, x, target_bytes=min(ends) - 100)
    assert not out["reached"] and len(out["log"]) == 2
    assert out["t"] == float(ends.index(min(ends))) and out["estimate"] == min(ends)          # the cheaper end
    assert out["bytes"] > out["target_bytes"]


def test_runs_repeat_and_bpp_equals_bytes(setup):
    from pcc_amd.rate_control import compress_to_target
    model, pts, x, ends = setup
    target = (ends[0] + ends[1]) // 2
    a = compress_to_target(model, x, target_bytes=target)
    b = compress_to_target(model, x, target_bytes=target)
    assert a["log"] == b["log"] and a["strings"] == b["strings"] and a["t"] == b["t"]
    n = pts.shape[0]
    c = compress_to_target(model, x, target_bpp=target * 8 / n)              # bits of y + z payload per input point
    assert c["target_bytes"] == target and c["log"] == a["log"] and c["strings"] == a["strings"]
    with pytest.raises(ValueError):
        compress_to_target(model, x)
    with pytest.raises(ValueError):
        compress_to_target(model, x, target_bytes=target, target_bpp=1.0)
