"""ColorModel.estimate_bits against the real coder: on the seeded q-responsive model (the FiLM gain tools/rd_sweep.py uses) and
the 4,904-point shell, the lengths of the y and z strings that compress writes lie inside the intervals estimate_bits
proved beforehand — in the reference's stream format and with the lane-parallel y stream, for the two-hyperprior variant and
for a two-item batch.  The intervals are the derived ones (entropy.stream_bytes_interval): 4 bytes wide per stream plus the
operation term, so a probe pins the payload to within a few words."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
QS = [(0.0, 0.0), (0.4, 0.8), (1.0, 1.0)]


@pytest.fixture(scope="module")
def frame(pcc):
    return pcc.synthetic.sphere_shell(**pcc.synthetic.CONFIG1)


def _model(pcc, config=None):
    syn = pcc.synthetic
    m = syn.make_model(0, DEV, config=config, film_gain=syn.FILM_GAIN_Q_RESPONSIVE)
    m.update()
    return m


@pytest.fixture(scope="module")
def model(pcc):
    return _model(pcc)


def _qmap(pcc, pts, q, batch=None):
    qc, qf = pcc.synthetic.uniform_qmap(pts[:, :3], *q)
    if batch is not None:
        qc[:, 0] = batch
    return pcc.SparseTensor(coordinates=torch.from_numpy(qc).to(DEV), features=torch.from_numpy(qf).to(DEV), device=DEV,
                            nbatch=None if batch is None else int(batch.max()) + 1)


def _inside(interval, length):
    return interval[0] <= length <= interval[1]


def _check_widths(est, n_sym_y, lanes, pairs=1):
    """the y interval is 4 bytes per stream wide plus one word per 2^21 / (2 * 3.386) = 309,679 operations (every frame here has
    fewer: no such word); the z interval 4 bytes per model"""
    streams = min(lanes, n_sym_y) if lanes else 1
    assert est["y"][1] - est["y"][0] <= 4 * streams * pairs
    assert est["z"][1] - est["z"][0] <= 4 * pairs
    assert est["bytes"] == (est["y"][0] + est["z"][0], est["y"][1] + est["z"][1])


@pytest.mark.parametrize("lanes", [0, 64])
@pytest.mark.parametrize("q", QS)
def test_stream_lengths_lie_in_the_estimated_intervals(pcc, model, frame, q, lanes):
    from pcc_amd import entropy as E
    x = torch.from_numpy(frame).to(DEV)
    E.set_stream_lanes(lanes)
    try:
        est = model.estimate_bits(x, _qmap(pcc, frame, q))
        strings, shape, k, coords = model.compress(x, _qmap(pcc, frame, q))
    finally:
        E.set_stream_lanes(0)
    ly, lz = len(strings[0][0]), len(strings[1][0])
    print(f"q {q} lanes {lanes}: y {ly} in {est['y']}, z {lz} in {est['z']}, escapes {est['escapes']}")
    assert _inside(est["y"], ly) and _inside(est["z"], lz) and _inside(est["bytes"], ly + lz)
    assert est["n_points"] == frame.shape[0] and est["escapes"] >= 0
    _check_widths(est, coords.shape[0] * 128, lanes)
    if lanes:
        assert strings[0][0][:4] == b"PCL1"


def test_estimate_first_leaves_the_bytes_unchanged(pcc, model, frame):
    x = torch.from_numpy(frame).to(DEV)
    q = QS[1]
    before = model.compress(x, _qmap(pcc, frame, q))
    est = model.estimate_bits(x, _qmap(pcc, frame, q))
    after = model.compress(x, _qmap(pcc, frame, q))
    assert before[0] == after[0] and before[1:3] == after[1:3] and torch.equal(before[3], after[3])
    assert est == model.estimate_bits(x, _qmap(pcc, frame, q))                     # and a probe repeats itself exactly
    fresh = _model(pcc)                                                            # a model that never estimated codes the same bytes
    assert fresh.compress(x, _qmap(pcc, frame, q))[0] == after[0]


def test_the_rate_follows_the_quality_map(pcc, model, frame):
    x = torch.from_numpy(frame).to(DEV)
    ends = [model.estimate_bits(x, _qmap(pcc, frame, q))["bytes"] for q in (QS[0], QS[2])]
    assert ends[0][0] > ends[1][1] or ends[1][0] > ends[0][1]                      # disjoint intervals: the two ends differ


@pytest.mark.parametrize("lanes", [0, 64])
def test_two_hyperprior_variant_sums_both_models(pcc, frame, lanes):
    from pcc_amd import entropy as E
    model = _model(pcc, pcc.synthetic.TWO_HYPERPRIOR_CONFIG)
    x = torch.from_numpy(frame).to(DEV)
    for q in QS:
        E.set_stream_lanes(lanes)
        try:
            est = model.estimate_bits(x, _qmap(pcc, frame, q))
            strings, shape, k, coords = model.compress(x, _qmap(pcc, frame, q))
        finally:
            E.set_stream_lanes(0)
        (y_main, z_main), (y_map, z_map) = strings
        ly, lz = len(y_main[0]) + len(y_map[0]), len(z_main[0]) + len(z_map[0])
        assert _inside(est["y"], ly) and _inside(est["z"], lz) and _inside(est["bytes"], ly + lz), (q, est, ly, lz)
        _check_widths(est, coords.shape[0] * 2, lanes, pairs=2)


@pytest.mark.parametrize("lanes", [0, 64])
def test_two_item_batch(pcc, model, frame, lanes):
    from pcc_amd import entropy as E
    other = pcc.synthetic.sphere_shell(grid=32, radius=12.0, half_width=0.875)
    pts = np.concatenate([frame, other], axis=0)
    batch = np.concatenate([np.zeros(frame.shape[0], np.int32), np.ones(other.shape[0], np.int32)])
    x, bt = torch.from_numpy(pts).to(DEV), torch.from_numpy(batch).to(DEV)
    E.set_stream_lanes(lanes)
    try:
        est = model.estimate_bits(x, _qmap(pcc, pts, QS[1], batch), batch=bt)
        strings, shape, k, coords = model.compress(x, _qmap(pcc, pts, QS[1], batch), batch=bt)
    finally:
        E.set_stream_lanes(0)
    ly, lz = len(strings[0][0]), len(strings[1][0])
    assert _inside(est["y"], ly) and _inside(est["z"], lz) and est["n_points"] == pts.shape[0]
    _check_widths(est, coords.shape[0] * 128, lanes)
    single = model.estimate_bits(torch.from_numpy(frame).to(DEV), _qmap(pcc, frame, QS[1]))
    assert est["bytes"][0] > single["bytes"][1]                                    # the second item costs something
