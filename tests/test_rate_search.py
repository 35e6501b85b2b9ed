"""rate_control.bracket_search on stub estimators (pure Python, no GPU): whatever the shape of the estimate — rising, falling,
crossing the target three times, flat — the result is the best probed value that fits the target, within 2 + max_probes
probes, with a log that a second run repeats and ``reached`` telling whether anything fitted."""
import math

import pytest

from pcc_amd.rate_control import bracket_search

STUBS = {
    "increasing": lambda t: int(1000 + 9000 * t),
    "decreasing": lambda t: int(10000 - 9000 * t * t),
    # rises through 5000 near t = 0.04, falls back through it near 0.32, rises through it for good near 0.66
    "three_crossings": lambda t: int(5000 + 4000 * math.sin(3 * math.pi * t) + 3000 * t - 1500),
    "constant": lambda t: 4200,
}


def _run(name, target, max_probes=8, tol=0):
    calls = []

    def estimate(t):
        assert 0.0 <= t <= 1.0
        calls.append(t)
        return STUBS[name](t)

    res = bracket_search(estimate, target, max_probes=max_probes, tol=tol)
    assert [t for t, _ in res.log] == calls and all(e == STUBS[name](t) for t, e in res.log)
    assert len(calls) <= 2 + max_probes and calls[:2] == [0.0, 1.0]
    assert len(set(calls)) == len(calls)                               # no probe is paid for twice
    fits = [(e, -t) for t, e in res.log if e <= target]
    assert res.reached == bool(fits)
    if fits:
        e, neg_t = max(fits)                                           # the largest that fits, ties to the smaller t
        assert (res.estimate, res.t) == (e, -neg_t) and res.estimate <= target
    else:
        assert (res.estimate, res.t) == min((e, t) for t, e in res.log)
    again = bracket_search(STUBS[name], target, max_probes=max_probes, tol=tol)
    assert again.log == res.log and (again.t, again.estimate, again.reached) == (res.t, res.estimate, res.reached)
    return res


@pytest.mark.parametrize("name", ["increasing", "decreasing"])
@pytest.mark.parametrize("target", [1500, 5000, 9999])
def test_monotone_estimates_converge_on_the_target(name, target):
    res = _run(name, target)
    assert res.reached and (len(res.log) == 10 or res.estimate == target)      # (a probe that meets the target ends the search)
    # eight halvings of [0, 1] on a slope of at most 18,000 per unit: within 18000 / 256 below the target
    assert target - 18000 / 256 <= res.estimate <= target
    few = _run(name, target, max_probes=2)
    assert len(few.log) <= 4 and few.reached and few.estimate <= res.estimate


def test_the_bracket_survives_three_crossings():
    f = STUBS["three_crossings"]
    assert f(0.0) < 5000 < f(1.0) and f(0.25) > 5000 > f(0.5)          # the target is crossed three times between the ends
    res = _run("three_crossings", 5000)
    assert res.reached and len(res.log) == 10
    # the invariant "one end <= target < other end" holds without monotonicity: the bracket closes on one of the crossings
    ts = sorted(t for t, _ in res.log)
    at = ts.index(res.t)
    assert any(f(ts[j]) > 5000 for j in (at - 1, at + 1) if 0 <= j < len(ts))
    assert 5000 - 200 <= res.estimate <= 5000


def test_constant_estimate():
    res = _run("constant", 4200)                                       # equal to both ends: fits, no bisection
    assert res.reached and (res.t, res.estimate) == (0.0, 4200) and len(res.log) == 2
    res = _run("constant", 4199)
    assert not res.reached and (res.t, res.estimate) == (0.0, 4200) and len(res.log) == 2
    res = _run("constant", 9000)
    assert res.reached and res.t == 0.0 and len(res.log) == 2


@pytest.mark.parametrize("name", ["increasing", "decreasing", "three_crossings"])
def test_target_outside_the_ends(name):
    f = STUBS[name]
    lo_t, hi_t = (0.0, 1.0) if f(0.0) < f(1.0) else (1.0, 0.0)
    below = _run(name, min(f(0.0), f(1.0)) - 1)                        # below both ends: the cheaper end, not reached
    assert not below.reached and below.t == lo_t and len(below.log) == 2
    above = _run(name, max(f(0.0), f(1.0)) + 1)                        # above both: the dearer end fits
    assert above.reached and above.t == hi_t and len(above.log) == 2


@pytest.mark.parametrize("name", ["increasing", "decreasing"])
def test_target_equal_to_an_end(name):
    f = STUBS[name]
    for t_end in (0.0, 1.0):
        res = _run(name, f(t_end))
        assert res.reached and (res.t, res.estimate) == (t_end, f(t_end)) and len(res.log) == 2


def test_tolerance_stops_early():
    exact = _run("increasing", 5000)
    loose = _run("increasing", 5000, tol=600)
    assert loose.reached and 4400 <= loose.estimate <= 5000 and len(loose.log) < len(exact.log)
    assert _run("increasing", 5000, max_probes=0).log == [(0.0, 1000), (1.0, 10000)]
