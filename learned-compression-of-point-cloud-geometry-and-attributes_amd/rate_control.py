"""Target-rate coding: "code this frame into at most B bytes" (DESIGN.md "Target-rate coding").

The rate of the codec is steered by the quality map ``Q = [q_g, q_a]``.  ``ColorModel.estimate_bits`` tells what a map would
cost without running the coder — an interval the real stream length is proven to lie in — so a search over a scalar
``t in [0, 1]`` that moves the map from ``q_lo`` to ``q_hi`` costs a handful of probes and ONE real ``compress`` at the end.
The search runs on the upper end of the interval: a probe that fits the target is a map whose stream fits it.
"""
import torch

from .q_map import uniform_map
from .sparse import CoordMap


class SearchResult:
    """``t``: the chosen position; ``estimate``: its estimate; ``reached``: whether that estimate is <= the target; ``log``: every
    probe as ``(t, estimate)`` in the order it was made."""
    __slots__ = ("t", "estimate", "reached", "log")

    def __init__(self, t, estimate, reached, log):
        self.t, self.estimate, self.reached, self.log = t, estimate, reached, log

    def __repr__(self):
        return f"SearchResult(t={self.t!r}, estimate={self.estimate!r}, reached={self.reached!r}, probes={len(self.log)})"


def bracket_search(estimate, target, max_probes=8, tol=0):
    """Find ``t in [0, 1]`` whose ``estimate(t)`` (an int: the upper end of a byte interval) is as large as possible without
    exceeding ``target``.

    ``t = 0`` and ``t = 1`` are probed first.  A target outside [min, max] of the two returns the nearer end: the cheaper one
    with ``reached=False`` when even that is above the target, the dearer one (which fits) when the target is above both.
    Otherwise the bracket is bisected, keeping "one end <= target < other end": that needs no monotonicity of ``estimate``
    (seeded and untrained weights give none), only the two ends it already holds.  It stops after ``max_probes`` bisection
    steps, or as soon as a probe lands within ``tol`` below the target (target - tol <= estimate <= target).

    Returns a SearchResult: among ALL probed ``t`` the one with the largest estimate <= target, ties to the smaller ``t``, and
    the full probe log.  At most ``2 + max_probes`` calls of ``estimate``; no randomness: the same estimator gives the same log.
    """
    log = []

    def probe(t):
        e = int(estimate(t))
        log.append((t, e))
        return e

    def best():
        fit = [(-e, t) for t, e in log if e <= target]
        if fit:
            e, t = min(fit)
            return SearchResult(t, -e, True, log)
        e, t = min((e, t) for t, e in log)          # nothing fits: the cheapest probe
        return SearchResult(t, e, False, log)

    e0, e1 = probe(0.0), probe(1.0)
    if target < min(e0, e1) or target >= max(e0, e1):
        return best()
    # (below, above): estimate(below) <= target < estimate(above)
    below, above = (0.0, 1.0) if e0 <= target else (1.0, 0.0)
    near = lambda e: target - tol <= e <= target
    if near(e0) or near(e1):
        return best()
    for _ in range(int(max_probes)):
        mid = (below + above) / 2
        if mid == below or mid == above:
            break
        e = probe(mid)
        if e <= target:
            below = mid
            if near(e):
                break
        else:
            above = mid
    return best()


def _payload(strings):
    """the bytes of every string of a compress result (one [y, z] pair, or one pair per model in the two-hyperprior variant)"""
    total = 0
    for s in strings:
        total += len(s) if isinstance(s, (bytes, bytearray)) else _payload(s)
    return total


@torch.no_grad()
def compress_to_target(model, x, target_bytes=None, target_bpp=None, q_lo=(0.0, 0.0), q_hi=(1.0, 1.0), qmap_of=None, max_probes=8,
                       batch=None):
    """Code ``x`` ([N, 6]: voxel coordinates + rgb) into at most ``target_bytes`` of y + z payload.

    ``Q(t)`` is the uniform map at ``q_lo + t (q_hi - q_lo)`` — or ``qmap_of(t)``, a callable returning the SparseTensor map
    for ``t`` (view-dependent and region-of-interest maps scaled by ``t``).  ``bracket_search`` runs on
    ``model.estimate_bits(x, Q(t))["bytes"][1]``, the UPPER end of the proven interval of the stream length, and the real
    ``model.compress`` runs once, at the chosen ``t``.  Because that upper end bounds the stream,

        len(y string) + len(z string) <= target_bytes   whenever ``reached`` is true

    is a guarantee, not a tendency.  ``reached`` is false only when no probed map fits; the result is then the cheapest probe.

    The latent-coordinate side channel and the 28-byte header of the file container do not depend on ``Q``: the target is the
    y + z payload.  ``target_bpp`` is that payload in bits over the N input points (what ``count_bits`` reports), i.e.
    ``target_bytes = floor(target_bpp * N / 8)``; give exactly one of the two.

    -> dict: ``strings``, ``shape``, ``k``, ``coordinates`` (what ``compress`` returns: ``model.decompress(**those)`` decodes
    them), ``q`` = (q_g, q_a) (None with ``qmap_of``), ``t``, ``reached``, ``estimate`` (the chosen probe's upper end),
    ``log`` (every probe as (t, upper end)), ``bytes`` (the actual payload), ``target_bytes``.
    """
    if (target_bytes is None) == (target_bpp is None):
        raise ValueError("compress_to_target: give target_bytes or target_bpp (one of them)")
    n = int(x.shape[0])
    if target_bytes is None:
        target_bytes = int(float(target_bpp) * n // 8)
    target_bytes = int(target_bytes)

    def q_at(t):
        return tuple(float(lo) + t * (float(hi) - float(lo)) for lo, hi in zip(q_lo, q_hi))

    def map_at(t):
        if qmap_of is not None:
            return qmap_of(t)
        bcol = torch.zeros((n, 1), device=x.device, dtype=torch.int32) if batch is None else batch.to(x.device, torch.int32).reshape(n, 1)
        coords = torch.cat([bcol, x[:, :3].to(torch.int32)], dim=1).contiguous()
        return uniform_map(CoordMap(coords, 1), *q_at(t))

    found = bracket_search(lambda t: model.estimate_bits(x, map_at(t), batch=batch)["bytes"][1], target_bytes, max_probes=max_probes)
    strings, shape, k, coordinates = model.compress(x, map_at(found.t), batch=batch)
    return {"strings": strings, "shape": shape, "k": k, "coordinates": coordinates, "q": None if qmap_of is not None else q_at(found.t),
            "t": found.t, "reached": found.reached, "estimate": found.estimate, "log": found.log, "bytes": _payload(strings),
            "target_bytes": target_bytes}
