"""Byzantine-robust aggregation on flat arenas: FedMedian, TrimmedMean, Krum.

A sample-weighted mean is moved arbitrarily far by ONE diverged or malicious
train-set member.  The three strategies here bound that influence:

* :class:`FedMedian` -- coordinate-wise median (Yin et al. 2018);
* :class:`TrimmedMean` -- coordinate-wise mean after dropping the ``trim``
  lowest and highest values (same paper);
* :class:`Krum` -- the model(s) closest to their nearest neighbours in squared
  L2 distance (Blanchard et al. 2017; ``m > 1`` is Multi-Krum).

Each is one streaming pass over the k arenas (``ops.trimmed_mean`` /
``ops.pairwise_sqdist``, csrc/robust_agg.hip) instead of a per-layer torch
loop.  None of them is a function of partial results, so they set
``partial_aggregation = False``: gossip delivers the train set's models one by
one and every member aggregates the same k single models, presented to the
kernel in sorted-contributor-key order -- bitwise the same result on every
node whatever the arrival order.
"""

from __future__ import annotations

from typing import Any, Dict, List, Tuple

import torch

from p2pfl_amd import ops
from p2pfl_amd.learning.aggregators.aggregator import Aggregator, NoModelsToAggregateError
from p2pfl_amd.learning.aggregators.fedavg import _reading_all
from p2pfl_amd.learning.arena import FlatParams, flatten
from p2pfl_amd.utils import finite


class _FlatAggregator(Aggregator):
    """Flattening, canonical order and result packaging shared by the three
    strategies; subclasses implement :meth:`_combine` on the flat arenas."""

    partial_aggregation = False

    def _combine(self, flats: List[torch.Tensor], weights: List[float]) -> torch.Tensor:
        raise NotImplementedError

    def aggregate(self, models: Dict[str, Tuple[Any, int]]) -> FlatParams:
        if len(models) == 0:
            raise NoModelsToAggregateError(f"({self.node_name}) Trying to aggregate models when there is no models")
        if len(models) > ops.MAX_ROBUST_INPUTS:
            raise ValueError(f"{type(self).__name__} aggregates at most {ops.MAX_ROBUST_INPUTS} models, got {len(models)}")
        keys = sorted(models)  # canonical order: ties and summation order do not depend on arrival
        entries = [models[k] for k in keys]
        ref = entries[-1][0]
        device = next(iter(ref.values())).device if len(ref) else torch.device("cpu")
        flats: List[FlatParams] = [flatten(m, device=device) for m, _ in entries]
        layout = flats[0].layout
        for f in flats:
            if not f.layout.compatible(layout):
                raise ValueError("Cannot aggregate models with different layouts")
        name = type(self).__name__
        with _reading_all(flats):  # a learner's live weights: after its last write, before its next
            out = self._combine([f.flat for f in flats], [float(w) for _, w in entries])
        if finite.ENABLED:
            for k, f in zip(keys, flats):
                finite.check(self.node_name, f"{name} input", f, key=k)
            finite.check(self.node_name, f"{name} result", out, keys=keys)
        result = FlatParams.from_flat(out, layout)
        if not isinstance(ref, FlatParams):
            # preserve the caller's key order/names for plain dicts
            renamed = FlatParams()
            for (pname, _), view in zip(ref.items(), result.values()):
                renamed[pname] = view
            renamed.flat, renamed.layout = result.flat, result.layout
            return renamed
        return result


class FedMedian(_FlatAggregator):
    """Coordinate-wise median of the models (the mean of the two middle values
    for an even count).  Sample weights are ignored."""

    def _combine(self, flats, weights):
        return ops.coordinate_median(flats)


class TrimmedMean(_FlatAggregator):
    """Coordinate-wise mean after dropping the ``trim`` lowest and ``trim``
    highest values; with k models on hand ``min(trim, (k - 1) // 2)`` are
    dropped at each end.  Sample weights are ignored."""

    def __init__(self, node_name: str = "unknown", trim: int = 1) -> None:
        super().__init__(node_name)
        if trim < 0:
            raise ValueError("trim must be >= 0")
        self.trim = int(trim)

    def _combine(self, flats, weights):
        return ops.trimmed_mean(flats, min(self.trim, (len(flats) - 1) // 2))


def krum_select(dist: List[List[float]], f: int, m: int) -> List[int]:
    """Indices (ascending) of the models (Multi-)Krum keeps, from the k x k
    matrix of squared distances.  ``score(i)`` is the sum of the
    ``k - f_eff - 2`` smallest ``dist[i][j != i]`` with
    ``f_eff = min(f, max(0, (k - 3) // 2))``; the ``min(m, k - f_eff)`` lowest
    scores win, ties going to the lower index (canonical key order)."""
    k = len(dist)
    f_eff = min(f, max(0, (k - 3) // 2))
    closest = max(k - f_eff - 2, 0)
    scores = [sum(sorted(dist[i][j] for j in range(k) if j != i)[:closest]) for i in range(k)]
    order = sorted(range(k), key=lambda i: (scores[i], i))
    return sorted(order[: max(1, min(m, k - f_eff))])


class Krum(_FlatAggregator):
    """Krum (``m = 1``) and Multi-Krum: score every model by the summed squared
    distance to its ``k - f - 2`` nearest other models, keep the ``m`` best and
    return their sample-weighted mean (for ``m = 1``: that model, bitwise).
    ``f`` is the number of Byzantine members tolerated; with k models on hand it
    is clamped to ``(k - 3) // 2``.  With k <= 2 there is nothing to score and
    the result is the unweighted mean."""

    def __init__(self, node_name: str = "unknown", f: int = 1, m: int = 1) -> None:
        super().__init__(node_name)
        if f < 0 or m < 1:
            raise ValueError("Krum needs f >= 0 and m >= 1")
        self.f, self.m = int(f), int(m)

    def _combine(self, flats, weights):
        k = len(flats)
        if k <= 2:
            return ops.weighted_average(flats, [1.0] * k)
        dist = ops.pairwise_sqdist(flats).tolist()  # one device-to-host copy of k * k floats
        keep = krum_select(dist, self.f, self.m)
        w = [1.0] if len(keep) == 1 else [weights[i] for i in keep]
        return ops.weighted_average([flats[i] for i in keep], w)
