"""Differentially private model updates: the Gaussian mechanism, per node.

A node's trained weights go to its train-set peers as they are, alone or inside
a partial aggregate, and a peer that subtracts the round's starting model holds
this node's exact update -- the object gradient-inversion and
membership-inference attacks work from.  With a :class:`GaussianMechanism` on
the node (``Node(..., privacy=GaussianMechanism(clip_norm, noise_multiplier))``)
``TrainStage`` releases a privatised copy instead: the update ``delta = w_trained
- w_round_start`` is scaled to an L2 norm of at most ``C = clip_norm`` and
``N(0, (z C)^2)``, ``z = noise_multiplier``, is added to every coordinate, in two
streaming HIP launches over the whole arena (``csrc/dp_update.hip``).  The
learner's own weights are not touched.

What this covers, and what it does not:

* It is *local*, node-level protection of each released update against the
  peers that receive it (and anyone behind them); there is no trusted party.
* The sample count sent with a model is not covered, and neither are the exempt
  tensors -- by default BatchNorm's running statistics, because a noised
  variance goes negative.  They travel as they are.
* The noise is sampled in fp32, with the known floating-point caveat of every
  such sampler (Mironov, "On significance of the least significant bits for
  differential privacy", CCS 2012), and is truncated at ``|g| <= 5.77``.
* What happens to a released model afterwards -- the ``q8`` and ``bf16`` wires,
  aggregation -- is post-processing and cannot weaken the guarantee.

Accounting (:meth:`GaussianMechanism.epsilon`): two updates each clipped to
``C`` differ by at most ``2 C`` in L2 norm, so one release satisfies Renyi DP
``(alpha, 2 alpha / z^2)``; ``T`` adaptive releases add up to ``alpha a`` with
``a = 2 T / z^2``, which converts to ``(alpha a + ln(1 / delta) / (alpha - 1),
delta)``-DP.  Minimised over ``alpha > 1`` (at ``alpha = 1 + sqrt(ln(1 / delta)
/ a)``) that is ``epsilon = a + 2 sqrt(a ln(1 / delta))``.
"""

from __future__ import annotations

import math
import secrets
import threading
from typing import Iterable, Optional

import torch

from p2pfl_amd import ops
from p2pfl_amd.learning import arena
from p2pfl_amd.learning.arena import FlatParams


def gaussian_epsilon(releases: int, noise_multiplier: float, delta: float) -> float:
    """``epsilon`` of ``releases`` adaptive Gaussian-mechanism releases of an
    update clipped to ``C`` with noise ``N(0, (z C)^2)`` (sensitivity ``2 C``),
    at ``delta``: ``a + 2 sqrt(a ln(1 / delta))`` with ``a = 2 T / z^2``; 0 for
    no release, ``inf`` without noise."""
    if releases <= 0:
        return 0.0
    if noise_multiplier <= 0:
        return math.inf
    a = 2.0 * releases / (noise_multiplier * noise_multiplier)
    return a + 2.0 * math.sqrt(a * math.log(1.0 / delta))


class GaussianMechanism:
    """Clip a node's update to ``clip_norm`` and add ``N(0, (noise_multiplier *
    clip_norm)^2)`` to every coordinate before it leaves the node.

    ``seed``: the 64-bit key of the counter-based generator; ``None`` draws
    ``secrets.randbits(64)`` per instance.  It is never logged or sent: whoever
    knows it can subtract the noise.  The draws are a function of ``(seed,
    release index, element)``: the generator's round word is this instance's
    own release counter, not the experiment's round number, which starts over
    with every experiment -- two releases under one (seed, word) would carry the
    same noise, and their difference none at all.  The counter only lives as
    long as the instance: do not build a second mechanism from an explicit
    ``seed`` that has already released something.
    ``exempt``: name suffixes of tensors that are copied through unprotected.
    """

    def __init__(
        self,
        clip_norm: float,
        noise_multiplier: float = 0.0,
        seed: Optional[int] = None,
        delta: float = 1e-5,
        exempt: Iterable[str] = arena.DP_EXEMPT,
    ) -> None:
        clip_norm, noise_multiplier, delta = float(clip_norm), float(noise_multiplier), float(delta)
        if not (clip_norm > 0 and math.isfinite(clip_norm)):
            raise ValueError("clip_norm must be finite and > 0")
        if not (noise_multiplier >= 0 and math.isfinite(noise_multiplier)):
            raise ValueError("noise_multiplier must be finite and >= 0")
        if not 0 < delta < 1:
            raise ValueError("delta must be in (0, 1)")
        seed = secrets.randbits(64) if seed is None else int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed must be in [0, 2^64)")
        self.clip_norm = clip_norm
        self.noise_multiplier = noise_multiplier
        self.delta = delta
        self.exempt = tuple(exempt)
        self._seed = seed
        self._lock = threading.Lock()
        self._releases = 0
        self.last_round: Optional[int] = None
        self._last_sqnorm: Optional[torch.Tensor] = None

    def __repr__(self) -> str:  # no seed
        return (f"GaussianMechanism(clip_norm={self.clip_norm}, noise_multiplier={self.noise_multiplier}, "
                f"delta={self.delta})")

    @property
    def releases(self) -> int:
        """Calls to :meth:`privatize` so far: the ``T`` of :meth:`epsilon`."""
        return self._releases

    def privatize(self, live: FlatParams, start: FlatParams, round: int) -> FlatParams:
        """The privatised copy of ``live`` for release: ``start + clip(live -
        start) + noise`` on the covered elements, ``live`` elsewhere.  ``live``
        may be a learner's live weights (read under ``arena.reading``), ``start``
        a snapshot of them from before training.  Both launches go to the
        caller's current stream and nothing is read back; returns a fresh
        :class:`FlatParams` with ``live``'s layout.  ``round`` is the caller's
        round number, kept as ``last_round``; the noise is indexed by the release
        counter (``releases`` before the call), which never repeats."""
        if not (isinstance(live, FlatParams) and isinstance(start, FlatParams)):
            raise TypeError("privatize takes FlatParams arenas")
        layout = live.layout
        if not start.layout.compatible(layout) or start.flat.device != live.flat.device:
            raise ValueError("the round-start weights do not match the live weights")
        if live.flat.numel() != layout.numel or start.flat.numel() != layout.numel or live.flat.dtype != torch.float32:
            raise ValueError("privatize takes fp32 arenas of the layout's size")
        table = arena.dp_block_table(layout, self.exempt, live.flat.device)
        with self._lock:
            # reserved before anything is launched and never handed out twice, also if the
            # launch fails: a release that may have happened counts
            index = self._releases
            if index >= 1 << 32:
                raise RuntimeError("this mechanism has used all 2^32 noise streams of its seed")
            self._releases = index + 1
            self.last_round = int(round)
        with arena.reading(live):
            ss = ops.dp_delta_sqnorm(live.flat, start.flat, table)
            out = ops.dp_apply(live.flat, start.flat, table, ss, self.clip_norm, self.noise_multiplier, self._seed,
                               index)
        with self._lock:
            self._last_sqnorm = ss
        return FlatParams.from_flat(out, layout)

    def last_update_norm(self) -> Optional[float]:
        """L2 norm of the last update before clipping (None before the first
        release).  Reads one scalar back from the device: waits for it."""
        ss = self._last_sqnorm
        return None if ss is None else math.sqrt(float(ss.item()))

    def epsilon(self, rounds: Optional[int] = None) -> float:
        """``epsilon`` at this mechanism's ``delta`` after ``rounds`` releases
        (default: the calls to :meth:`privatize` so far); see
        :func:`gaussian_epsilon`."""
        t = self._releases if rounds is None else int(rounds)
        return gaussian_epsilon(t, self.noise_multiplier, self.delta)
