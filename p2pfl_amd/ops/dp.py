"""Differentially private model updates (``csrc/dp_update.hip``): the Gaussian
mechanism on the update ``w - w0`` of a flat fp32 arena.

Two streaming passes, :func:`dp_delta_sqnorm` (the squared L2 norm of the
update) and :func:`dp_apply` (clip to ``C``, add ``N(0, (z C)^2)``), driven by
a block table with one byte per 64-element block: byte ``c`` says that the
first ``c`` elements of the block are privatised and the rest copied through
(``0``: an exempt block; ``64``: a full one; ``1..63``: a tensor's last block,
which is how padding stays untouched).
:func:`p2pfl_amd.learning.arena.dp_block_table` derives it from a layout.

The noise is a function of ``(seed, round, element index)`` alone: Philox4x32-10
keyed by the seed, counter ``(i // 4, round)``, four words per group of four
elements turned into two Box-Muller pairs.  ``u`` is at least ``2^-24``, so
``|g| <= sqrt(48 ln 2) ~= 5.77``: the Gaussian is truncated there.

As for every op, CPU tensors take the torch reference and GPU tensors require
the extension.
"""

from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

DP_BLOCK = 64  # elements per table byte = arena.ALIGN: a block never mixes two tensors
DP_NOISE_MAX = float(np.sqrt(48.0 * np.log(2.0)))  # the largest |g| the sampler can return

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_reference(counter_words: Sequence, key_words: Sequence) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., SC'11, the Random123 constants) in numpy
    ``uint64`` arithmetic.  ``counter_words``: four 32-bit words, each a scalar
    or an array (broadcast against each other); ``key_words``: two.  Returns
    ``uint32 [..., 4]``."""
    if len(counter_words) != 4 or len(key_words) != 2:
        raise ValueError("philox4x32: four counter words and two key words")
    c = list(np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _MASK for x in counter_words]))
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key_words)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]  # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def dp_noise_reference(n: int, seed: int, round: int, first: int = 0) -> np.ndarray:
    """The mechanism's standard-normal draws ``g[first .. first + n)`` in fp64, from the
    same bits as the kernel: group ``q = i // 4`` has counter ``(q low, q high,
    round, 0)`` and key ``(seed low, seed high)``; its words ``r0..r3`` give the
    Box-Muller pairs ``(r0, r1)`` and ``(r2, r3)`` with ``u = ((ra >> 8) + 1)
    2^-24``, ``t = (rb >> 8) 2^-24``, ``rad = sqrt(-2 ln u)`` and the pair
    ``(rad cos 2 pi t, rad sin 2 pi t)``."""
    n, seed, round, first = int(n), int(seed), int(round), int(first)
    if not (0 <= seed < 1 << 64 and 0 <= round < 1 << 32):
        raise ValueError("dp: seed must be in [0, 2^64) and round in [0, 2^32)")
    if first < 0 or first % 4:
        raise ValueError("dp: first must be a non-negative multiple of 4")
    q = np.arange(first // 4, first // 4 + -(-n // 4), dtype=np.uint64)
    r = philox4x32_reference((q & _MASK, q >> _S32, round, 0), (seed & 0xFFFFFFFF, seed >> 32))
    u = ((r[:, 0::2] >> 8).astype(np.float64) + 1.0) * 2.0**-24
    t = (r[:, 1::2] >> 8).astype(np.float64) * 2.0**-24
    rad = np.sqrt(-2.0 * np.log(u))
    g = np.stack([rad * np.cos(2.0 * np.pi * t), rad * np.sin(2.0 * np.pi * t)], axis=-1)  # [q, pair, (cos, sin)]
    return g.reshape(-1)[:n]


def _check(w: torch.Tensor, w0: torch.Tensor, table: torch.Tensor, op: str) -> int:
    n = w.numel()
    if w.dim() != 1 or n < DP_BLOCK or n % DP_BLOCK:
        raise ValueError(f"{op}: w must be a 1-D arena of a positive multiple of {DP_BLOCK} elements")
    if w.dtype != torch.float32 or w0.dtype != torch.float32:
        raise ValueError(f"{op}: w and w0 must be float32 arenas")
    if w0.shape != w.shape or w0.device != w.device:
        raise ValueError(f"{op}: w0 must have w's size and device")
    if table.dtype != torch.uint8 or table.dim() != 1 or table.numel() != n // DP_BLOCK or table.device != w.device:
        raise ValueError(f"{op}: table must be a uint8 [n / {DP_BLOCK}] tensor on the arena's device")
    return n


def _mask(table: torch.Tensor) -> torch.Tensor:
    """bool [n]: the privatised elements."""
    lane = torch.arange(DP_BLOCK, device=table.device, dtype=torch.int16)
    return (lane[None, :] < table.to(torch.int16)[:, None]).reshape(-1)


def dp_delta_sqnorm_reference(w: torch.Tensor, w0: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """``sum (w - w0)^2`` over the privatised elements, fp32, a 1-element tensor."""
    _check(w, w0, table, "dp_delta_sqnorm")
    d = torch.where(_mask(table), w - w0, torch.zeros_like(w))
    return d.square().sum().reshape(1)


def dp_delta_sqnorm(w: torch.Tensor, w0: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """Squared L2 norm of the update ``w - w0`` over the privatised elements:
    a 1-element fp32 tensor on the arenas' device, never read back here.  On the
    GPU one streaming launch plus a one-block finish, reduced in a fixed order
    without atomics on a grid that depends on ``n`` alone: the same inputs give
    the bitwise-same value on every node and stream."""
    from p2pfl_amd import ops

    w, w0 = w.detach(), w0.detach()
    if not ops._gpu(w):
        return dp_delta_sqnorm_reference(w, w0, table)
    _check(w, w0, table, "dp_delta_sqnorm")
    return ops.ext().dp_delta_sqnorm(w, w0, table)


def _check_apply(sqnorm: torch.Tensor, clip: float, noise_multiplier: float, seed: int, round: int) -> None:
    if not isinstance(sqnorm, torch.Tensor) or sqnorm.numel() != 1 or sqnorm.dtype != torch.float32:
        raise ValueError("dp_apply: sqnorm must be a 1-element float32 tensor")
    if not (clip > 0 and np.isfinite(clip)):
        raise ValueError("dp_apply: clip must be finite and > 0")
    if not (noise_multiplier >= 0 and np.isfinite(noise_multiplier)):
        raise ValueError("dp_apply: noise_multiplier must be finite and >= 0")
    if not (0 <= seed < 1 << 64 and 0 <= round < 1 << 32):
        raise ValueError("dp_apply: seed must be in [0, 2^64) and round in [0, 2^32)")


def _overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Byte ranges of two contiguous tensors on one device intersect (the binding's check)."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a.device == b.device and a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def dp_apply_reference(
    w: torch.Tensor,
    w0: torch.Tensor,
    table: torch.Tensor,
    sqnorm: torch.Tensor,
    clip: float,
    noise_multiplier: float,
    seed: int,
    round: int,
) -> torch.Tensor:
    """The mechanism in torch fp32, one singly rounded operation at a time (the
    kernel's sequence, so ``base`` agrees bit for bit): ``base = w`` if
    ``sqnorm <= C * C`` else ``w0 + (C / sqrt(sqnorm)) * (w - w0)``; then ``base
    + float32(z C) * g`` with ``g`` = :func:`dp_noise_reference` rounded to fp32
    (the kernel samples in fp32: it agrees to a few ulp there, not bitwise).
    Elements outside the table's counts are ``w``."""
    _check(w, w0, table, "dp_apply")
    clip, noise_multiplier, seed, round = float(clip), float(noise_multiplier), int(seed), int(round)
    _check_apply(sqnorm, clip, noise_multiplier, seed, round)
    dev = w.device
    ss = sqnorm.detach().reshape(()).to(dev)
    c = torch.tensor(clip, dtype=torch.float32, device=dev)
    if bool(ss <= c * c):
        base = w.clone()
    else:
        s = c / ss.sqrt()
        base = w0 + s * (w - w0)
    if noise_multiplier > 0:
        sigma = torch.tensor(noise_multiplier * clip, dtype=torch.float32, device=dev)  # the product rounded once
        g = torch.from_numpy(dp_noise_reference(w.numel(), seed, round).astype(np.float32)).to(dev)
        base = base + sigma * g
    return torch.where(_mask(table), base, w)


def dp_apply(
    w: torch.Tensor,
    w0: torch.Tensor,
    table: torch.Tensor,
    sqnorm: torch.Tensor,
    clip: float,
    noise_multiplier: float,
    seed: int,
    round: int,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Clip the update ``w - w0`` to L2 norm ``clip`` given its squared norm
    (``sqnorm``, a 1-element tensor on the device: :func:`dp_delta_sqnorm`) and
    add ``N(0, (noise_multiplier * clip)^2)`` to every privatised element.
    Returns a fresh arena (``out`` if given; it may not overlap ``w`` or
    ``w0``); elements the table does not privatise are ``w`` bitwise, and so is
    everything when nothing is clipped and ``noise_multiplier`` is 0.  One
    launch, no host synchronisation."""
    from p2pfl_amd import ops

    w, w0 = w.detach(), w0.detach()
    if not ops._gpu(w):
        res = dp_apply_reference(w, w0, table, sqnorm, clip, noise_multiplier, seed, round)
        if out is not None:
            if _overlaps(out, w) or _overlaps(out, w0):
                raise ValueError("dp_apply: out must not overlap w or w0")
            out.copy_(res)
            return out
        return res
    _check(w, w0, table, "dp_apply")
    clip, noise_multiplier, seed, round = float(clip), float(noise_multiplier), int(seed), int(round)
    _check_apply(sqnorm, clip, noise_multiplier, seed, round)
    return ops.ext().dp_apply(w, w0, table, sqnorm, clip, noise_multiplier, seed, round, out)
