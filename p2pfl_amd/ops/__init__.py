"""Hand-written HIP/CDNA4 kernels (``csrc/*.hip``, extension ``p2pfl_amd._C``).

Every op has a plain-torch implementation used for CPU tensors (the control
plane and the CPU test-suite run without a GPU) and as the fp32 reference in
numerics tests.  For GPU tensors the HIP kernel is mandatory: if the extension
is missing on a GPU box the call raises instead of silently falling back, so a
"passing" GPU run always exercised the native path.
"""

from __future__ import annotations

import importlib
import os
from typing import Tuple, List, Optional, Sequence

import torch

_ext = None
_ext_error: Optional[BaseException] = None


def _load():
    global _ext, _ext_error
    if _ext is None and _ext_error is None:
        try:
            _ext = importlib.import_module("p2pfl_amd._C")
        except BaseException as e:  # ImportError, OSError (missing HIP runtime), ...
            _ext_error = e
    return _ext


def available() -> bool:
    return _load() is not None


def ext():
    """The native extension; raises loudly if it was not built."""
    m = _load()
    if m is None:
        raise RuntimeError(
            "p2pfl_amd native extension (p2pfl_amd._C) is not available: "
            f"{_ext_error!r}. Build it with `python setup.py build_ext --inplace` "
            "(PYTORCH_ROCM_ARCH=gfx950)."
        )
    return m


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda and os.environ.get("P2PFL_FORCE_TORCH_OPS") != "1"


# ----------------------------------------------------------------------------
# aggregation
# ----------------------------------------------------------------------------
def normalized_weights(weights: Sequence[float]) -> List[float]:
    total = float(sum(weights))
    if total <= 0:
        return [1.0 / len(weights)] * len(weights)
    return [float(w) / total for w in weights]


def fedavg_weights(weights: Sequence[float]) -> Tuple[List[float], float]:
    """(per-input weights, final scale) of a weighted mean: ``sum w_i x_i / sum w_i``
    is computed as raw-weight fp32 FMAs followed by ONE multiply by ``1 / sum w``,
    so it can be folded in several pieces (running sum) with bitwise-equal
    results.  All-zero weights fall back to the plain mean."""
    total = float(sum(weights))
    if total <= 0:
        return [1.0] * len(weights), 1.0 / len(weights)
    return [float(w) for w in weights], 1.0 / total


def weighted_sum_into(
    out: torch.Tensor,
    flats: Sequence[torch.Tensor],
    weights: Sequence[float],
    acc_in: Optional[torch.Tensor] = None,
    scale: float = 1.0,
) -> torch.Tensor:
    """``out = scale * (acc_in + sum_i weights[i] * flats[i])`` in fp32 (``acc_in``
    None = 0; it may be ``out`` itself).  One fused kernel on the GPU; the same
    operation sequence on the CPU, so pieces folded separately equal one call."""
    if not flats and acc_in is None:
        raise ValueError("no inputs")
    dev_t = flats[0] if flats else out
    if not _gpu(dev_t):
        acc = acc_in.clone() if acc_in is not None else torch.zeros(out.shape, dtype=torch.float32, device=out.device)
        for f, w in zip(flats, weights):
            acc.add_(f.to(acc.device, torch.float32), alpha=float(w))
        if scale != 1.0:
            acc.mul_(scale)
        out.copy_(acc)
        return out
    dev = out.device
    ok = (torch.float32, torch.bfloat16)
    srcs = [f if (f.device == dev and f.dtype in ok and f.is_contiguous() and f.data_ptr() % 16 == 0)
            else f.to(dev, torch.float32).contiguous() for f in flats]
    ext().weighted_sum(srcs, [float(w) for w in weights], out, acc_in, float(scale))
    return out


def weighted_average_reference(flats: Sequence[torch.Tensor], weights: Sequence[float]) -> torch.Tensor:
    w, scale = fedavg_weights(weights)
    acc = torch.zeros_like(flats[0], dtype=torch.float32)
    for f, wi in zip(flats, w):
        acc.add_(f.float(), alpha=wi)
    return acc.mul_(scale)


def weighted_average(
    flats: Sequence[torch.Tensor],
    weights: Sequence[float],
    out: Optional[torch.Tensor] = None,
    out_dtype: torch.dtype = torch.float32,
) -> torch.Tensor:
    """``sum_i w_i * flats[i] / sum_i w_i`` with fp32 accumulation (one fused kernel on GPU).

    Inputs may be fp32 or bf16 arenas in any mix (bf16 ones come from peers on
    the bf16 wire option) -- the kernel widens them in registers, no
    conversion pass; the result is fp32 (default) or bf16.
    """
    if len(flats) == 0:
        raise ValueError("no inputs")
    n = flats[0].numel()
    for f in flats:
        if f.numel() != n:
            raise ValueError("inputs differ in size")
    if out is not None:
        out_dtype = out.dtype
    w, scale = fedavg_weights(weights)
    if not _gpu(flats[0]):
        res = weighted_average_reference(flats, weights)
        if out is not None:
            out.copy_(res)
            return out
        return res.to(out_dtype)
    dev = flats[0].device
    if out_dtype == torch.bfloat16 and len(flats) > 16:
        res = weighted_average(flats, weights)  # fp32 partial sums, then one cast
        if out is None:
            return res.to(torch.bfloat16)
        out.copy_(res)
        return out
    if out is None:
        out = torch.empty(n, dtype=out_dtype, device=dev)
    return weighted_sum_into(out, flats, w, None, scale)


# ----------------------------------------------------------------------------
# robust aggregation (coordinate-wise order statistics, pairwise distances)
# ----------------------------------------------------------------------------
MAX_ROBUST_INPUTS = 16  # csrc/kernels.h kMaxInputs: one launch holds every input in registers


def _check_robust_inputs(flats: Sequence[torch.Tensor], op: str) -> int:
    k = len(flats)
    if k == 0:
        raise ValueError(f"{op}: no inputs")
    if k > MAX_ROBUST_INPUTS:
        raise ValueError(f"{op}: at most {MAX_ROBUST_INPUTS} inputs are supported, got {k}")
    n = flats[0].numel()
    for f in flats:
        if f.numel() != n:
            raise ValueError(f"{op}: inputs differ in size")
        if f.device != flats[0].device:
            raise ValueError(f"{op}: inputs are on different devices")
    return k


def _kernel_arenas(flats: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    ok = (torch.float32, torch.bfloat16)
    return [f if (f.dtype in ok and f.is_contiguous() and f.data_ptr() % 16 == 0) else f.float().contiguous()
            for f in (f.reshape(-1) for f in flats)]


def trimmed_mean_reference(flats: Sequence[torch.Tensor], trim: int) -> torch.Tensor:
    """Per coordinate: sort the k values, drop the ``trim`` lowest and highest,
    add the rest in ascending order in fp32 and divide by ``k - 2 * trim`` (the
    kernel's operation sequence)."""
    k = len(flats)
    s = torch.stack([f.reshape(-1).float() for f in flats]).sort(0).values
    acc = s[trim].clone()
    for j in range(trim + 1, k - trim):
        acc.add_(s[j])
    return acc.div_(float(k - 2 * trim))


def trimmed_mean(
    flats: Sequence[torch.Tensor],
    trim: int,
    out: Optional[torch.Tensor] = None,
    out_dtype: torch.dtype = torch.float32,
) -> torch.Tensor:
    """Coordinate-wise trimmed mean of up to 16 flat arenas (fp32 / bf16 in any
    mix): the ``trim`` lowest and ``trim`` highest values of every coordinate
    are dropped, ``0 <= trim <= (k - 1) // 2``.  ``trim = (k - 1) // 2`` is the
    median (numpy's: the mean of the two middle values for even k), ``trim = 0``
    the unweighted mean.  The result does not depend on the order of ``flats``.
    Inputs must be finite.  One fused kernel on the GPU."""
    k = _check_robust_inputs(flats, "trimmed_mean")
    trim = int(trim)
    if not 0 <= trim <= (k - 1) // 2:
        raise ValueError(f"trimmed_mean: trim must be in [0, {(k - 1) // 2}] for {k} inputs, got {trim}")
    n = flats[0].numel()
    if out is not None:
        if out.numel() != n or out.device != flats[0].device:
            raise ValueError("trimmed_mean: out must have the inputs' size and device")
        out_dtype = out.dtype
    if not _gpu(flats[0]):
        res = trimmed_mean_reference(flats, trim)
        if out is not None:
            out.copy_(res)
            return out
        return res.to(out_dtype)
    if out is None:
        out = torch.empty(n, dtype=out_dtype, device=flats[0].device)
    ext().trimmed_mean(_kernel_arenas(flats), trim, out)
    return out


def coordinate_median(
    flats: Sequence[torch.Tensor],
    out: Optional[torch.Tensor] = None,
    out_dtype: torch.dtype = torch.float32,
) -> torch.Tensor:
    """Coordinate-wise median: :func:`trimmed_mean` with ``trim = (k - 1) // 2``."""
    _check_robust_inputs(flats, "coordinate_median")
    return trimmed_mean(flats, (len(flats) - 1) // 2, out=out, out_dtype=out_dtype)


def pairwise_sqdist_reference(flats: Sequence[torch.Tensor]) -> torch.Tensor:
    """``D[i, j] = sum((flats[i] - flats[j]) ** 2)`` in fp32, one pair at a time."""
    k = len(flats)
    x = [f.reshape(-1).float() for f in flats]
    d = torch.zeros(k, k, dtype=torch.float32, device=x[0].device)
    for i in range(k):
        for j in range(i + 1, k):
            d[i, j] = d[j, i] = (x[i] - x[j]).square().sum()
    return d


def pairwise_sqdist(flats: Sequence[torch.Tensor]) -> torch.Tensor:
    """``k x k`` fp32 matrix of squared L2 distances between up to 16 flat
    arenas (fp32 / bf16), symmetric with a zero diagonal.  On the GPU every
    arena is read once and all reductions run in a fixed order without atomics:
    the same inputs in the same order give the bitwise-same matrix."""
    k = _check_robust_inputs(flats, "pairwise_sqdist")
    if not _gpu(flats[0]):
        return pairwise_sqdist_reference(flats)
    if k == 1:
        return torch.zeros(1, 1, dtype=torch.float32, device=flats[0].device)
    return ext().pairwise_sqdist(_kernel_arenas(flats))


# ----------------------------------------------------------------------------
# block-quantised int8 model wire, "q8" (csrc/quant_wire.hip)
# ----------------------------------------------------------------------------
Q8_BLOCK = 64  # elements per quantisation block = arena.ALIGN: a block never mixes two tensors
_Q8_NAN_BITS = 0x7FC00000
_Q8_INF_BITS = 0x7F800000
_Q8_TINY = 127.0 * 2.0**-126  # 127 * FLT_MIN, exact in fp32


def q8_packed_nbytes(n: int, n_raw: int = 0) -> int:
    """Bytes of the packed buffer of ``n`` elements with ``n_raw`` raw blocks:
    ``64 nb`` int8 codes, ``256 n_raw`` bytes of exact fp32 blocks, ``4 nb``
    bytes of fp32 scales, ``nb = ceil(n / 64)``; every section 64-byte aligned."""
    n, n_raw = int(n), int(n_raw)
    if n < 1 or n_raw < 0:
        raise ValueError("q8: n must be >= 1 and n_raw >= 0")
    nb = -(-n // Q8_BLOCK)
    return 64 * nb + 256 * n_raw + 4 * nb


def _q8_raw_ids(raw_blocks, nb: int, device: torch.device, table_ok: bool = False):
    """``raw_blocks`` as what the kernels or the reference take on ``device``: an
    int32 tensor, or (``table_ok``: for the kernels) the extension's
    ``Q8RawTable`` unchanged (None when there are none).  Checked here for host tables; the bindings check device tables."""
    if raw_blocks is None:
        return None
    if type(raw_blocks).__name__ == "Q8RawTable":  # the extension's table, checked where it was built
        if table_ok:
            return raw_blocks
        raw_blocks = raw_blocks.tensor().cpu()
    t = raw_blocks if isinstance(raw_blocks, torch.Tensor) else torch.tensor(list(raw_blocks), dtype=torch.int32)
    if t.numel() == 0:
        return None
    if t.dtype != torch.int32 or t.dim() != 1:
        raise ValueError("q8: raw_blocks must be a 1-D int32 tensor")
    if not t.is_cuda:
        if int(t.min()) < 0 or int(t.max()) >= nb:
            raise ValueError(f"q8: raw block index outside [0, {nb})")
        if t.numel() > 1 and not bool((t[1:] > t[:-1]).all()):
            raise ValueError("q8: raw_blocks must be sorted and unique")
    return t.to(device).contiguous()


def q8_encode_reference(flat: torch.Tensor, raw_blocks=None) -> torch.Tensor:
    """The q8 format written out literally in torch (IEEE binary32 throughout):
    per 64-element block ``scale = amax / 127`` and ``code = clamp(rint(x /
    scale), -127, 127)``; a block holding NaN or Inf gets a quiet-NaN scale and
    one with ``amax < 127 FLT_MIN`` a zero scale, codes 0 in both; the blocks
    in ``raw_blocks`` are also carried as exact fp32."""
    x = flat.detach().reshape(-1).float()  # bf16 widens exactly
    n = x.numel()
    nb = -(-n // Q8_BLOCK)
    raw = _q8_raw_ids(raw_blocks, nb, x.device)
    n_raw = 0 if raw is None else raw.numel()
    xb = torch.zeros(nb * Q8_BLOCK, dtype=torch.float32, device=x.device)
    xb[:n] = x
    xb = xb.view(nb, Q8_BLOCK)
    # the unsigned order of |x| bit patterns is their numeric order, and every
    # Inf / NaN pattern is >= 0x7F800000 (int32 is enough: the sign bit is cleared)
    mbits = (xb.view(torch.int32) & 0x7FFFFFFF).max(dim=1).values.contiguous()
    amax = mbits.view(torch.float32)
    nonfinite = mbits >= _Q8_INF_BITS
    tiny = ~nonfinite & (amax < _Q8_TINY)
    normal = ~(nonfinite | tiny)
    scale = amax / 127.0
    q = torch.round(xb / torch.where(normal, scale, torch.ones_like(scale))[:, None]).clamp_(-127.0, 127.0)
    q = torch.where(normal[:, None], q, torch.zeros_like(q)).to(torch.int8)
    sbits = scale.view(torch.int32).clone()
    sbits[tiny] = 0
    sbits[nonfinite] = _Q8_NAN_BITS
    packed = torch.empty(q8_packed_nbytes(n, n_raw), dtype=torch.uint8, device=x.device)
    c, r = 64 * nb, 256 * n_raw
    packed[:c] = q.view(torch.uint8).reshape(-1)
    if n_raw:
        packed[c : c + r] = xb[raw.long()].contiguous().view(torch.uint8).reshape(-1)
    packed[c + r :] = sbits.view(torch.uint8).reshape(-1)
    return packed


def _q8_cast(y: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """fp32 -> ``out_dtype``, round-to-nearest-even.  Rounding says nothing about
    a NaN, and torch's CPU conversion answers differently from one machine to
    the next (0x7FC0 on its scalar path, 0xFFFF on its AVX-512 one), so the
    format pins the usual IEEE choice, which is also what the gfx950 conversion
    instruction does: a bf16 NaN keeps the sign and the upper payload bits of
    the fp32 NaN and has its quiet bit set."""
    out = y.to(out_dtype)
    if out_dtype == torch.bfloat16:
        nan = torch.isnan(y)
        if bool(nan.any()):
            bits = (y.contiguous().view(torch.int32) >> 16) | 0x40  # arithmetic shift: the int16 pattern, sign kept
            out.view(torch.int16)[nan] = bits[nan].to(torch.int16)
    return out


def q8_decode_reference(packed: torch.Tensor, n: int, raw_blocks=None, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``y = float(code) * scale`` (one fp32 multiply), converted to ``out_dtype``
    round-to-nearest-even (:func:`_q8_cast`), then the raw blocks overwritten
    with their exact values."""
    n = int(n)
    nb = -(-n // Q8_BLOCK)
    raw = _q8_raw_ids(raw_blocks, nb, packed.device)
    n_raw = 0 if raw is None else raw.numel()
    if packed.dtype != torch.uint8 or packed.dim() != 1 or packed.numel() != q8_packed_nbytes(n, n_raw):
        raise ValueError("q8_decode: packed buffer does not have the size of n elements and these raw blocks")
    c, r = 64 * nb, 256 * n_raw
    codes = packed[:c].clone().view(torch.int8).view(nb, Q8_BLOCK)
    scales = packed[c + r :].clone().view(torch.float32)
    y = _q8_cast(codes.float() * scales[:, None], out_dtype)
    if n_raw:
        y[raw.long()] = _q8_cast(packed[c : c + r].clone().view(torch.float32).view(n_raw, Q8_BLOCK), out_dtype)
    return y.reshape(-1)[:n].clone()


def q8_encode(flat: torch.Tensor, raw_blocks=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pack a flat fp32 / bf16 arena into the q8 wire format: a ``uint8`` tensor
    of :func:`q8_packed_nbytes` bytes on the arena's device (0.27 of the fp32
    bytes).  ``raw_blocks``: sorted, unique int32 block indices kept exactly
    (:func:`p2pfl_amd.learning.arena.q8_raw_blocks`), already on the arena's
    device.  One kernel on the GPU plus a small one for the raw blocks.  A
    raw-block table given as a device tensor is read back and checked by the
    extension on every call, which waits for the work queued on the current
    stream; the ``Q8RawTable`` that ``q8_raw_table`` makes was checked where it
    was built and costs nothing per call."""
    flat = flat.detach().reshape(-1)
    if not _gpu(flat):
        res = q8_encode_reference(flat, raw_blocks)
        if out is not None:
            out.copy_(res)
            return out
        return res
    if flat.dtype not in (torch.float32, torch.bfloat16):
        flat = flat.float()
    if not (flat.is_contiguous() and flat.data_ptr() % 16 == 0):
        flat = flat.clone(memory_format=torch.contiguous_format)  # a fresh, aligned block
    nb = -(-flat.numel() // Q8_BLOCK)
    return ext().q8_encode(flat, _q8_raw_ids(raw_blocks, nb, flat.device, table_ok=True), out)


def q8_decode(
    packed: torch.Tensor,
    n: int,
    raw_blocks=None,
    out: Optional[torch.Tensor] = None,
    out_dtype: torch.dtype = torch.float32,
) -> torch.Tensor:
    """Unpack a q8 buffer of ``n`` elements into a flat fp32 (default) or bf16
    arena on the buffer's device; ``raw_blocks`` as for :func:`q8_encode`."""
    n = int(n)
    if out is not None:
        out_dtype = out.dtype
    if not _gpu(packed):
        res = q8_decode_reference(packed, n, raw_blocks, out_dtype)
        if out is not None:
            out.copy_(res)
            return out
        return res
    if not (packed.is_contiguous() and packed.data_ptr() % 16 == 0):
        packed = packed.clone(memory_format=torch.contiguous_format)
    if out is None:
        out = torch.empty(n, dtype=out_dtype, device=packed.device)
    ext().q8_decode(packed, n, _q8_raw_ids(raw_blocks, -(-n // Q8_BLOCK), packed.device, table_ok=True), out)
    return out


# ----------------------------------------------------------------------------
# optimizers (whole-arena, in place)
# ----------------------------------------------------------------------------
def adam_step_reference(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, decoupled=False):
    if weight_decay != 0:
        if decoupled:
            p.mul_(1 - lr * weight_decay)
        else:
            g = g + weight_decay * p
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1**step
    bc2 = 1 - beta2**step
    denom = (v.sqrt() / (bc2**0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)


def adam_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, decoupled=False, p_bf16=None):
    """In-place Adam/AdamW over flat fp32 buffers (optionally also writes a bf16 copy of p)."""
    if not _gpu(p):
        adam_step_reference(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, decoupled)
        if p_bf16 is not None:
            p_bf16.copy_(p)
        return
    ext().adam_step(p, g, m, v, p_bf16, float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), bool(decoupled))


def sgd_step_reference(p, g, buf, lr, momentum, dampening, weight_decay, nesterov, first_step):
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        if first_step:
            buf.copy_(g)
        else:
            buf.mul_(momentum).add_(g, alpha=1 - dampening)
        g = g + momentum * buf if nesterov else buf
    p.add_(g, alpha=-lr)


def sgd_step(p, g, buf, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first_step=False, p_bf16=None):
    if not _gpu(p):
        sgd_step_reference(p, g, buf, lr, momentum, dampening, weight_decay, nesterov, first_step)
        if p_bf16 is not None:
            p_bf16.copy_(p)
        return
    ext().sgd_step(p, g, buf, p_bf16, float(lr), float(momentum), float(dampening), float(weight_decay), bool(nesterov), bool(first_step))


# ----------------------------------------------------------------------------
# multi-tensor optimizers (mixed-precision learners: per-tensor grads, flat state)
# ----------------------------------------------------------------------------
def _mt_reference(step_fn, p, states, pbf, table, grads):
    for (off, n, flags), g in zip(table, grads):
        if g is None:
            continue
        view = lambda t: t[off : off + n]  # noqa: E731
        step_fn(view(p), g.reshape(-1).float(), *[view(s) if s is not None else None for s in states])
        if pbf is not None and flags & 2:
            if flags & 4:  # channels-last shadow region
                i, hw = (flags >> 8) & 0xFFFFFF, (flags >> 32) & 0xFFFFFF
                view(pbf).view(-1, hw, i).copy_(view(p).view(-1, i, hw).transpose(1, 2))
            else:
                view(pbf).copy_(view(p))


def adam_mt_step(p, m, v, grads, mt, *, lr, beta1, beta2, eps, weight_decay, step, decoupled=False, p_bf16=None, gtab=None, t_dev=None):
    """Adam/AdamW for tensors whose grads live outside the arena (``mt``: :class:`~p2pfl_amd.learning.optim.MTTables`).

    ``gtab`` (device int64 [T]) replaces ``grads`` by a persistent table of
    gradient addresses and ``t_dev`` (device int32 [1]) supplies the step
    count: together they make the launch replayable inside a HIP graph.
    """
    if not _gpu(p):
        _mt_reference(
            lambda pp, g, mm, vv: adam_step_reference(pp, g, mm, vv, lr, beta1, beta2, eps, weight_decay, step, decoupled),
            p, (m, v), p_bf16, mt.table, grads,
        )
        return
    ext().adam_mt_step(
        p, m, v, p_bf16, mt.tens, mt.chunks, list(grads), mt.numels, mt.grad_bf16, mt.grad_cl,
        float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), bool(decoupled), gtab, t_dev,
    )


def sgd_mt_step(p, buf, grads, mt, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first_step=False, p_bf16=None, gtab=None):
    if not _gpu(p):
        _mt_reference(
            lambda pp, g, b: sgd_step_reference(pp, g, b, lr, momentum, dampening, weight_decay, nesterov, first_step),
            p, (buf,), p_bf16, mt.table, grads,
        )
        return
    ext().sgd_mt_step(
        p, buf, p_bf16, mt.tens, mt.chunks, list(grads), mt.numels, mt.grad_bf16, mt.grad_cl,
        float(lr), float(momentum), float(dampening), float(weight_decay), bool(nesterov), bool(first_step), gtab,
    )


# ----------------------------------------------------------------------------
# fused transformer / classifier ops (csrc/fused_ops.hip)
# ----------------------------------------------------------------------------
from p2pfl_amd.ops.fused import (  # noqa: E402
    add_layer_norm,
    add_layer_norm_reference,
    attention_qkv,
    attention_qkv_reference,
    bias_gelu,
    bias_gelu_reference,
    embed_tokens,
    layer_norm,
    layer_norm_reference,
    patchify_u8,
    softmax_xent,
    softmax_xent_reference,
)
from p2pfl_amd.ops.fused import linear as linear_blas  # noqa: E402,F401  (hipBLASLt comparison path)
from p2pfl_amd.ops.gemm import gemm, gemm_reference, linear, linear_gelu  # noqa: E402,F401
from p2pfl_amd.ops.conv import conv2d  # noqa: E402,F401
from p2pfl_amd.ops.dp import (  # noqa: E402,F401  (csrc/dp_update.hip)
    DP_BLOCK,
    DP_NOISE_MAX,
    dp_apply,
    dp_apply_reference,
    dp_delta_sqnorm,
    dp_delta_sqnorm_reference,
    dp_noise_reference,
    philox4x32_reference,
)
