"""Fused GroupNorm (+ residual add) (+ ReLU) on channels-last activations (``csrc/groupnorm.hip``).

GroupNorm has no buffers, uses no batch statistics and behaves the same in
training and evaluation: the normalisation for label-skewed federated shards and
for differentially private updates (a ``norm="group"`` ResNet has nothing the
Gaussian mechanism must exempt).  :func:`group_norm_act` runs ``GroupNorm ->
(+ shortcut) -> ReLU`` as one launch forward and one (plus a tiny parameter-
gradient reduction) backward: a (sample, slab of whole groups) unit stays in LDS
between its statistics and its apply, so every tensor crosses HBM once.

Semantics equal ``act(F.group_norm(x, ...) + residual)`` (biased two-pass
variance per sample and group).  CPU tensors, NCHW-contiguous tensors, dtypes
other than bf16 / fp32, non-affine modules, ``C / G`` not a multiple of 8 or
above 512 and misaligned pointers use the plain PyTorch chain.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

# which path the calls took: the HIP kernels (forward / backward) or the PyTorch chain
STATS = {"native_fwd": 0, "native_bwd": 0, "fallback": 0}
MAX_CPG = 512  # csrc/groupnorm.hip kMaxOct * 8: one wave covers a slab row


def _gx():
    from p2pfl_amd.ops import ext

    return ext().gn


def _nhwc_3d(t: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] channels-last tensor -> its [N, H*W, C] storage view."""
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n, h * w, c)


def _from_3d(t3: torch.Tensor, shape) -> torch.Tensor:
    n, c, h, w = shape
    return t3.view(n, h, w, c).permute(0, 3, 1, 2)


def group_norm_act_reference(x, num_groups, weight, bias, eps, residual=None, relu=True):
    """Plain PyTorch definition (also the CPU / fallback path)."""
    y = F.group_norm(x, num_groups, weight, bias, eps)
    if residual is not None:
        y = y + residual
    return torch.relu(y) if relu else y


class _GroupNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, groups, eps, relu):
        x3 = _nhwc_3d(x)
        r3 = _nhwc_3d(residual.to(x.dtype)) if residual is not None else None
        y3, mean, rstd = _gx().fwd(x3, weight, bias, int(groups), r3, float(eps), bool(relu))
        STATS["native_fwd"] += 1
        ctx.save_for_backward(x3, y3, weight, mean, rstd)
        ctx.shape, ctx.relu, ctx.has_res = x.shape, bool(relu), residual is not None
        ctx.res_dtype = residual.dtype if residual is not None else None
        return _from_3d(y3, x.shape)

    @staticmethod
    def backward(ctx, dy):
        x3, y3, weight, mean, rstd = ctx.saved_tensors
        if dy.dtype != x3.dtype:
            dy = dy.to(x3.dtype)
        if not dy.is_contiguous(memory_format=torch.channels_last):
            dy = dy.contiguous(memory_format=torch.channels_last)
        out = _gx().bwd(_nhwc_3d(dy), y3, x3, weight, mean, rstd, ctx.relu, ctx.has_res and ctx.needs_input_grad[3])
        STATS["native_bwd"] += 1
        dx = _from_3d(out[0], ctx.shape)
        dres = _from_3d(out[3], ctx.shape).to(ctx.res_dtype) if len(out) > 3 else None
        return dx, out[1].to(weight.dtype), out[2].to(weight.dtype), dres, None, None, None


def _native_ok(x: torch.Tensor, gn: nn.GroupNorm, residual: Optional[torch.Tensor]) -> bool:
    from p2pfl_amd.ops import _gpu

    if not (_gpu(x) and x.dim() == 4 and x.dtype in (torch.bfloat16, torch.float32) and x.numel() > 0):
        return False
    cpg = gn.num_channels // gn.num_groups
    if not x.is_contiguous(memory_format=torch.channels_last) or x.shape[1] != gn.num_channels or cpg % 8 or cpg > MAX_CPG:
        return False
    if not gn.affine or any(p.dtype != torch.float32 or not p.is_contiguous() or p.data_ptr() % 16 for p in (gn.weight, gn.bias)):
        return False
    if residual is not None and (residual.shape != x.shape or not residual.is_contiguous(memory_format=torch.channels_last)):
        return False
    # 16-byte aligned rows of 8 channels
    return x.data_ptr() % 16 == 0 and (residual is None or residual.data_ptr() % 16 == 0)


def group_norm_act(x: torch.Tensor, gn: nn.GroupNorm, residual: Optional[torch.Tensor] = None, relu: bool = True,
                   fork: bool = False):
    """``act(gn(x) [+ residual])`` for a ``GroupNorm`` module, fused on MI355X; the same
    launch in training and evaluation.  ``fork=True`` returns the pair ``(y, y)`` for an
    output with two consumers (autograd adds their gradients)."""
    if _native_ok(x, gn, residual):
        y = _GroupNormAct.apply(x, gn.weight, gn.bias, residual, gn.num_groups, gn.eps, relu)
    else:
        STATS["fallback"] += 1
        y = group_norm_act_reference(x, gn.num_groups, gn.weight, gn.bias, gn.eps, residual, relu)
    return (y, y) if fork else y
