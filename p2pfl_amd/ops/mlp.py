"""Fused MLP step on three HIP launches (``csrc/mlp.hip``).

``Linear+ReLU -> Linear+ReLU -> Linear -> softmax cross-entropy``: the MNIST
MLP (784-256-128-10).  :func:`mlp_xent` returns ``(loss, logits, accuracy)``
from two forward launches; when a gradient is wanted the second one goes on to
the activation gradients, and the backward is one launch producing all six
parameter gradients (weights bf16, biases fp32: what the arena's multi-tensor
optimizer consumes).  There is no input gradient.  PyTorch-ROCm runs the same
step as two GEMM launches, two ReLUs, a hipBLASLt GEMM for the 10-class layer,
two log-softmaxes, an nll and autograd's mirror of all of it.  The reference's
model: ``mnist_examples/models/mlp.py``.
"""

from __future__ import annotations

from typing import Tuple

import torch
from torch import nn

# which path MLP(fused=True) steps took: the HIP kernels or the plain model path
STATS = {"native": 0, "fallback": 0}
MAX_H1, MAX_H2, MAX_C = 256, 128, 32  # csrc/mlp.h


def _C():
    from p2pfl_amd.ops import ext

    return ext()


def mlp_ok(x: torch.Tensor, l1: nn.Linear, l2: nn.Linear, l3: nn.Linear, y: torch.Tensor) -> bool:
    """True when the kernels serve this step: GPU tensors, ``x`` fp32 / bf16, contiguous
    and without a gradient, bf16 weights and fp32 biases (the learner's mixed-precision
    arena), ``K0 % 16 == 0``, ``H1 % 32 == 0 <= 256``, ``H2 % 32 == 0 <= 128``, ``1 <= C <= 32``."""
    from p2pfl_amd.ops import _gpu

    if not _gpu(x) or x.dim() < 2 or x.shape[0] < 1 or x.dtype not in (torch.float32, torch.bfloat16):
        return False
    if x.requires_grad or not x.is_contiguous() or x.data_ptr() % 16:
        return False
    k0, h1, h2, c = l1.in_features, l1.out_features, l2.out_features, l3.out_features
    if x[0].numel() != k0 or l2.in_features != h1 or l3.in_features != h2:
        return False
    if k0 % 16 or h1 % 32 or h1 > MAX_H1 or h2 % 32 or h2 > MAX_H2 or not 1 <= c <= MAX_C:
        return False
    for lin in (l1, l2, l3):
        w, b = lin.weight, lin.bias
        if b is None or w.device != x.device or b.device != x.device:
            return False
        if w.dtype != torch.bfloat16 or not w.is_contiguous() or w.data_ptr() % 16:
            return False
        if b.dtype != torch.float32 or not b.is_contiguous():
            return False
    return y.device == x.device and y.dtype == torch.int64 and y.dim() == 1 and y.shape[0] == x.shape[0]


class _MlpXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, y, train):
        from p2pfl_amd.ops import splitk

        x2 = x.reshape(x.shape[0], -1)
        y = y.contiguous()
        loss, logits, acc, acts = _C().mlp.fwd(x2, w1, b1, w2, b2, w3, b3, y, splitk.counters(1, x.device), train)
        if train:
            ctx.save_for_backward(x2, acts)
            ctx.dims = (w1.shape[0], w2.shape[0], w3.shape[0])
        ctx.mark_non_differentiable(logits, acc)
        ctx.set_materialize_grads(False)  # no zero-filled gradients for logits / accuracy
        return loss, logits, acc

    @staticmethod
    def backward(ctx, gloss, _glogits, _gacc):
        x2, acts = ctx.saved_tensors
        dw1, db1, dw2, db2, dw3, db3 = _C().mlp.bwd(gloss.float().reshape(1), x2, acts, *ctx.dims)
        return None, dw1, db1, dw2, db2, dw3, db3, None, None


def mlp_xent(x: torch.Tensor, l1: nn.Linear, l2: nn.Linear, l3: nn.Linear,
             y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(mean cross-entropy, logits, accuracy)`` of ``l3(relu(l2(relu(l1(x)))))`` against ``y``
    (:func:`mlp_ok`); differentiable in the six parameters."""
    params = (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
    # the backward half of the second launch runs only when a gradient will be asked for
    train = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    return _MlpXent.apply(x, *params, y, train)


def mlp_xent_reference(x, w1, b1, w2, b2, w3, b3, y):
    """Plain torch definition in the operands' dtype: ``(loss, logits, accuracy)``."""
    h = torch.relu(x.reshape(x.shape[0], -1) @ w1.t() + b1)
    h = torch.relu(h @ w2.t() + b2)
    logits = h @ w3.t() + b3
    return nn.functional.cross_entropy(logits, y), logits, (logits.argmax(dim=1) == y).to(logits.dtype).mean()
