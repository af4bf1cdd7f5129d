"""MNIST MLP 784-256-128-10 (reference ``mnist_examples/models/mlp.py:29-102``).

Same layer names (``l1``, ``l2``, ``l3``) so state-dict keys and the wire layout
match the reference.  ``forward`` returns log-probabilities and the loss is
cross-entropy on them (a double log-softmax, idempotent: quirk Q21 kept).

``fused=True`` runs the training and evaluation steps on the three launches of
``csrc/mlp.hip`` (:func:`p2pfl_amd.ops.mlp_xent`) when :func:`p2pfl_amd.ops.mlp_ok`
allows -- on the GPU learner's mixed-precision arena -- and the path above
otherwise.  The kernels take the cross-entropy of the logits, which equals the
reference's cross-entropy of log-probabilities: ``log_softmax`` is idempotent
(quirk Q21), so the second one changes nothing.  ``forward`` is the same either
way.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from p2pfl_amd.models.base import FLModule, seed_everything


class MLP(FLModule):
    def __init__(self, out_channels: int = 10, lr_rate: float = 0.001, seed: Optional[int] = None,
                 fused: bool = False) -> None:
        seed_everything(seed)
        super().__init__()
        self.lr_rate = lr_rate
        self.fused = bool(fused)
        self.l1 = nn.Linear(28 * 28, 256)
        self.l2 = nn.Linear(256, 128)
        self.l3 = nn.Linear(128, out_channels)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.reshape(x.shape[0], -1)
        if x.is_cuda:
            from p2pfl_amd import ops

            if ops.available():
                # 784->256 and 256->128 on the hand-written MFMA GEMM (bias in its epilogue)
                x = torch.relu(ops.linear(x, self.l1.weight, self.l1.bias))
                x = torch.relu(ops.linear(x, self.l2.weight, self.l2.bias))
                return torch.log_softmax(self.l3(x), dim=1)
        x = torch.relu(self.l1(x))
        x = torch.relu(self.l2(x))
        return torch.log_softmax(self.l3(x), dim=1)

    # forward + loss (+ activation gradients) as two HIP launches (ops/mlp.py) when the gate allows
    def _fused_step(self, x: torch.Tensor, y: torch.Tensor):
        """``(loss, accuracy)`` from the fused kernels, or None: not asked for, not
        servable, or a subclass overrides ``loss_fn`` (the kernels compute the default)."""
        if not self.fused:
            return None
        from p2pfl_amd.ops import mlp

        if type(self).loss_fn is FLModule.loss_fn and mlp.mlp_ok(x, self.l1, self.l2, self.l3, y):
            mlp.STATS["native"] += 1
            loss, _, acc = mlp.mlp_xent(x, self.l1, self.l2, self.l3, y)
            return loss, acc
        mlp.STATS["fallback"] += 1
        return None

    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        out = self._fused_step(*batch)
        if out is None:
            return super().training_step(batch, batch_idx)
        self.log("train_loss", out[0], prog_bar=True)
        return out[0]

    def _eval_step(self, batch, prefix: str) -> torch.Tensor:
        out = self._fused_step(*batch)
        if out is None:
            return super()._eval_step(batch, prefix)
        self.log(f"{prefix}_loss", out[0], prog_bar=True)
        self.log(f"{prefix}_metric", out[1], prog_bar=True)
        return out[0]
