"""The fused MLP step's plain-torch definition and its CPU fallback."""

from __future__ import annotations

import torch
from torch import nn

from p2pfl_amd import ops
from p2pfl_amd.models import MLP


def test_mlp_xent_reference_equals_the_model_in_float64():
    """Cross-entropy of the logits = the model's cross-entropy of log-probabilities (quirk Q21)."""
    m = MLP(seed=3).double()
    x, y = torch.rand(9, 1, 28, 28, dtype=torch.float64), torch.randint(0, 10, (9,))
    params = [p for lin in (m.l1, m.l2, m.l3) for p in (lin.weight, lin.bias)]
    loss, logits, acc = ops.mlp_xent_reference(x, *params, y)
    out = m(x)
    want = nn.functional.cross_entropy(out, y)
    torch.testing.assert_close(loss, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(torch.log_softmax(logits, 1), out, rtol=1e-12, atol=1e-12)
    assert float(acc) == float((out.argmax(1) == y).double().mean())
    for g, w in zip(torch.autograd.grad(loss, params), torch.autograd.grad(want, params)):
        torch.testing.assert_close(g, w, rtol=1e-10, atol=1e-12)


def test_mlp_fused_on_cpu_trains_through_the_fallback_bitwise():
    from p2pfl_amd.ops import mlp as mlp_ops

    before = mlp_ops.STATS["fallback"]
    models = [MLP(seed=5), MLP(seed=5, fused=True)]
    g = torch.Generator().manual_seed(0)
    batches = [(torch.rand(8, 1, 28, 28, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(3)]
    for m in models:
        opt = m.configure_optimizers()
        for i, b in enumerate(batches):
            opt.zero_grad()
            m.training_step(b, i).backward()
            opt.step()
        m.test_step(batches[0], 0)
    assert mlp_ops.STATS["fallback"] == before + 4
    assert models[0].pop_logged().keys() == models[1].pop_logged().keys()
    for a, b in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(a, b)
