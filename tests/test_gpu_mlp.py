"""Fused MLP step (csrc/mlp.hip) against float64 and against the unfused path."""

from __future__ import annotations

import os

import pytest
import torch
from torch import nn

from p2pfl_amd import ops
from p2pfl_amd.ops import mlp as mlp_ops
from p2pfl_amd.ops import splitk

pytestmark = pytest.mark.gpu
NAMES = ["loss", "logits", "dW1", "db1", "dW2", "db2", "dW3", "db3"]


def _layers(K0, H1, H2, C, seed):
    """l1..l3 as the mixed-precision arena holds them: bf16 weights (1/sqrt(fan_in)), fp32 biases."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for i, o in ((K0, H1), (H1, H2), (H2, C)):
        lin = nn.Linear(i, o).cuda()
        lin.weight.data = (torch.randn(o, i, device="cuda", generator=g) / i**0.5).to(torch.bfloat16)
        lin.bias.data = torch.randn(o, device="cuda", generator=g) * 0.1
        out.append(lin)
    return out


def _inputs(B, K0, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(B, K0, device="cuda", generator=g)
    x = x * (torch.rand(B, K0, device="cuda", generator=g) > 1 / 3)  # a third of the pixels exactly 0
    y = torch.randint(0, C, (B,), device="cuda", generator=g)
    y[0], y[-1] = C - 1, 0
    return x, y


def _run(fn, layers, gscale):
    """[loss, logits, dW1, db1, dW2, db2, dW3, db3] and the accuracy of one step."""
    for lin in layers:
        lin.weight.grad = lin.bias.grad = None
    loss, logits, acc = fn()
    (loss * gscale).backward()
    grads = [t.grad.detach().clone() for lin in layers for t in (lin.weight, lin.bias)]
    return [loss.detach(), logits.detach()] + grads, float(acc)


@pytest.mark.parametrize("B,K0,H1,H2,C,gscale", [
    (1, 784, 256, 128, 10, 1.0), (31, 784, 256, 128, 10, 1.0), (32, 784, 256, 128, 10, 0.5), (33, 784, 256, 128, 10, 1.0),
    (69, 784, 256, 128, 10, 1.0), (5, 16, 32, 32, 1, 1.0), (40, 48, 64, 32, 32, 1.0)])
def test_mlp_xent_vs_float64(B, K0, H1, H2, C, gscale):
    """Per-tensor relative L2 error against float64 on the bf16-rounded weights and x: at most
    twice the error of the unfused path (Linear under bf16 autocast + F.cross_entropy + autograd).
    Both round gradients to bf16 once per layer, at different points; the factor covers that.
    Observed errors: profiles/mlp_fused.md."""
    ops.ext()
    layers = _layers(K0, H1, H2, C, seed=B + K0 + C)
    x, y = _inputs(B, K0, C, seed=B)
    assert mlp_ops.mlp_ok(x, *layers, y)
    fused, acc = _run(lambda: ops.mlp_xent(x, *layers, y), layers, gscale)

    from p2pfl_amd.models import MLP

    model = MLP()
    model.l1, model.l2, model.l3 = layers
    seen = []
    model.l3.register_forward_hook(lambda _m, _i, out: seen.append(out))  # forward() returns log-probabilities

    def unfused():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logp = model(x)
            return nn.functional.cross_entropy(logp, y), seen[-1], (logp.argmax(1) == y).float().mean()

    plain, _ = _run(unfused, layers, gscale)
    p64 = [t.detach().double().requires_grad_(True) for lin in layers for t in (lin.weight, lin.bias)]
    l64, lg64, _ = ops.mlp_xent_reference(x.to(torch.bfloat16).double(), *p64, y)
    (l64 * gscale).backward()
    ref = [l64.detach(), lg64.detach()] + [p.grad for p in p64]
    err = lambda a, r: float((a.double() - r).norm() / r.norm().clamp_min(1e-300))  # noqa: E731
    rows = []
    for name, a, u, r in zip(NAMES, fused, plain, ref):
        ef, eu = err(a, r), err(u, r)
        rows.append(f"| {B},{K0},{H1},{H2},{C} | {name} | {ef:.3e} | {eu:.3e} |")
        print(rows[-1])
    out = os.environ.get("P2PFL_MLP_ERRORS")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(rows) + "\n")
    for name, a, u, r in zip(NAMES, fused, plain, ref):
        assert a.shape == r.shape and err(a, r) <= 2 * err(u, r), name
    # accuracy: exact unless two logits of a row tie within the logits' error
    top = lg64.topk(min(2, C), dim=1).values
    tol = (fused[1].double() - lg64).abs().max()
    if C == 1 or bool(((top[:, 0] - top[:, -1]) > 2 * tol).all()):
        assert acc == pytest.approx(float((lg64.argmax(1) == y).double().mean()), abs=1e-6)


def test_mlp_masks_and_padding():
    """Dead ReLU units get exactly zero gradients; what lies behind row B is never read."""
    B, K0, H1, H2, C = 33, 784, 256, 128, 10
    layers = _layers(K0, H1, H2, C, seed=1)
    layers[0].bias.data[::2] = -100.0
    x, y = _inputs(B, K0, C, seed=2)
    a, acc_a = _run(lambda: ops.mlp_xent(x, *layers, y), layers, 1.0)
    assert not a[2][::2].any() and not a[3][::2].any() and a[2][1::2].any() and a[3][1::2].any()
    big = torch.full((B + 40, K0), float("nan"), device="cuda")
    big[:B] = x
    b, acc_b = _run(lambda: ops.mlp_xent(big[:B], *layers, y), layers, 1.0)
    assert acc_a == acc_b and all(torch.equal(s, t) for s, t in zip(a, b))


def test_mlp_deterministic_and_graph_replay():
    """The same inputs twice are bitwise equal, eagerly and from a captured graph replayed twice."""
    B, K0, H1, H2, C = 69, 784, 256, 128, 10
    layers = _layers(K0, H1, H2, C, seed=3)
    x, y = _inputs(B, K0, C, seed=4)
    step = lambda: _run(lambda: ops.mlp_xent(x, *layers, y), layers, 1.0)  # noqa: E731
    a, acc_a = step()
    b, acc_b = step()
    assert acc_a == acc_b and all(torch.equal(s, t) for s, t in zip(a, b))
    params = [t for lin in layers for t in (lin.weight, lin.bias)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loss, logits, _ = ops.mlp_xent(x, *layers, y)  # warm-up on the capture stream
        torch.autograd.grad(loss, params)
    torch.cuda.current_stream().wait_stream(side)
    graph, ring = torch.cuda.CUDAGraph(), splitk.GraphCounters(x.device, 64)  # the ring lives as long as the graph
    with splitk.graph_scope(ring), torch.cuda.graph(graph):
        loss, logits, acc = ops.mlp_xent(x, *layers, y)
        grads = torch.autograd.grad(loss, params)
    for _ in range(2):
        for t in (loss, logits, acc, *grads):
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert float(acc) == acc_a and all(torch.equal(s, t) for s, t in zip(a, [loss, logits, *grads]))


def test_mlp_fused_learner_end_to_end():
    """TorchLearner(MLP(fused=True)): two fits (the second replays the step graphs, ragged last
    batch included) and an evaluation, all on the fused kernels."""
    from p2pfl_amd.data import MnistFederatedDM
    from p2pfl_amd.learning.torch_learner import TorchLearner
    from p2pfl_amd.models import MLP
    from p2pfl_amd.ops.gemm import STATS as gemm_stats

    for s in (mlp_ops.STATS, gemm_stats):
        for k in s:
            s[k] = 0
    nl = TorchLearner(MLP(seed=0, fused=True), MnistFederatedDM(sub_id=0, number_sub=20), "gpu-mlp-fused", 1, device="cuda")
    ev0 = nl.evaluate()["test_loss"]
    nl.fit()
    nl.fit()
    torch.cuda.synchronize()
    params = nl.get_parameters()
    assert all(torch.isfinite(v).all() for v in params.values())
    assert nl.evaluate()["test_loss"] < ev0
    assert mlp_ops.STATS["fallback"] == 0 and mlp_ops.STATS["native"] > 0 and gemm_stats["torch"] == 0
    for name in nl.arena.shadow_names:
        w = dict(nl.model.named_parameters())[name]
        assert w.dtype == torch.bfloat16 and torch.equal(w.detach(), params[name].to(torch.bfloat16)), name
