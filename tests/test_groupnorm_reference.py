"""ops.group_norm_act off the GPU, and the ``norm="group"`` ResNets (no GPU needed)."""

from __future__ import annotations

import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from p2pfl_amd import ops
from p2pfl_amd.models.resnet import ResNet18


@pytest.mark.parametrize("has_res,relu", [(False, True), (True, True), (False, False), (True, False)])
def test_reference_is_group_norm_add_relu_in_float64(has_res, relu):
    g = torch.Generator().manual_seed(3)
    gn = nn.GroupNorm(3, 48).double()
    with torch.no_grad():
        gn.weight.copy_(torch.randn(48, generator=g, dtype=torch.float64))
        gn.bias.copy_(torch.randn(48, generator=g, dtype=torch.float64))
    dy = torch.randn(2, 48, 5, 7, generator=g, dtype=torch.float64)
    outs = []
    for ours in (True, False):
        x = torch.randn(2, 48, 5, 7, generator=torch.Generator().manual_seed(4), dtype=torch.float64, requires_grad=True)
        r = torch.randn(2, 48, 5, 7, generator=torch.Generator().manual_seed(5), dtype=torch.float64, requires_grad=True)
        gn.zero_grad()
        if ours:
            y, y2 = ops.group_norm_act(x, gn, r if has_res else None, relu, fork=True)
            assert y2 is y
        else:
            y = F.group_norm(x, 3, gn.weight, gn.bias, gn.eps)
            y = y + r if has_res else y
            y = torch.relu(y) if relu else y
        y.backward(dy)
        outs.append([y.detach(), x.grad, gn.weight.grad.clone(), gn.bias.grad.clone()] + ([r.grad] if has_res else []))
    for a, b in zip(*outs):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def test_group_resnet_has_no_buffers_and_trains_a_cpu_step():
    model, batch_model = ResNet18(norm="group", seed=0), ResNet18(seed=0)
    assert list(model.buffers()) == []
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in batch_model.named_parameters()]
    assert model.stem[1].num_groups == 4 and ResNet18(norm="group", gn_channels_per_group=8).layer4[1].bn2.num_groups == 64
    opt = model.configure_optimizers()
    x = torch.randint(0, 256, (2, 3, 32, 32), dtype=torch.uint8)
    before = model.layer1[0].bn1.weight.detach().clone()
    loss = model.training_step((x, torch.tensor([1, 7])), 0)
    loss.backward()
    opt.step()
    assert bool(torch.isfinite(loss)) and not torch.equal(before, model.layer1[0].bn1.weight)
    model.eval()  # no running statistics: evaluation normalises exactly as training did
    with torch.no_grad():
        assert bool(torch.isfinite(model(x)).all())


def test_unknown_norm_raises():
    with pytest.raises(ValueError):
        ResNet18(norm="layer")


def test_default_resnet_state_dict_keeps_its_batchnorm_keys():
    keys = list(ResNet18().state_dict())
    norms = [k for k in keys if re.search(r"(stem\.1|bn\d|shortcut\.1)\.", k)]
    assert len(keys) == 122 and len(norms) == 100  # 20 BatchNorms x 5 tensors, 21 convolutions, fc weight + bias
    for k in norms:
        assert k.rsplit(".", 1)[1] in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    assert sum(k.endswith("running_var") for k in keys) == 20
