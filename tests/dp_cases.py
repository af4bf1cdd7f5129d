"""Inputs shared by tests/test_privacy.py and tests/test_gpu_dp_update.py."""

from __future__ import annotations

import math

import torch

from p2pfl_amd.learning.arena import ParamLayout

# (name, size, dtype): every way a tensor can end inside a 64-element block, one
# tensor of more than one full block plus a tail, an integer buffer and a float
# running statistic (both exempt)
SYNTHETIC = (
    ("a.weight", 1, torch.float32),
    ("b.weight", 63, torch.float32),
    ("c.weight", 64, torch.float32),
    ("d.weight", 65, torch.float32),
    ("e.weight", 4099, torch.float32),
    ("bn.num_batches_tracked", 1, torch.int64),
    ("bn.running_var", 130, torch.float32),
)
# blocks: a 0 | b 1 | c 2 | d 3-4 | e 5-69 | counter 70 | running_var 71-73
SYNTHETIC_COUNTS = [1, 63, 64, 64, 1] + [64] * 64 + [3] + [0] + [0, 0, 0]


def synthetic_layout() -> ParamLayout:
    return ParamLayout.from_tensors(
        (name, torch.zeros((), dtype=dt) if name.endswith("tracked") else torch.zeros(n, dtype=dt))
        for name, n, dt in SYNTHETIC
    )


def arenas(n: int, norm: float, seed: int = 0, device: str = "cpu"):
    """(w, w0): fp32 arenas of n elements whose difference has an L2 norm of about
    ``norm`` over all n elements (padding included: it must come through untouched)."""
    g = torch.Generator().manual_seed(seed)
    w0 = torch.randn(n, generator=g)
    d = torch.randn(n, generator=g)
    w = w0 + d * (norm / math.sqrt(n))
    return w.to(device), w0.to(device)
