"""Worker for tests/test_gpu_attention.py: the fused attention kernels on the whole case list in a fresh process.

    P2PFL_ATTN_WAVES=4 P2PFL_ATTN_LDS_ROWS=0 python tests/attn_variant_worker.py OUT.pt

``csrc/attention.hip`` reads its two switches once per process, so every
compiled arm other than the default (8 waves, row operands staged in LDS) needs
a process of its own.  The worker runs ``attn_fwd`` / ``attn_bwd`` on every
case and saves ``{case: (o, lse, dqkv)}`` (CPU tensors) to ``OUT.pt``; the test
holds them against the fp64 reference and against the default arm's bits.

The module also owns the case list (``cases()`` / ``make_case()``), which the
test imports so that both sides build the same inputs from the same seeds.
Inputs are generated on the CPU: the values do not depend on the device.
"""

from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

B, H, D = 2, 2, 64
C = H * D
# every partial-tile edge of the 32-key tiles, the odd / even token-pair edge of the transposed
# staging, one and two 4-wave blocks (129+), ViT's 197 and the 256 limit
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 197, 224, 225, 255, 256)
FAMILIES = ("random", "uniform", "ascending", "descending", "spike", "large")


def cases():
    return [(f, t) for f in FAMILIES for t in LENGTHS]


def case_id(case) -> str:
    return f"{case[0]}-T{case[1]}"


def _ascending_qk(g, T):
    """q ~ 8u + 0.1 noise, k_t ~ 4.2 (t // 32) u + 0.3 noise: the row max climbs ~6 exponent units per key tile."""
    u = torch.randn(B, 1, H, D, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    q = 8.0 * u + 0.1 * torch.randn(B, T, H, D, generator=g)
    level = (torch.arange(T) // 32).float().view(1, T, 1, 1)
    k = 4.2 * level * u + 0.3 * torch.randn(B, T, H, D, generator=g)
    return q, k


def make_case(family: str, T: int, batch: int = B, heads: int = H, seed: int | None = None):
    """(qkv [batch, T, 3 * heads * 64], do [batch, T, heads * 64]) in bf16 on the CPU, from a fixed seed."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(family) + T if seed is None else seed)
    if family in ("ascending", "descending"):
        assert (batch, heads) == (B, H)
        q, k = _ascending_qk(g, T)
    else:
        amp = 9.0 if family == "large" else 1.5
        q = torch.randn(batch, T, heads, D, generator=g) * amp
        k = torch.randn(batch, T, heads, D, generator=g) * amp
    v = torch.randn(batch, T, heads, D, generator=g) * 1.5
    do = torch.randn(batch, T, heads, D, generator=g)
    if family == "uniform":
        q = torch.zeros_like(q)
    elif family == "descending":
        k, v, do = k.flip(1), v.flip(1), do.flip(1)
    elif family == "spike":  # the dominant key is the row that the kernels' clamped padding duplicates
        k[:, T - 1] = 40.0 * q[:, 0] / q[:, 0].norm(dim=-1, keepdim=True)
    qkv = torch.stack([q, k, v], dim=2).reshape(batch, T, 3 * heads * D).to(torch.bfloat16)
    return qkv, do.reshape(batch, T, heads * D).to(torch.bfloat16)


def run_case(fx, case, device="cuda"):
    """(o, lse, dqkv) of the native kernels for one case, as CPU tensors."""
    qkv, do = (t.to(device) for t in make_case(*case))
    o, lse = fx.attn_fwd(qkv, H)
    dqkv = fx.attn_bwd(qkv, o, do, lse, H)
    return o.cpu(), lse.cpu(), dqkv.cpu()


def main(out: str) -> None:
    from p2pfl_amd import ops

    fx = ops.ext().fused
    res = {case_id(c): run_case(fx, c) for c in cases()}
    torch.cuda.synchronize()
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1])
