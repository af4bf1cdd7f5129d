"""LayerNorm kernels at the ViT-B/16 training shape (6304 x 768, bf16): forward
with and without the fused residual add, and the backward, device time per
call (HIP events over back-to-back calls).

    python scripts/ln_bench.py [--reps 200] [--all]

``--all`` adds the other ops of ``csrc/fused_ops.hip`` at the same step's shapes:
bias+GELU forward and backward and the linear bias gradient's column sums at
6304 x 3072, softmax cross-entropy forward + backward at 64 x 1000.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1000.0 / reps, 2)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--all", action="store_true", help="also bias+GELU, column_sum and softmax cross-entropy")
    args = ap.parse_args()
    from p2pfl_amd.ops import fused

    def t(fn):
        return timed(fn, args.reps, args.warmup)

    N, C = 6304, 768
    x = torch.randn(N, C, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    r = torch.randn(N, C, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    w = torch.randn(C, device="cuda", requires_grad=True)
    b = torch.randn(C, device="cuda", requires_grad=True)
    dy = torch.randn(N, C, device="cuda", dtype=torch.bfloat16)
    res = {}
    with torch.no_grad():
        res["ln_fwd"] = t(lambda: fused.layer_norm(x, w, b))
        res["add_ln_fwd"] = t(lambda: fused.add_layer_norm(x, r, w, b))
    res["ln_fwd_bwd"] = t(lambda: torch.autograd.grad(fused.layer_norm(x, w, b), (x, w, b), dy))
    res["bytes_ln_fwd_MB"] = round(2 * N * C * 2 / 1e6, 1)
    if args.all:
        H = 3072
        xh = torch.randn(N, H, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        bh = torch.randn(H, device="cuda", requires_grad=True)
        dyh = torch.randn(N, H, device="cuda", dtype=torch.bfloat16)
        with torch.no_grad():
            res["bias_gelu_fwd"] = t(lambda: fused.bias_gelu(xh, bh))
        yh = fused.bias_gelu(xh, bh)
        res["bias_gelu_bwd"] = t(lambda: torch.autograd.grad(yh, (xh, bh), dyh, retain_graph=True))
        with torch.no_grad():
            res["column_sum"] = t(lambda: fused._fx().column_sum(dyh, False))
        z = torch.randn(64, 1000, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        lab = torch.randint(0, 1000, (64,), device="cuda")
        res["softmax_xent_fwd_bwd"] = t(lambda: torch.autograd.grad(fused.softmax_xent(z, lab), (z,)))
    print(json.dumps({"us_per_call": res}))


if __name__ == "__main__":
    main()
