"""Where a native GEMM launch's time goes on the ViT products: the kernel with its
timing-probe variant bits (no C stores / no K loop / no DMA after the prologue),
device time per launch (HIP events behind a spin kernel, as ops/autotune.py
times, so host launch overhead is excluded), next to hipBLASLt.

    python scripts/gemm_anatomy.py [--out gpurun_out/gemm_anatomy.md]

Probe bits (ops/variant.py PROBE_*): the 128-tile kernels of gemm_core.h only; the
ping-pong kernels carry none (their recorded anatomy: profiles/r3_gemm_pingpong.md,
profiles/r5_vit_gemm_sweep.md).  Probe timings are not correct outputs.
"""

from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from p2pfl_amd.ops import autotune  # noqa: E402
from p2pfl_amd.ops.gemm import gemm  # noqa: E402
from p2pfl_amd.ops.variant import (A_PANEL, PP, PP_M16, PROBE_NO_DMA, PROBE_NO_KLOOP, PROBE_NO_STORE, RING4,  # noqa: E402
                                   SINGLE_BUF)


def dev_time(fn, iters=20) -> float:
    return autotune._time(fn, iters) * 1e3  # us


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bf = torch.bfloat16
    torch.manual_seed(0)
    shapes = [("qkv fwd", 6304, 2304, 768), ("proj fwd", 6304, 768, 768), ("fc2 fwd", 6304, 768, 3072),
              ("fc1 fwd", 6304, 3072, 768), ("square 4096", 4096, 4096, 4096)]
    kernels = [
        ("pingpong", PP, {"full": 0}),
        ("pingpong16", PP | PP_M16, {"full": 0}),
        ("128 dbuf", A_PANEL, {"full": 0, "no stores": PROBE_NO_STORE, "no K loop": PROBE_NO_KLOOP, "no DMA in loop": PROBE_NO_DMA}),
        ("128 1buf", A_PANEL | SINGLE_BUF, {"full": 0, "no stores": PROBE_NO_STORE, "no K loop": PROBE_NO_KLOOP}),
        ("128 ring4", RING4 | A_PANEL, {"full": 0, "no stores": PROBE_NO_STORE, "no K loop": PROBE_NO_KLOOP}),
    ]
    cols = ["full", "no stores", "no K loop", "no DMA in loop"]
    lines = ["| product | kernel | " + " | ".join(cols) + " | hipBLASLt |", "|---|---|" + "---:|" * (len(cols) + 1)]
    for name, M, N, K in shapes:
        a = torch.randn(M, K, device="cuda").to(bf)
        b = (torch.randn(N, K, device="cuda") * 0.02).to(bf)
        lib = dev_time(lambda: torch.mm(a, b.t()))
        c = torch.empty(M, N, device="cuda", dtype=bf)
        fill = dev_time(lambda: c.fill_(1.0))
        lines.append(f"| {name} {M}x{N}x{K} | torch fill_ of C ({M * N * 2 / 1e6:.1f} MB) | {fill:.1f} ({M * N * 2 / fill / 1e6:.2f} TB/s) | | | | |")
        fl = 2.0 * M * N * K
        for kname, v, probes in kernels:
            cells = []
            for col in cols:
                if col not in probes:
                    cells.append("-")
                    continue
                t = dev_time(lambda: gemm(a, b, variant=v | probes[col]))
                cells.append(f"{t:.1f}" + (f" ({fl / t / 1e6:.0f} TF)" if col == "full" else ""))
            lines.append(f"| {name} {M}x{N}x{K} | {kname} | " + " | ".join(cells) + f" | {lib:.1f} ({fl / lib / 1e6:.0f} TF) |")
            print(lines[-1], flush=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
