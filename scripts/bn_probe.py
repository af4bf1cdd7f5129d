"""Time the BatchNorm launches of csrc/batchnorm.hip at ResNet sizes.

The distinct ``[M, C]`` activations (M = N H W rows of C channels, bf16) that the BatchNorms of
ResNet-18 and ResNet-50 see at bench.py's batch of 32 CIFAR images (3x3 stem, no max-pool):
``fwd_train`` with running statistics, ``bwd`` with ReLU, ``bwd`` with ReLU and a residual
gradient, and ``fwd_eval``, each through the bindings (``ext().bn``), so a call is its launches plus
the output allocations.

    python scripts/bn_probe.py [--iters N] [--fused]

One JSON line per shape, microseconds per call.  ``--fused`` hands the calls an arrival counter
(the one-launch statistics + finalize kernels where the shape is eligible).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from p2pfl_amd import ops  # noqa: E402

# batch 32; rows = 32 H W.  ResNet-18 (BasicBlock): every BN of a stage sees one shape.
# ResNet-50 (Bottleneck): bn1 of a stage's first block still runs at the previous resolution.
SHAPES = {
    "resnet18": [(32768, 64), (8192, 128), (2048, 256), (512, 512)],
    "resnet50": [(32768, 64), (32768, 256), (32768, 128), (8192, 128), (8192, 512), (8192, 256), (2048, 256),
                 (2048, 1024), (2048, 512), (512, 512), (512, 2048)],
}


def timeit(fn, iters, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300, help="timed calls per figure")
    ap.add_argument("--fused", action="store_true", help="pass an arrival counter (one-launch statistics + finalize)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    bn = ops.ext().bn
    done = set()
    for model, shapes in SHAPES.items():
        for M, C in shapes:
            if (M, C) in done:
                continue
            done.add((M, C))
            g = torch.Generator(device=dev).manual_seed(M + C)
            x, res, dy = (torch.randn(M, C, device=dev, generator=g).to(torch.bfloat16) for _ in range(3))
            w, b = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g)
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            nbt = torch.zeros((), dtype=torch.int64, device=dev)
            ctr = torch.zeros(16, dtype=torch.int32, device=dev) if args.fused else None
            y, mean, rstd = bn.fwd_train(x, w, b, res, rm, rv, nbt, 0.1, 1e-5, True, ctr)
            row = {"first_model": model, "M": M, "C": C, "fused_rows": int(bn.fused_rows(M, C)) if args.fused else 0,
                   "fwd_train_us": timeit(lambda: bn.fwd_train(x, w, b, None, rm, rv, nbt, 0.1, 1e-5, True, ctr), args.iters),
                   "bwd_relu_us": timeit(lambda: bn.bwd(dy, y, x, w, mean, rstd, True, False, ctr, None), args.iters),
                   "bwd_relu_res_us": timeit(lambda: bn.bwd(dy, y, x, w, mean, rstd, True, True, ctr, None), args.iters),
                   "fwd_eval_us": timeit(lambda: bn.fwd_eval(x, w, b, None, rm, rv, 1e-5, True), args.iters)}
            print(json.dumps({k: round(v, 2) if isinstance(v, float) else v for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
