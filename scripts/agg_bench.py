"""Robust-aggregation kernels against the weighted sum and against the torch
formulation a user would write without them, at the CNN and ViT-B arena sizes.

Arms per (n, k), alternated in one process, device events around batches of
back-to-back calls, every arm warmed up and timed for >= --seconds in total:

    median        ops.trimmed_mean(flats, (k - 1) // 2)         (k + 1) * 4n bytes
    sqdist        ops.pairwise_sqdist(flats)                    k * 4n bytes
    wsum          ops.weighted_average(flats, w)                (k + 1) * 4n bytes
    torch_median  torch.stack(flats).sort(0) + slice mean
    torch_sqdist  (a - b).square().sum() per pair

    python scripts/agg_bench.py [--seconds 0.3] [--rounds 5] [--out table.md]

Prints one JSON line per point and a markdown table (time per call in us,
min..max over the rounds as the spread, achieved GB/s by the byte counts above).
"""

from __future__ import annotations

import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SIZES = {"cnn": 6_497_216, "vit_b": 86_567_656}
KS = (4, 8, 16)


def batch_us(fn, reps: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps


def torch_median(flats):
    k = len(flats)
    b = (k - 1) // 2
    return torch.stack(flats).sort(0).values[b : k - b].mean(0)


def torch_sqdist(flats):
    k = len(flats)
    d = torch.zeros(k, k, device=flats[0].device)
    for i in range(k):
        for j in range(i + 1, k):
            d[i, j] = d[j, i] = (flats[i] - flats[j]).square().sum()
    return d


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seconds", type=float, default=0.3, help="timed work per arm and point, at least")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the arms (spread = min..max over them)")
    ap.add_argument("--sizes", default="cnn,vit_b")
    ap.add_argument("--out", default=None, help="also write the markdown table here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("agg_bench.py needs a GPU")
    from p2pfl_amd import ops

    ops.ext()
    rows = []
    for name in args.sizes.split(","):
        n = SIZES[name]
        g = torch.Generator(device="cuda").manual_seed(0)
        arenas = [torch.randn(n, device="cuda", generator=g) for _ in range(max(KS))]
        out = torch.empty(n, device="cuda")
        for k in KS:
            flats = arenas[:k]
            w = [float(i % 5 + 1) for i in range(k)]
            arms = {
                "median": (lambda: ops.trimmed_mean(flats, (k - 1) // 2, out=out), (k + 1) * 4 * n),
                "sqdist": (lambda: ops.pairwise_sqdist(flats), k * 4 * n),
                "wsum": (lambda: ops.weighted_average(flats, w, out=out), (k + 1) * 4 * n),
                "torch_median": (lambda: torch_median(flats), (k + 1) * 4 * n),
                "torch_sqdist": (lambda: torch_sqdist(flats), k * 4 * n),
            }
            reps = {}
            for arm, (fn, _) in arms.items():  # warm up, and size the batches
                fn()
                torch.cuda.synchronize()
                t = batch_us(fn, 2)
                reps[arm] = max(1, math.ceil(args.seconds * 1e6 / args.rounds / t))
            samples = {arm: [] for arm in arms}
            for _ in range(args.rounds):
                for arm, (fn, _) in arms.items():
                    samples[arm].append(batch_us(fn, reps[arm]))
            point = {"size": name, "n": n, "k": k}
            for arm, (_, nbytes) in arms.items():
                s = sorted(samples[arm])
                med = s[len(s) // 2]
                point[arm] = {"us": round(med, 1), "min_us": round(s[0], 1), "max_us": round(s[-1], 1),
                              "GBps": round(nbytes / med / 1e3, 1), "calls": reps[arm] * args.rounds}
            print(json.dumps(point), flush=True)
            rows.append(point)
        del arenas, out
        torch.cuda.empty_cache()

    arms = ["median", "sqdist", "wsum", "torch_median", "torch_sqdist"]
    lines = ["| arena | k | " + " | ".join(f"{a} us (min..max) / GB/s" for a in arms) + " | median / wsum | sqdist / wsum |",
             "|---|---|" + "---|" * (len(arms) + 2)]
    for p in rows:
        cells = [f"{p[a]['us']} ({p[a]['min_us']}..{p[a]['max_us']}) / {p[a]['GBps']}" for a in arms]
        lines.append(f"| {p['size']} ({p['n']}) | {p['k']} | " + " | ".join(cells)
                     + f" | {p['median']['us'] / p['wsum']['us']:.2f} | {p['sqdist']['us'] / p['wsum']['us']:.2f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
