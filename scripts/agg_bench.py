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
    python scripts/agg_bench.py --q8 ...    the q8 wire kernels beside the k = 1 weighted sum (q8_main)
    python scripts/agg_bench.py --dp ...    the differential-privacy kernels beside the k = 2 weighted sum (dp_main)

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


def q8_main(args) -> None:
    """--q8: the q8 wire kernels beside the k = 1 weighted sum, at the arenas of
    the MNIST CNN and of ResNet-50 with their own raw-block tables.

        q8_encode     fp32 arena -> packed             4n + packed bytes
        q8_decode     packed -> fp32 arena             packed + 4n bytes
        wsum_k1       ops.weighted_average([x], [1])   8n bytes
        q8_*_r0       the same without raw blocks: the main launch alone
    """
    from p2pfl_amd import ops
    from p2pfl_amd.learning.arena import flatten, q8_raw_blocks, q8_raw_table
    from p2pfl_amd.models import CNN
    from p2pfl_amd.models.resnet import ResNet50

    rows = []
    for name, make in (("cnn", CNN), ("resnet50", ResNet50)):
        layout = flatten(make().state_dict()).layout
        n, raw = layout.numel, q8_raw_table(layout, "cuda")
        n_raw = len(q8_raw_blocks(layout))
        nbytes = ops.q8_packed_nbytes(n, n_raw)
        x = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        out = torch.empty(n, device="cuda")
        packed = ops.q8_encode(x, raw)
        packed0 = ops.q8_encode(x)  # no raw blocks: the main launch alone
        arms = {
            "q8_encode": (lambda: ops.q8_encode(x, raw, out=packed), 4 * n + nbytes),
            "q8_decode": (lambda: ops.q8_decode(packed, n, raw, out=out), nbytes + 4 * n),
            "wsum_k1": (lambda: ops.weighted_average([x], [1.0], out=out), 8 * n),
            "q8_encode_r0": (lambda: ops.q8_encode(x, out=packed0), 4 * n + packed0.numel()),
            "q8_decode_r0": (lambda: ops.q8_decode(packed0, n, out=out), packed0.numel() + 4 * n),
        }
        reps = {}
        for arm, (fn, _) in arms.items():
            fn()
            torch.cuda.synchronize()
            reps[arm] = max(1, math.ceil(args.seconds * 1e6 / args.rounds / batch_us(fn, 2)))
        samples = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm, (fn, _) in arms.items():
                samples[arm].append(batch_us(fn, reps[arm]))
        point = {"size": name, "n": n, "raw_blocks": n_raw, "packed_bytes": nbytes}
        for arm, (_, moved) in arms.items():
            s = sorted(samples[arm])
            med = s[len(s) // 2]
            point[arm] = {"us": round(med, 1), "min_us": round(s[0], 1), "max_us": round(s[-1], 1),
                          "GBps": round(moved / med / 1e3, 1), "calls": reps[arm] * args.rounds}
        print(json.dumps(point), flush=True)
        rows.append(point)
        del x, out, packed, packed0
        torch.cuda.empty_cache()
    arms = ["q8_encode", "q8_decode", "wsum_k1", "q8_encode_r0", "q8_decode_r0"]
    lines = ["| arena | raw blocks | packed / fp32 bytes | " + " | ".join(f"{a} us (min..max) / GB/s" for a in arms)
             + " | encode / wsum | decode / wsum |", "|---|---|---|" + "---|" * (len(arms) + 2)]
    for p in rows:
        cells = [f"{p[a]['us']} ({p[a]['min_us']}..{p[a]['max_us']}) / {p[a]['GBps']}" for a in arms]
        lines.append(f"| {p['size']} ({p['n']}) | {p['raw_blocks']} | {p['packed_bytes'] / (4 * p['n']):.4f} | "
                     + " | ".join(cells) + f" | {p['q8_encode']['us'] / p['wsum_k1']['us']:.2f} | "
                     f"{p['q8_decode']['us'] / p['wsum_k1']['us']:.2f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


def dp_main(args) -> None:
    """--dp: the differential-privacy kernels beside the k = 2 weighted sum (which
    moves the same 12n bytes as the clipping apply pass), at the arenas of the
    MNIST CNN and of ResNet-50 with their own block tables.

        dp_sqnorm       ops.dp_delta_sqnorm(w, w0, table)            8n bytes
        dp_apply_id     ops.dp_apply, z = 0, update inside the clip  8n + n/64   (w0 is not read)
        dp_apply_clip   ops.dp_apply, z = 0, update clipped          12n + n/64
        dp_apply_noise  ops.dp_apply, z = 1, update clipped          12n + n/64
        wsum_k2         ops.weighted_average([w, w0], [1, 1])        12n bytes
    """
    from p2pfl_amd import ops
    from p2pfl_amd.learning.arena import DP_EXEMPT, dp_block_table, flatten
    from p2pfl_amd.models import CNN
    from p2pfl_amd.models.resnet import ResNet50

    rows = []
    for name, make in (("cnn", CNN), ("resnet50", ResNet50)):
        layout = flatten(make().state_dict()).layout
        n, table = layout.numel, dp_block_table(layout, DP_EXEMPT, "cuda")
        g = torch.Generator(device="cuda").manual_seed(0)
        w0 = torch.randn(n, device="cuda", generator=g)
        w = w0 + 0.01 * torch.randn(n, device="cuda", generator=g)
        out = torch.empty(n, device="cuda")
        ss = ops.dp_delta_sqnorm(w, w0, table)
        norm = math.sqrt(float(ss))
        arms = {
            "dp_sqnorm": (lambda: ops.dp_delta_sqnorm(w, w0, table), 8 * n),
            "dp_apply_id": (lambda: ops.dp_apply(w, w0, table, ss, 2 * norm, 0.0, 1, 0, out=out), 8 * n + n // 64),
            "dp_apply_clip": (lambda: ops.dp_apply(w, w0, table, ss, norm / 2, 0.0, 1, 0, out=out), 12 * n + n // 64),
            "dp_apply_noise": (lambda: ops.dp_apply(w, w0, table, ss, norm / 2, 1.0, 1, 0, out=out), 12 * n + n // 64),
            "wsum_k2": (lambda: ops.weighted_average([w, w0], [1.0, 1.0], out=out), 12 * n),
        }
        reps = {}
        for arm, (fn, _) in arms.items():
            fn()
            torch.cuda.synchronize()
            reps[arm] = max(1, math.ceil(args.seconds * 1e6 / args.rounds / batch_us(fn, 2)))
        samples = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm, (fn, _) in arms.items():
                samples[arm].append(batch_us(fn, reps[arm]))
        point = {"size": name, "n": n, "covered": int(table.sum())}
        for arm, (_, moved) in arms.items():
            s = sorted(samples[arm])
            med = s[len(s) // 2]
            point[arm] = {"us": round(med, 1), "min_us": round(s[0], 1), "max_us": round(s[-1], 1),
                          "GBps": round(moved / med / 1e3, 1), "calls": reps[arm] * args.rounds}
        print(json.dumps(point), flush=True)
        rows.append(point)
        del w, w0, out
        torch.cuda.empty_cache()
    arms = ["dp_sqnorm", "dp_apply_id", "dp_apply_clip", "dp_apply_noise", "wsum_k2"]
    lines = ["| arena | covered elements | " + " | ".join(f"{a} us (min..max) / GB/s" for a in arms)
             + " | sqnorm / wsum | clip / wsum | noise / wsum | noise / clip |", "|---|---|" + "---|" * (len(arms) + 4)]
    for p in rows:
        cells = [f"{p[a]['us']} ({p[a]['min_us']}..{p[a]['max_us']}) / {p[a]['GBps']}" for a in arms]
        ws = p["wsum_k2"]["us"]
        lines.append(f"| {p['size']} ({p['n']}) | {p['covered']} | " + " | ".join(cells)
                     + f" | {p['dp_sqnorm']['us'] / ws:.2f} | {p['dp_apply_clip']['us'] / ws:.2f} | "
                     f"{p['dp_apply_noise']['us'] / ws:.2f} | {p['dp_apply_noise']['us'] / p['dp_apply_clip']['us']:.2f} |")
    table_md = "\n".join(lines)
    print(table_md)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table_md + "\n")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--dp", action="store_true",
                    help="time ops.dp_delta_sqnorm / ops.dp_apply beside the k = 2 weighted sum instead (CNN and ResNet-50 arenas)")
    ap.add_argument("--q8", action="store_true",
                    help="time ops.q8_encode / ops.q8_decode beside the k = 1 weighted sum instead (CNN and ResNet-50 arenas)")
    ap.add_argument("--seconds", type=float, default=0.3, help="timed work per arm and point, at least")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the arms (spread = min..max over them)")
    ap.add_argument("--sizes", default="cnn,vit_b")
    ap.add_argument("--out", default=None, help="also write the markdown table here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("agg_bench.py needs a GPU")
    from p2pfl_amd import ops

    ops.ext()
    if args.q8:
        return q8_main(args)
    if args.dp:
        return dp_main(args)
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
