"""Forward-only (evaluation) kernels of the fused CNN: us per kernel and per launch chain.

    python scripts/eval_fwd_probe.py                 128-row launches (P2CNN_CONV2_FWD_LDS=1: the LDS-staged conv2)
    python scripts/eval_fwd_probe.py --rows 128 384 512

With --rows: for every row count R (R images, FC1 on R rows) both FC1 paths -- fc1_eval
in one launch against gemm_skinny<4> x R / 128 chunks -- both conv2 kernels -- the image
loop (at the dispatch rule's images per workgroup and around it) against conv2_fwd_lds x
chunks -- conv1 and the head at R images, and the whole chain both ways.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from p2pfl_amd import ops  # noqa: E402
from p2pfl_amd.learning.fused_cnn import FEAT, HID, FusedCNNEngine, _EvalForward  # noqa: E402
from p2pfl_amd.models import CNN  # noqa: E402
from p2pfl_amd.ops.autotune import _time  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="*", default=None, help="row counts (multiples of 128 up to 512)")
ap.add_argument("--iters", type=int, default=50)
args = ap.parse_args()

ops.ext()
dev = torch.device("cuda")
eng = FusedCNNEngine(CNN(seed=1).cuda(), device=dev)
C = eng.C
bf = torch.bfloat16
RMAX = max(args.rows) if args.rows else 128
g = torch.Generator(device="cuda").manual_seed(0)
x = torch.randint(0, 256, (RMAX, 784), dtype=torch.uint8, device="cuda", generator=g)
y = torch.randint(0, 10, (RMAX,), device="cuda", generator=g)
p1 = torch.zeros(RMAX * 196 * 32, dtype=bf, device=dev)
am1 = torch.zeros(RMAX * 196 * 32, dtype=torch.uint8, device=dev)
a1 = torch.zeros(RMAX * FEAT, dtype=bf, device=dev)
am2 = torch.zeros(RMAX * FEAT, dtype=torch.uint8, device=dev)
slabs = torch.zeros(max(eng.S1 * 128, 4 * RMAX) * HID, device=dev)
H = torch.zeros(RMAX * HID, dtype=bf, device=dev)
dH = torch.zeros(RMAX * HID, dtype=bf, device=dev)
dl = torch.zeros(RMAX * 10, device=dev)
stats = torch.zeros(4, device=dev)
us = lambda f: round(_time(f, args.iters) * 1e3, 2)  # noqa: E731

if not args.rows:
    B, M = 128, 128
    ks = {
        "conv1_fwd": lambda: C.conv1_fwd(x, None, eng.params, eng.off, p1, am1, None, B),
        "conv2_fwd": lambda: C.conv2_fwd(p1, eng.w2r, eng.params, eng.off, a1, am2, B, M),
        "gemm_fc1": lambda: C.gemm_skinny(a1, eng.w1bf, slabs, M, HID, FEAT, eng.S1),
        "head": lambda: C.head(slabs, eng.S1, M, eng.params, eng.off, y, None, B, False, H, dH, dl, stats, eng.w2bf),
    }
    print({"lds_conv2": os.environ.get("P2CNN_CONV2_FWD_LDS", "0"), "us": {k: us(f) for k, f in ks.items()}}, flush=True)
    sys.exit(0)

S = _EvalForward.FC1_SPLITS
idx = torch.arange(RMAX, device=dev)


def chain128(R):  # the 128-row path: R / 128 chains of four launches
    for s in range(0, R, 128):
        C.conv1_fwd(x, idx[s : s + 128], eng.params, eng.off, p1, am1, None, 128)
        C.conv2_fwd(p1, eng.w2r, eng.params, eng.off, a1, am2, 128, 128)
        C.gemm_skinny(a1, eng.w1bf, slabs, 128, HID, FEAT, eng.S1)
        C.head(slabs, eng.S1, 128, eng.params, eng.off, y, idx[s : s + 128], 128, False, H, dH, dl, stats, eng.w2bf)


def chain(R):  # one chain of four launches
    C.conv1_fwd(x, idx[:R], eng.params, eng.off, p1, am1, None, R)
    C.conv2_fwd(p1, eng.w2r, eng.params, eng.off, a1, am2, R, R)
    C.fc1_eval(a1, eng.w1bf, slabs, R, S)
    C.head(slabs, S, R, eng.params, eng.off, y, idx[:R], R, False, H, dH, dl, stats, eng.w2bf)


def times(f, n):  # n back-to-back launches of f as one timed unit
    def run():
        for _ in range(n):
            f()

    return run


for R in args.rows:
    n = R // 128
    C.conv1_fwd(x, None, eng.params, eng.off, p1, am1, None, R)
    C.conv2_fwd_loop(p1, eng.w2r, eng.params, eng.off, a1, am2, R, R, 0)
    ipw0 = C.conv2_loop_ipw(R) if R > 128 else 1
    out = {"rows": R, "chunks": n, "fc1_splits": S}
    out["conv1_us"] = us(lambda: C.conv1_fwd(x, None, eng.params, eng.off, p1, am1, None, R))
    out["conv1_128_x_chunks_us"] = us(times(lambda: C.conv1_fwd(x, None, eng.params, eng.off, p1, am1, None, 128), n))
    for ipw in sorted({max(1, ipw0 - 1), ipw0, ipw0 + 1}):
        out[f"conv2_loop_ipw{ipw}_us"] = us(lambda: C.conv2_fwd_loop(p1, eng.w2r, eng.params, eng.off, a1, am2, R, R, ipw))
    out["conv2_loop_rule_ipw"] = ipw0
    out["conv2_lds_x_chunks_us"] = us(times(lambda: C.conv2_fwd(p1, eng.w2r, eng.params, eng.off, a1, am2, 128, 128), n))
    for s in (1, 2, 4):
        out[f"fc1_eval_S{s}_us"] = us(lambda: C.fc1_eval(a1, eng.w1bf, slabs, R, s))
    out["fc1_eval_tflops"] = round(2.0 * R * HID * FEAT / (out[f"fc1_eval_S{S}_us"] * 1e-6) / 1e12, 1)
    out["gemm_skinny4_x_chunks_us"] = us(times(lambda: C.gemm_skinny(a1, eng.w1bf, slabs, 128, HID, FEAT, eng.S1), n))
    out["head_us"] = us(lambda: C.head(slabs, S, R, eng.params, eng.off, y, None, R, False, H, dH, dl, stats, eng.w2bf))
    out["head_128_x_chunks_us"] = us(times(lambda: C.head(slabs, eng.S1, 128, eng.params, eng.off, y, None, 128, False, H, dH, dl, stats, eng.w2bf), n))
    out["chain_us"] = us(lambda: chain(R))
    out["chain_128_us"] = us(lambda: chain128(R))
    print(json.dumps(out), flush=True)
