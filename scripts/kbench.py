"""Per-kernel micro-benchmark of the fused CNN step (MI355X).

Times every kernel of one training step in isolation (each launched ``--reps``
times back to back, HIP events around the batch) on the engine's real buffers,
after one full warm-up step so every input holds realistic data.  Meant to be
run directly or under ``rocprofv3 --pmc ... -- python3 scripts/kbench.py``.

    python scripts/kbench.py [--reps 200] [--only route,conv_adam]

``--fc1-slice 0,256,512`` adds, per slice ``n``: the conv2 backward launch hosting
the first ``n`` FC1 tiles (``conv2_bwd_fc1``), the merged Adam launch from tile ``n``
(``fc2_fc1_conv_adam``), their sum, and the graph-captured step of an engine with
``fc1_slice = n`` (``step_graph``; the figure the default is picked from).

``--route-slice 0,128,256`` adds, per routing slice ``r`` (and per ``--fc1-slice`` value
``n``, default the engine's): the routing launch hosting FC1 tiles ``[0, r)``
(``route_rm_fc1``), the conv2 backward launch hosting ``[r, r + n)``, the merged Adam
launch from tile ``r + n``, their sum (``trio``), and the graph-captured step of an engine
with ``route_slice = r, fc1_slice = n``: 20 steps, an even count, so every step hops
between the two W1 shadow buffers.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", default="")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--no-graph", action="store_true", help="skip the graph-captured step (use under --pmc)")
    ap.add_argument("--fc1-slice", default="", help="comma-separated FC1 slices to sweep (see above)")
    ap.add_argument("--route-slice", default="", help="comma-separated routing-launch slices to sweep (see above)")
    args = ap.parse_args()

    from p2pfl_amd.learning.fused_cnn import FusedCNNEngine
    from p2pfl_amd.models import CNN

    dev = torch.device("cuda")
    eng = FusedCNNEngine(CNN(seed=0).to(dev), device=dev)
    C, M, B = eng.C, eng.mrows, args.batch
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randint(0, 256, (B, 1, 28, 28), dtype=torch.uint8, device=dev, generator=g).reshape(-1, 784)
    y = torch.randint(0, 10, (B,), device=dev, generator=g)
    stats = torch.zeros(4, device=dev)
    for _ in range(3):
        eng.train_step_async(x, y, None, B, stats, 1)
    torch.cuda.synchronize()
    a = eng._adam()
    # Adam kernels write into the params: run them on scratch copies so repeated
    # launches do not drift the weights into NaN territory
    P, Mm, V = eng.params.clone(), eng.m.clone(), eng.v.clone()
    w1t = eng.w1bf.view(2048, 3136).t().contiguous()  # for the W1^T-shadow variants
    w2s = torch.zeros(10 * 2048, dtype=torch.bfloat16, device=dev)  # scratch bf16 W2 copy for the Adam arm
    rws = torch.zeros(98 * 2 * M * 32, device=dev)  # split-K routing partials / tickets
    rctr = torch.zeros(98, dtype=torch.int32, device=dev)
    ks = {
        "conv1_fwd": lambda: C.conv1_fwd(x, None, eng.params, eng.off, eng.p1, eng.am1, eng.p1s, B),
        "conv2_fwd": lambda: C.conv2_fwd(eng.p1, eng.w2r, eng.params, eng.off, eng.a1, eng.am2, B, M),
        "conv12_fwd": lambda: C.conv12_fwd(x, None, eng.params, eng.off, eng.w2r, None, eng.am1, eng.p1s, eng.a1, eng.am2, B, M),
        "gemm_fc1": lambda: C.gemm_skinny(eng.a1, eng.w1bf, eng.slabs1, M, 2048, 3136, eng.S1),
        "head": lambda: C.head(eng.slabs1, eng.S1, M, eng.params, eng.off, y, None, B, True, eng.H, eng.dH, eng.dlogits, stats, eng.w2bf),
        "head_w2fp32": lambda: C.head(eng.slabs1, eng.S1, M, eng.params, eng.off, y, None, B, True, eng.H, eng.dH, eng.dlogits, stats),
        "route_fc2": lambda: C.route_fc2(eng.dH, eng.w1_route, eng.am2, M, B, eng.dc2m, eng.gb, eng.dlogits, eng.H, P, Mm, V, None, eng.off, eng.adam_t, 1, *a, True, eng.route_rm),
        "route_dA1_only": lambda: C.route_fc2(eng.dH, eng.w1bf, eng.am2, M, B, eng.dc2m, eng.gb, eng.dlogits, eng.H, P, Mm, V, None, eng.off, eng.adam_t, 1, *a, False, True),
        "route_dA1_split2": lambda: C.route_fc2(eng.dH, eng.w1bf, eng.am2, M, B, eng.dc2m, eng.gb, eng.dlogits, eng.H, P, Mm, V, None, eng.off, eng.adam_t, 1, *a, False, True, rws, rctr),
        "route_dA1_w1t": lambda: C.route_fc2(eng.dH, w1t, eng.am2, M, B, eng.dc2m, eng.gb, eng.dlogits, eng.H, P, Mm, V, None, eng.off, eng.adam_t, 1, *a, False, False),
        "fc1_conv_adam_w1t": lambda: C.fc1_conv_adam(eng.dH, eng.a1, M, eng.wslab1, eng.wslab2, eng.gb, B, P, Mm, V, None, eng.w1bf, w1t, eng.w2r, eng.w2q, eng.off, eng.adam_t, 1, *a, eng.dlogits, eng.H),
        "fc1_conv_adam": lambda: C.fc1_conv_adam(eng.dH, eng.a1, M, eng.wslab1, eng.wslab2, eng.gb, B, P, Mm, V, None, eng.w1bf, eng.w1tbf, eng.w2r, eng.w2q, eng.off, eng.adam_t, 1, *a),
        "fc2_fc1_conv_adam": lambda: C.fc1_conv_adam(eng.dH, eng.a1, M, eng.wslab1, eng.wslab2, eng.gb, B, P, Mm, V, None, eng.w1bf, eng.w1tbf, eng.w2r, eng.w2q, eng.off, eng.adam_t, 1, *a, eng.dlogits, eng.H, w2s),
        "fc1_wgrad_adam": lambda: C.fc1_wgrad_adam(eng.dH, eng.a1, M, P, Mm, V, None, eng.w1bf, eng.w1tbf, eng.off, eng.adam_t, 1, *a),
        "conv2_bwd": lambda: C.conv2_bwd(eng.dc2m, eng.p1s, eng.am1, eng.w2q, x, None, eng.wslab1, eng.wslab2, B),
        "conv_adam": lambda: C.conv_adam(eng.wslab1, eng.wslab2, eng.gb, B, P, Mm, V, None, eng.w2r, eng.w2q, eng.off, eng.adam_t, 1, *a),
    }
    only = [s for s in args.only.split(",") if s]

    def timeit(fn) -> float:
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) * 1000.0 / args.reps, 2)

    def step_graph() -> float:
        """One step of ``eng`` as it is configured now: 20 captured, 5 replays."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        hop = eng.hop_steps(20) == 20  # an even plan: every step hops when the routing launch hosts tiles
        with torch.cuda.stream(s):
            for _ in range(2):
                eng.train_step_async(x, y, None, B, stats, 1, hop=hop)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(20):
                eng.train_step_async(x, y, None, B, stats, 1, hop=hop)
        gr.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) * 1000.0 / 100, 2)

    res = {}
    for name, fn in ks.items():
        if only and not any(o in name for o in only):
            continue
        res[name] = timeit(fn)
    # whole step, graph-captured, for reference
    if not only and not args.no_graph:
        res["step_graph"] = step_graph()
    slices = {}
    fc1_slices = [int(v) for v in args.fc1_slice.split(",") if v]
    route_slices = [int(v) for v in args.route_slice.split(",") if v]
    routes = {}
    for n in (fc1_slices or [eng.fc1_slice]) if route_slices else []:
        for r in route_slices:
            if r + n > 1600:
                continue
            w1w = eng._w1s[1]  # the hosted tiles write the shadow buffer the routing blocks do not read
            t = {
                "route_rm_fc1": timeit(lambda: C.route_rm_fc1(eng.dH, eng.w1bf, eng.am2, M, B, eng.dc2m, eng.gb, eng.dlogits, eng.H, P, Mm, V, None, eng.off, eng.adam_t, 1, *a, False, eng.a1, w1w, r)),
                "conv2_bwd_fc1": timeit(lambda: C.conv2_bwd_fc1(eng.dc2m, eng.p1s, eng.am1, eng.w2q, x, None, eng.wslab1, eng.wslab2, B, eng.dH, eng.a1, M, P, Mm, V, None, w1w, None, eng.off, eng.adam_t, 1, *a, n, r)),
                "fc2_fc1_conv_adam": timeit(lambda: C.fc1_conv_adam(eng.dH, eng.a1, M, eng.wslab1, eng.wslab2, eng.gb, B, P, Mm, V, None, w1w, None, eng.w2r, eng.w2q, eng.off, eng.adam_t, 1, *a, eng.dlogits, eng.H, w2s, r + n)),
            }
            t["trio"] = round(sum(t.values()), 2)
            if not args.no_graph:
                keep = eng.fc1_slice, eng.route_slice
                eng.fc1_slice, eng.route_slice = n, r
                t["step_graph"] = step_graph()
                eng.fc1_slice, eng.route_slice = keep
            routes[f"{r}+{n}"] = t
    for n in [] if route_slices else fc1_slices:
        r = {
            "conv2_bwd_fc1": timeit(lambda: C.conv2_bwd_fc1(eng.dc2m, eng.p1s, eng.am1, eng.w2q, x, None, eng.wslab1, eng.wslab2, B, eng.dH, eng.a1, M, P, Mm, V, None, eng.w1bf, eng.w1tbf, eng.off, eng.adam_t, 1, *a, n)),
            "fc2_fc1_conv_adam": timeit(lambda: C.fc1_conv_adam(eng.dH, eng.a1, M, eng.wslab1, eng.wslab2, eng.gb, B, P, Mm, V, None, eng.w1bf, eng.w1tbf, eng.w2r, eng.w2q, eng.off, eng.adam_t, 1, *a, eng.dlogits, eng.H, w2s, n)),
        }
        r["pair"] = round(r["conv2_bwd_fc1"] + r["fc2_fc1_conv_adam"], 2)
        if not args.no_graph:
            keep, eng.fc1_slice = eng.fc1_slice, n
            r["step_graph"] = step_graph()
            eng.fc1_slice = keep
        slices[n] = r
    if not only:
        res["sum_isolated"] = round(sum(v for k, v in res.items() if k in ("conv1_fwd", "conv2_fwd", "gemm_fc1", "head", "route_dA1_split2" if eng.route_ws is not None else "route_dA1_only", "conv2_bwd", "fc2_fc1_conv_adam")), 2)
    out = {"us_per_kernel": res, "batch": B}
    if slices:
        out["fc1_slice"] = slices
    if routes:
        out["route+fc1_slice"] = routes
    print(json.dumps(out))


if __name__ == "__main__":
    main()
