"""Time the optimizer launches of csrc/optim.hip at ResNet sizes.

Multi-tensor (`ops.sgd_mt_step` / `ops.adam_mt_step`) on the parameter sets of ResNet-18 and
ResNet-50: conv weights are channels-last (bf16 gradient and shadow in (O, kh, kw, I) order,
fp32 master and state in OIHW order), everything else plain -- the layout the
mixed-precision learner hands them.  Whole-arena (`ops.sgd_step` / `ops.adam_step`) on a flat
fp32 arena of ResNet-50's size with an fp32 gradient, with and without the bf16 shadow.

    python scripts/optim_probe.py [--iters N]

One JSON line per model and one for the whole-arena kernels; every time comes with the
bytes the kernel has to move over that time (TB/s).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from p2pfl_amd import ops  # noqa: E402
from p2pfl_amd.learning.optim import mt_layout  # noqa: E402
from p2pfl_amd.models.resnet import ResNet18, ResNet50  # noqa: E402


class Tables:
    def __init__(self, shapes, dev):
        self.table, off = [], 0
        self.numels, self.grad_bf16, self.grad_cl = [], [], []
        for s in shapes:
            n = int(torch.Size(s).numel())
            flags = 1 | 2
            cl = len(s) == 4 and s[2] * s[3] > 1
            if cl:
                flags |= 4 | (s[1] << 8) | ((s[2] * s[3]) << 32)
            self.table.append((off, n, flags))
            off = (off + n + 63) // 64 * 64
            self.numels.append(n)
            self.grad_bf16.append(True)
            self.grad_cl.append(cl)
        self.numel = off
        self.tens, self.chunks = mt_layout(self.table, dev)


def timeit(fn, iters=50, warm=5):
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


def arena_probe(n, dev, iters):
    """Whole-arena kernels on n fp32 elements.  Bytes per element: SGD reads p, g, buf and writes
    p, buf = 20; Adam reads p, g, m, v and writes p, m, v = 28; the bf16 shadow adds 2."""
    p, g = torch.randn(n, device=dev), torch.randn(n, device=dev)
    buf, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    shadow = torch.zeros(n, device=dev, dtype=torch.bfloat16)
    row = {"model": "resnet50_arena", "params": n}
    for tag, sh, extra in (("", None, 0), ("_shadow", shadow, 2)):
        sgd = timeit(lambda: ops.sgd_step(p, g, buf, lr=0.05, momentum=0.9, weight_decay=5e-4, p_bf16=sh), iters)
        adam = timeit(lambda: ops.adam_step(p, g, m, v, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                                            step=1, p_bf16=sh), iters)
        row.update({f"sgd{tag}_us": round(sgd, 2), f"sgd{tag}_TBps": round((20 + extra) * n / sgd / 1e6, 2),
                    f"adam{tag}_us": round(adam, 2), f"adam{tag}_TBps": round((28 + extra) * n / adam / 1e6, 2)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="timed launches per figure")
    iters = ap.parse_args().iters
    dev = torch.device("cuda")
    for name, net in (("resnet18", ResNet18), ("resnet50", ResNet50)):
        shapes = [tuple(p.shape) for p in net(seed=0).parameters()]
        mt = Tables(shapes, dev)
        p = torch.randn(mt.numel, device=dev)
        buf, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
        shadow = torch.zeros(mt.numel, device=dev, dtype=torch.bfloat16)
        grads = []
        for s in shapes:
            g = torch.randn(s, device=dev).to(torch.bfloat16)
            grads.append(g.contiguous(memory_format=torch.channels_last) if len(s) == 4 and s[2] * s[3] > 1 else g)
        # persistent gradient-address table (as the captured training step uses): no per-call upload
        gtab = torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64, device=dev)
        sgd = timeit(lambda: ops.sgd_mt_step(p, buf, grads, mt, lr=0.05, momentum=0.9, weight_decay=5e-4, p_bf16=shadow,
                                             gtab=gtab), iters)
        adam = timeit(lambda: ops.adam_mt_step(p, m, v, grads, mt, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                                               weight_decay=0.0, step=1, p_bf16=shadow, gtab=gtab), iters)
        n = sum(mt.numels)
        # bytes: SGD reads p, buf (fp32) + grad (bf16), writes p, buf + shadow (bf16) = 20 B / param;
        # Adam reads p, m, v + grad, writes p, m, v + shadow = 28 B / param
        print(json.dumps({"model": name, "params": n, "sgd_mt_us": round(sgd, 2), "sgd_TBps": round(20 * n / sgd / 1e6, 2),
                          "adam_mt_us": round(adam, 2), "adam_TBps": round(28 * n / adam / 1e6, 2)}), flush=True)
        del p, buf, m, v, shadow, grads, gtab
    print(json.dumps(arena_probe(mt.numel, dev, iters)), flush=True)


if __name__ == "__main__":
    main()
