"""Adam's step scalars computed once per step by the head launch (MI355X only).

With ``step_scalars`` an engine's training head launch leaves ``lr / (1 - beta1^t)`` and
``1 / sqrt(1 - beta2^t)`` of step ``t = adam_t[0] + t_off`` in a 16-byte device buffer and
every Adam role of the step reads them from there; without it every thread of every role
computes them.  Both come from one device function on the same inputs, so every tensor of
the two arms must be bitwise equal -- eagerly, and in a captured graph replayed with a moved
``adam_t`` base (a scalar fixed at capture would show there).

Loss sums: the head adds the per-sample losses with fp32 atomics, whose order varies from
run to run (also between two runs of one engine; tests/test_gpu_cnn_route_slice.py), so the
loss column of the stats row is compared within the reordering bound of an fp32 sum of B
terms, 2 (B - 1) 2^-24 of the sum (zero at B = 1).  The correct-count column and everything
else are compared bitwise, including the per-sample ``dlogits`` the losses come from.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from p2pfl_amd import ops
from p2pfl_amd.models import CNN

pytestmark = pytest.mark.gpu

N = 160
STATE = ("params", "m", "v", "w1_cur", "w2r", "w2q", "w2bf", "dlogits")


def _data():
    g = torch.Generator(device="cuda").manual_seed(77)
    x = torch.randint(0, 256, (N, 1, 28, 28), dtype=torch.uint8, device="cuda", generator=g).reshape(-1, 784)
    y = torch.randint(0, 10, (N,), device="cuda", generator=g)
    perm = torch.randperm(N, device="cuda", generator=g)
    return x, y, perm


def _engine(step_scalars, **kw):
    from p2pfl_amd.learning.fused_cnn import FusedCNNEngine

    ops.ext()
    eng = FusedCNNEngine(CNN(seed=1234).cuda(), device=torch.device("cuda"), mrows=32, step_scalars=step_scalars, **kw)
    assert (eng.step_scal is not None) == step_scalars
    return eng


def _assert_same(on, off, st_on, st_off, B, what):
    for name in STATE:
        assert torch.equal(getattr(on, name), getattr(off, name)), f"{name} differs {what}"
    assert torch.equal(st_on[1:], st_off[1:]), f"correct count differs {what}"
    a, r = float(st_on[0]), float(st_off[0])
    bound = 2 * (B - 1) * 2.0**-24 * max(abs(a), abs(r))
    print(f"{what}: loss sums {a!r} {r!r} diff {abs(a - r):.3e} bound {bound:.3e}")
    assert abs(a - r) <= bound, (what, a, r)


# (batch, t_off) per step: base 0, then base 170 (a second epoch); the tail batch and B = 1
FIRST = [(32, 1), (32, 2), (12, 3), (1, 4)]
SECOND = [(32, 1), (12, 2), (1, 3)]


@pytest.mark.parametrize("route_slice,fc1_slice,hop", [(288, 448, True), (0, 448, False), (0, 0, False)])
def test_the_two_arms_are_bitwise_equal(route_slice, fc1_slice, hop):
    x, y, perm = _data()
    engs = [_engine(s, route_slice=route_slice, fc1_slice=fc1_slice) for s in (True, False)]
    stats = [torch.zeros((len(FIRST) + len(SECOND), 4), device="cuda") for _ in engs]
    j, s = 0, 0
    for base, steps in ((0, FIRST), (170, SECOND)):
        for e in engs:
            e.adam_t.fill_(base)
        for B, t_off in steps:
            for e, st in zip(engs, stats):
                e.train_step_async(x, y, perm[s : s + B], B, st[j], t_off, hop=hop)
            torch.cuda.synchronize()
            _assert_same(engs[0], engs[1], stats[0][j], stats[1][j], B, f"after step {j} (t = {base + t_off}, B = {B})")
            j, s = j + 1, s + B
    assert float(engs[0].m.abs().sum()) > 0 and not torch.equal(engs[0].params, _engine(False).params)


def test_a_captured_graph_follows_a_moved_step_base():
    x, y, perm = _data()
    plan = [(0, 32), (32, 32), (64, 32), (96, 12)]  # two hopping steps, two in place

    def enqueue(eng, stats):
        for j, (s, b) in enumerate(plan):
            eng.train_step_async(x, y, perm[s : s + b], b, stats[j], j + 1, hop=j < 2)
        assert eng._wp == 0

    warm = _engine(True)  # loads every kernel of the plan before the capture
    enqueue(warm, torch.zeros((4, 4), device="cuda"))
    torch.cuda.synchronize()

    on, off = _engine(True), _engine(False)
    st_on, st_off = torch.zeros((4, 4), device="cuda"), torch.zeros((4, 4), device="cuda")
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        enqueue(on, st_on)
    for base in (0, 85):
        for e, st in ((on, st_on), (off, st_off)):
            e.adam_t.fill_(base)
            st.zero_()
        gr.replay()
        enqueue(off, st_off)
        torch.cuda.synchronize()
        for j, (_, b) in enumerate(plan):
            _assert_same(on, off, st_on[j], st_off[j], b, f"replay at base {base}, step {j}")
    # the second replay moved on from the first one's result
    assert not torch.equal(on.params, warm.params)


def _inline(eng, n):
    """Adam's scalars of steps 1 .. n as the Adam roles compute them inline, [n, 2]."""
    out = torch.zeros(2 * n, device="cuda")
    eng.adam_t.fill_(0)
    eng.C.adam_scal_probe(eng.adam_t, 1, eng.lr, *eng.betas, out)
    torch.cuda.synchronize()
    return out.view(n, 2)


def _head_scalars(eng, x, y, t):
    eng.adam_t.fill_(t - 1)
    eng.step_scal.fill_(-1.0)
    eng.forward(x, y, None, 32, torch.zeros(4, device="cuda"), True, t_off=1)
    return eng.step_scal[:2].clone()


def test_the_buffer_holds_adams_scalars():
    x, y, _ = _data()
    eng = _engine(True)
    lr, b1, b2 = (float(np.float32(v)) for v in (eng.lr, *eng.betas))  # what the kernels see
    stats = torch.zeros(4, device="cuda")
    inline_all = _inline(eng, 1000).cpu()
    worst = 0.0
    for t in (1, 2, 85, 1000):
        got, inline = _head_scalars(eng, x, y, t).cpu(), inline_all[t - 1]
        ref = (lr / (1.0 - b1**t), 1.0 / math.sqrt(1.0 - b2**t))
        rel = [abs(float(v) - r) / r for v, r in zip(inline.tolist(), ref)]
        print(f"t = {t}: buffer {got.tolist()} inline {inline.tolist()} fp64 {ref} inline rel. error {rel}")
        worst = max(worst, *rel)
        # the bound is the inline arm's own error at this t, plus nothing: the same bits
        assert torch.equal(got.view(torch.int32), inline.view(torch.int32)), (t, got, inline)
        assert max(rel) <= 1e-5, (t, rel)
    print(f"largest relative error against fp64: {worst:.3e}")

    # evaluation launches write nothing there: through the engine, and handed the buffer directly
    sentinel = torch.tensor([123.5, -7.25, 3.0, 4.0], device="cuda")
    eng.step_scal.copy_(sentinel)
    eng.forward(x, y, None, 32, stats, False)
    eng.C.head(eng.slabs1, eng.S1, 32, eng.params, eng.off, y, None, 32, False, eng.H, eng.dH, eng.dlogits, stats,
               eng.w2bf, eng.step_scal, eng.adam_t, 1, eng.lr, *eng.betas)
    torch.cuda.synchronize()
    assert torch.equal(eng.step_scal, sentinel)
    # a training step without the step offset (a bare forward) writes none either
    eng.forward(x, y, None, 32, stats, True)
    torch.cuda.synchronize()
    assert torch.equal(eng.step_scal, sentinel)


def test_every_step_of_three_epochs_gets_the_inline_bits():
    """Steps 1 .. 255 (three 85-step epochs): the head's scalars are the inline ones, bit for bit."""
    x, y, _ = _data()
    eng = _engine(True)
    inline = _inline(eng, 255)
    got = torch.stack([_head_scalars(eng, x, y, t) for t in range(1, 256)])
    torch.cuda.synchronize()
    bad = (got.view(torch.int32) != inline.view(torch.int32)).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"steps {[b + 1 for b in bad][:10]}: head {got[bad[0]].tolist()} inline {inline[bad[0]].tolist()}"


def test_the_fc1_bias_gradient_keeps_its_summation_order():
    x, y, perm = _data()
    engs = [_engine(s) for s in (True, False)]
    for e in engs:
        e.gdump = torch.zeros_like(e.params)
        e.train_step_async(x, y, perm[:32], 32, torch.zeros(4, device="cuda"), 1, hop=True)
    torch.cuda.synchronize()
    on, off = engs
    lo = on.off[5]
    sl = slice(lo, lo + 2048)  # l1.bias
    for name in ("gdump", "params", "m", "v"):
        assert torch.equal(getattr(on, name)[sl], getattr(off, name)[sl]), f"l1.bias {name} differs"
    assert torch.equal(on.gdump, off.gdump)
    # the column sums of dH over the samples b = 0 .. 31, in that order, in fp32
    dH = on.dH.view(32, 2048).float()
    g = torch.zeros(2048, device="cuda")
    for b in range(32):
        g = g + dH[b]
    assert torch.equal(on.gdump[sl], g)
    assert float(g.abs().sum()) > 0
