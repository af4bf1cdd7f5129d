"""FC1 weight-gradient + Adam tiles hosted by the dA1 routing launch (MI355X only).

An engine with ``route_slice = n`` runs FC1 tiles ``[0, n)`` as extra blocks of the
routing launch (``route_rm_fc1``), ``[n, n + fc1_slice)`` in the conv2 backward launch
and the rest in ``fc1_conv_adam``.  Routing reads the row-major W1 shadow, so such a step
"hops": it reads one of two shadow buffers and every tile writes the other.  A tile is
computed by the same device function in every launch, and a plan hops an even number of
times, so every tensor must be bitwise what in-place steps with nothing hosted give, and
the current shadow is buffer 0 (``eng.w1bf``) when the plan ends.

Loss sums: the head adds the per-sample losses with fp32 atomics, whose order varies
from run to run (also between two runs of the same engine), so two correct runs can
differ by a reordering of that sum (measured on MI355X: about half of the step sums of
two such runs differ, by 1 ulp, e.g. 77.275925 against 77.275932).  The loss column is
therefore compared within the
reordering bound of an fp32 sum of B non-negative terms, 2 (B - 1) 2^-24 of the sum;
the correct-count column (exact integers) and everything else are compared bitwise,
including the per-sample ``dlogits`` the losses come from.
"""

from __future__ import annotations

import functools

import pytest
import torch

from p2pfl_amd import ops
from p2pfl_amd.models import CNN

pytestmark = pytest.mark.gpu

TENSORS = ("params", "m", "v", "w1bf", "w2r", "w2q", "w2bf")
# 4 even steps; 5 steps with a ragged last one: odd, so the last step runs in place
PLANS = {
    "even": (32, [(0, 32), (32, 32), (64, 32), (96, 32)]),
    "odd": (32, [(0, 32), (32, 32), (64, 32), (96, 32), (128, 12)]),
    "rows64": (64, [(0, 40), (40, 40), (80, 40), (120, 40)]),
}
# (route_slice, fc1_slice): one tile; an odd count; a typical pair; the Adam launch left
# without an FC1 tile; every tile in the routing launch
PAIRS = [(1, 0), (97, 384), (276, 384), (1216, 384), (1600, 0)]


def _batch(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(0, 256, (n, 1, 28, 28), dtype=torch.uint8, device="cuda", generator=g)
    y = torch.randint(0, 10, (n,), device="cuda", generator=g)
    perm = torch.randperm(n, device="cuda", generator=g)
    return x.reshape(-1, 784), y, perm


def _engine(seed=5, **kw):
    from p2pfl_amd.learning.fused_cnn import FusedCNNEngine

    ops.ext()
    return FusedCNNEngine(CNN(seed=seed).cuda(), device=torch.device("cuda"), **kw)


def _enqueue(eng, plan, x, y, perm, stats, after_first=None):
    """The plan's steps as the learner enqueues them: the leading even count hops."""
    hops = eng.hop_steps(len(plan))
    for j, (s, b) in enumerate(plan):
        eng.train_step_async(x, y, perm[s : s + b], b, stats[j], j + 1, hop=j < hops)
        if j == 0 and after_first is not None:
            after_first()
    assert eng._wp == 0, "a plan ends on shadow buffer 0"


def _run(plan_name, route_slice, fc1_slice):
    mrows, plan = PLANS[plan_name]
    n = plan[-1][0] + plan[-1][1]
    x, y, perm = _batch(n, seed=31)
    eng = _engine(mrows=mrows, route_slice=route_slice, fc1_slice=fc1_slice)
    assert (eng.route_slice, eng.fc1_slice) == (route_slice, fc1_slice)
    assert eng.hop_steps(len(plan)) == (len(plan) - len(plan) % 2 if route_slice else 0)
    stats = torch.zeros((len(plan), 4), device="cuda")
    out = {}

    def first():
        torch.cuda.synchronize()
        out["dc2m"], out["gb"] = eng.dc2m.clone(), eng.gb.clone()

    _enqueue(eng, plan, x, y, perm, stats, after_first=first)
    torch.cuda.synchronize()
    out.update({name: getattr(eng, name).clone() for name in TENSORS})
    out["dlogits"], out["stats"] = eng.dlogits.clone(), stats.clone()
    # what pack_shadows makes of the final parameters, in a scratch engine
    scratch = _engine(seed=1, mrows=mrows)
    scratch.params.copy_(eng.params)
    scratch.pack_shadows()
    torch.cuda.synchronize()
    out["packed_w1bf"] = scratch.w1bf.clone()
    return out


@functools.lru_cache(maxsize=None)
def _in_place(plan_name):
    """Nothing hosted anywhere, every step in place: computed once per plan, only read."""
    return _run(plan_name, 0, 0)


def _assert_stats(got, ref, plan):
    assert torch.equal(got[:, 1:], ref[:, 1:]), "correct counts differ"
    for j, (_, b) in enumerate(plan):
        a, r = float(got[j, 0]), float(ref[j, 0])
        bound = 2 * (b - 1) * 2.0**-24 * max(abs(a), abs(r))
        print(f"step {j} loss sums {a!r} {r!r} diff {abs(a - r):.3e} bound {bound:.3e}")
        assert abs(a - r) <= bound, (j, a, r)


def _check(plan_name, route_slice, fc1_slice):
    ref, got = _in_place(plan_name), _run(plan_name, route_slice, fc1_slice)
    for name in TENSORS + ("dc2m", "gb", "dlogits"):
        assert torch.equal(got[name], ref[name]), f"{name} differs ({plan_name}, {route_slice}, {fc1_slice})"
    _assert_stats(got["stats"], ref["stats"], PLANS[plan_name][1])
    # buffer 0 is the current shadow when the plan ends
    assert torch.equal(got["w1bf"], got["packed_w1bf"])
    assert torch.equal(ref["w1bf"], ref["packed_w1bf"])


@pytest.mark.parametrize("plan_name", ["even", "odd"])
@pytest.mark.parametrize("route_slice,fc1_slice", PAIRS)
def test_route_hosted_tiles_are_bitwise_the_in_place_step(route_slice, fc1_slice, plan_name):
    _check(plan_name, route_slice, fc1_slice)


def test_route_hosted_tiles_with_64_row_launches():
    _check("rows64", 97, 384)


def test_in_place_reference_moved_every_fc1_tile():
    """Guard for the comparisons above: the plan changes the bf16 shadow inside every one
    of the 1600 tiles, so a tile that no launch ran would show as a difference."""
    before = _engine().w1bf.view(64, 32, 3136)
    after = _in_place("even")["w1bf"].view(64, 32, 3136)
    moved = torch.stack([(before != after)[:, :, k : k + 128].any(dim=2).any(dim=1) for k in range(0, 3136, 128)])
    assert moved.shape == (25, 64) and bool(moved.all())


def test_binding_rejects_tiles_that_write_the_shadow_routing_reads():
    eng = _engine(seed=3)
    x, y, _ = _batch(32, seed=1)
    a = eng._adam()
    eng.forward(x, y, None, 32, torch.zeros(4, device="cuda"), True)
    torch.cuda.synchronize()
    before = eng.params.clone()

    def route(w1_write, n_tiles):
        return eng.C.route_rm_fc1(eng.dH, eng.w1bf, eng.am2, 32, 32, eng.dc2m, eng.gb, eng.dlogits, eng.H, eng.params,
                                  eng.m, eng.v, None, eng.off, eng.adam_t, 1, *a, False, eng.a1, w1_write, n_tiles)

    with pytest.raises(RuntimeError, match="other W1 shadow"):
        route(eng.w1bf, 1)
    with pytest.raises(RuntimeError, match="n_tiles"):
        route(eng._w1s[1], 1601)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, before), "a rejected call must not launch"
    assert route(eng.w1bf, 0) == 0  # nothing hosted: the plain routing launch, same buffer allowed
    torch.cuda.synchronize()


def test_route_slice_range_and_environment(monkeypatch):
    with pytest.raises(ValueError):
        _engine(route_slice=-1)
    with pytest.raises(ValueError):
        _engine(route_slice=1601, fc1_slice=0)
    with pytest.raises(ValueError):
        _engine(route_slice=1217, fc1_slice=384)
    assert _engine(route_slice=1216, fc1_slice=384).route_slice == 1216
    monkeypatch.setenv("P2PFL_CNN_ROUTE_SLICE", "77")
    assert _engine().route_slice == 77
    assert _engine(route_slice=0).route_slice == 0
    monkeypatch.setenv("P2PFL_CNN_ROUTE_SLICE", "1300")
    with pytest.raises(ValueError):
        _engine(fc1_slice=384)


def test_captured_hopping_plan_replays_bitwise():
    """A 5-step plan (4 hops + an in-place ragged step) captured in one graph and replayed
    twice against the same ten steps launched eagerly: every replay starts on buffer 0."""
    _, plan = PLANS["odd"]
    x, y, perm = _batch(140, seed=32)
    stats = torch.zeros((len(plan), 4), device="cuda")
    eager = _engine(seed=6, route_slice=97, fc1_slice=384)
    for _ in range(2):
        _enqueue(eager, plan, x, y, perm, stats)
    torch.cuda.synchronize()
    eng = _engine(seed=6, route_slice=97, fc1_slice=384)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="relaxed"):
        _enqueue(eng, plan, x, y, perm, stats)
    torch.cuda.synchronize()
    assert torch.equal(eng.m, torch.zeros_like(eng.m)), "recording a capture must execute nothing"
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for name in TENSORS:
        assert torch.equal(getattr(eng, name), getattr(eager, name)), name


def test_learner_fit_with_and_without_the_route_slice(monkeypatch):
    """Two epochs over a 140-sample shard (5 steps, ragged last one; the epoch graph
    replays from buffer 0 both times) with the default route slice and with none:
    the same parameters, and the same validation / test metrics -- the evaluation
    snapshot reads the current shadow."""
    from p2pfl_amd.data import MnistFederatedDM
    from p2pfl_amd.data.datamodule import FederatedDataModule
    from p2pfl_amd.data.synthetic import ImageSet
    from p2pfl_amd.learning.fused_cnn import FusedCNNLearner

    ops.ext()
    base = MnistFederatedDM(sub_id=0, number_sub=40)
    cut = lambda ld, n: ImageSet(ld.x[:n].cpu(), ld.y[:n].cpu())  # noqa: E731
    got = []
    for route_slice in (None, "0"):
        if route_slice is not None:
            monkeypatch.setenv("P2PFL_CNN_ROUTE_SLICE", route_slice)
        dm = FederatedDataModule(cut(base.train_loader, 140), cut(base.val_loader, 40), cut(base.test_loader, 100),
                                 batch_size=32, seed=3)
        ln = FusedCNNLearner(CNN(seed=13), dm, f"rs-{route_slice}", 2, device=torch.device("cuda"))
        if route_slice is not None:
            assert ln.engine.route_slice == 0
        seen = {}
        ln._log = lambda k, v, step=None, _s=seen: _s.__setitem__(k, v)  # noqa: E731
        ln.fit()
        assert ln.drain(60)
        params = ln.get_parameters().flat.clone()
        test = ln.evaluate()
        assert ln.engine._wp == 0
        got.append((params, seen["val_loss"], seen["val_metric"], test["test_loss"], test["test_metric"]))
    assert torch.equal(got[0][0], got[1][0])
    assert got[0][2] == got[1][2] and got[0][4] == got[1][4]
    # mean losses over 40 / 100 samples, summed by fp32 atomics in any order (see the module docstring)
    for i, n in ((1, 40), (3, 100)):
        a, r = got[0][i], got[1][i]
        print(f"loss {a!r} {r!r} diff {abs(a - r):.3e}")
        assert abs(a - r) <= 2 * (n - 1) * 2.0**-24 * max(abs(a), abs(r)), (i, a, r)
