"""FC1 weight-gradient + Adam tiles hosted by the conv2 backward launch (MI355X only).

``conv2_bwd_fc1(..., n_tiles)`` runs the first ``n_tiles`` of the 1600 FC1 tiles
as extra blocks of the conv2 backward launch and ``fc1_conv_adam(..., first_tile)``
the rest.  A tile is computed by the same device function in either launch, so
every tensor the two launches write must be bitwise what the separate launches
(``conv2_bwd`` + the whole ``fc1_conv_adam``) give.
"""

from __future__ import annotations

import functools

import pytest
import torch

from p2pfl_amd import ops
from p2pfl_amd.models import CNN

pytestmark = pytest.mark.gpu

# 0 / everything; the bias tile (bx == 0) alone; up to, through and past the ragged
# last feature tile (bx == 24) of row 0, i.e. a row boundary; all but the last tile
SLICES = [0, 1, 24, 25, 26, 1599, 1600]
OP_TENSORS = ("params", "m", "v", "w1bf", "w2r", "w2q", "w2bf", "wslab1", "wslab2")


def _batch(B, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(0, 256, (B, 1, 28, 28), dtype=torch.uint8, device="cuda", generator=g)
    y = torch.randint(0, 10, (B,), device="cuda", generator=g)
    return x.reshape(-1, 784), y


def _engine(seed=0, **kw):
    from p2pfl_amd.learning.fused_cnn import FusedCNNEngine

    ops.ext()
    return FusedCNNEngine(CNN(seed=seed).cuda(), device=torch.device("cuda"), **kw)


def _backward_ops(B, mrows, n_tiles, route_rm, gdump):
    """One forward + route on a fixed batch, then the conv2 backward and the merged Adam
    launch: the plain pair for ``n_tiles`` None, else the hosting pair split at ``n_tiles``.
    Returns every tensor the two launches write."""
    import p2pfl_amd.learning.fused_cnn as fc

    old, fc._ROUTE_RM = fc._ROUTE_RM, route_rm
    try:
        eng = _engine(seed=3, mrows=mrows)
    finally:
        fc._ROUTE_RM = old
    assert (eng.w1tbf is None) == route_rm
    if gdump:
        eng.gdump = torch.zeros_like(eng.params)
    x, y = _batch(B, seed=40 + B)
    C, M, a = eng.C, eng.mrows, eng._adam()
    stats = torch.zeros(4, device="cuda")
    eng.forward(x, y, None, B, stats, True)
    C.route_fc2(eng.dH, eng.w1_route, eng.am2, M, B, eng.dc2m, eng.gb, eng.dlogits, eng.H, eng.params, eng.m, eng.v,
                eng.gdump, eng.off, eng.adam_t, 1, *a, False, eng.route_rm, eng.route_ws, eng.route_ctr)
    if n_tiles is None:
        C.conv2_bwd(eng.dc2m, eng.p1s, eng.am1, eng.w2q, x, None, eng.wslab1, eng.wslab2, B)
        C.fc1_conv_adam(eng.dH, eng.a1, M, eng.wslab1, eng.wslab2, eng.gb, B, eng.params, eng.m, eng.v, eng.gdump,
                        eng.w1bf, eng.w1tbf, eng.w2r, eng.w2q, eng.off, eng.adam_t, 1, *a, eng.dlogits, eng.H, eng.w2bf)
    else:
        na = C.conv2_bwd_fc1(eng.dc2m, eng.p1s, eng.am1, eng.w2q, x, None, eng.wslab1, eng.wslab2, B, eng.dH, eng.a1, M,
                             eng.params, eng.m, eng.v, eng.gdump, eng.w1bf, eng.w1tbf, eng.off, eng.adam_t, 1, *a, n_tiles)
        assert na == n_tiles
        C.fc1_conv_adam(eng.dH, eng.a1, M, eng.wslab1, eng.wslab2, eng.gb, B, eng.params, eng.m, eng.v, eng.gdump,
                        eng.w1bf, eng.w1tbf, eng.w2r, eng.w2q, eng.off, eng.adam_t, 1, *a, eng.dlogits, eng.H, eng.w2bf,
                        first_tile=na)
    torch.cuda.synchronize()
    out = {n: getattr(eng, n).clone() for n in OP_TENSORS}
    if not route_rm:
        out["w1tbf"] = eng.w1tbf.clone()
    if gdump:
        out["gdump"] = eng.gdump.clone()
    return out


@functools.lru_cache(maxsize=None)
def _separate(B, mrows, route_rm, gdump):
    """The separate launches' result, computed once per configuration and only read."""
    return _backward_ops(B, mrows, None, route_rm, gdump)


def _check_ops(B, mrows, n_tiles, route_rm=True, gdump=False):
    ref = _separate(B, mrows, route_rm, gdump)
    got = _backward_ops(B, mrows, n_tiles, route_rm, gdump)
    assert set(got) == set(ref)
    for name in ref:
        assert torch.equal(got[name], ref[name]), f"{name} differs (B={B}, mrows={mrows}, n_tiles={n_tiles})"


@pytest.mark.parametrize("B", [32, 7])
@pytest.mark.parametrize("n_tiles", SLICES)
def test_hosted_tiles_are_bitwise_the_separate_launches(n_tiles, B):
    _check_ops(B, 32, n_tiles)


def test_hosted_tiles_write_the_same_gradient_dump():
    _check_ops(32, 32, 26, gdump=True)


@pytest.mark.parametrize("n_tiles", [26, 1600])
def test_hosted_tiles_write_the_same_transposed_shadow(n_tiles):
    """With the W1^T-shadow routing kernel the FC1 tiles also write ``w1tbf``."""
    _check_ops(32, 32, n_tiles, route_rm=False)


@pytest.mark.parametrize("B", [40, 7])
@pytest.mark.parametrize("n_tiles", [1, 26, 1600])
def test_hosted_tiles_with_64_row_launches(n_tiles, B):
    _check_ops(B, 64, n_tiles)


def test_separate_launches_moved_every_fc1_tile():
    """Guard for the comparisons above: one step changes the bf16 shadow inside every one
    of the 1600 tiles, so a tile that neither launch ran would show as a difference."""
    before = _engine(seed=3).w1bf.view(64, 32, 3136)
    after = _separate(32, 32, True, False)["w1bf"].view(64, 32, 3136)
    moved = torch.stack([(before != after)[:, :, k : k + 128].any(dim=2).any(dim=1) for k in range(0, 3136, 128)])
    assert moved.shape == (25, 64) and bool(moved.all())


PLANS = [[(0, 32), (32, 32), (64, 32), (96, 4)], [(0, 7), (7, 32)]]
STEP_TENSORS = ("params", "m", "v", "w1bf", "w2r", "w2q")


def _run_plan(eng, plan, x, y, perm):
    stats = torch.zeros((len(plan), 4), device="cuda")
    for j, (s, b) in enumerate(plan):
        eng.train_step_async(x, y, perm[s : s + b], b, stats[j], j + 1)
    return stats


@pytest.mark.parametrize("plan", PLANS)
def test_engine_with_a_slice_is_bitwise_equal(plan):
    """Whole training steps (ragged batches included) with a mid-row slice against slice 0."""
    n = plan[-1][0] + plan[-1][1]
    x, y = _batch(n, seed=21)
    perm = torch.randperm(n, device="cuda")
    out = []
    for sl in (0, 300):
        eng = _engine(seed=5, fc1_slice=sl)
        assert eng.fc1_slice == sl
        stats = _run_plan(eng, plan, x, y, perm)
        torch.cuda.synchronize()
        out.append([getattr(eng, n_).clone() for n_ in STEP_TENSORS] + [stats.clone()])
    for name, a, b in zip(STEP_TENSORS, out[0], out[1]):
        assert torch.equal(a, b), name
    # the loss / accuracy sums are float atomics of the head (order-dependent last bits)
    torch.testing.assert_close(out[0][-1], out[1][-1], rtol=1e-5, atol=1e-5)


def test_slice_defaults_from_the_environment(monkeypatch):
    monkeypatch.setenv("P2PFL_CNN_FC1_SLICE", "77")
    assert _engine(seed=5).fc1_slice == 77
    assert _engine(seed=5, fc1_slice=0).fc1_slice == 0
    with pytest.raises(ValueError):
        _engine(seed=5, fc1_slice=1601)


def test_captured_steps_with_a_slice_replay_bitwise():
    """Three steps with a slice captured in one graph and replayed twice against the
    same six steps launched eagerly."""
    plan = [(0, 32), (32, 32), (64, 12)]
    x, y = _batch(76, seed=22)
    perm = torch.randperm(76, device="cuda")
    eager = _engine(seed=6, fc1_slice=300)
    for _ in range(2):
        _run_plan(eager, plan, x, y, perm)
    torch.cuda.synchronize()
    eng = _engine(seed=6, fc1_slice=300)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="relaxed"):
        _run_plan(eng, plan, x, y, perm)
    torch.cuda.synchronize()
    assert torch.equal(eng.m, torch.zeros_like(eng.m)), "recording a capture must execute nothing"
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for name in STEP_TENSORS:
        assert torch.equal(getattr(eng, name), getattr(eager, name)), name


@pytest.mark.parametrize("bad", [-1, 1601])
def test_binding_rejects_a_tile_count_out_of_range(bad):
    eng = _engine(seed=3)
    x, _ = _batch(32, seed=1)
    a = eng._adam()
    before = eng.params.clone()
    with pytest.raises(RuntimeError, match="n_tiles"):
        eng.C.conv2_bwd_fc1(eng.dc2m, eng.p1s, eng.am1, eng.w2q, x, None, eng.wslab1, eng.wslab2, 32, eng.dH, eng.a1, 32,
                            eng.params, eng.m, eng.v, None, eng.w1bf, eng.w1tbf, eng.off, eng.adam_t, 1, *a, bad)
    with pytest.raises(RuntimeError, match="first_tile"):
        eng.C.fc1_conv_adam(eng.dH, eng.a1, 32, eng.wslab1, eng.wslab2, eng.gb, 32, eng.params, eng.m, eng.v, None,
                            eng.w1bf, eng.w1tbf, eng.w2r, eng.w2q, eng.off, eng.adam_t, 1, *a, eng.dlogits, eng.H,
                            eng.w2bf, first_tile=bad)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, before), "a rejected call must not launch"
