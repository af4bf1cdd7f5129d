"""The differential-privacy HIP kernels (csrc/dp_update.hip) against fp64 and
bitwise references, and a GaussianMechanism round end to end on one MI355X."""

from __future__ import annotations

import functools
import math

import pytest
import torch

from dp_cases import synthetic_layout
from p2pfl_amd import ops
from p2pfl_amd.learning import arena
from p2pfl_amd.learning.privacy import GaussianMechanism, gaussian_epsilon

pytestmark = pytest.mark.gpu

CNN_ARENA = 6_497_216  # more than one grid-stride trip at 2048 blocks of 256 lanes x 4 elements
SHAPES = ["synthetic", 64, 1_048_640, CNN_ARENA]
SEED, ROUND = 1234, 7


@pytest.fixture(autouse=True)
def _require_ext():
    ops.ext()  # fail loudly if the native extension is missing on a GPU box


@functools.lru_cache(maxsize=None)
def _table(shape) -> torch.Tensor:
    if shape == "synthetic":
        return arena.dp_block_table(synthetic_layout(), arena.DP_EXEMPT, "cuda")
    nb = shape // 64
    t = torch.full((nb,), 64, dtype=torch.uint8)
    if nb > 1:  # exempt blocks and tail blocks of every length, spread over the arena
        i = torch.arange(nb)
        t[i % 97 == 5] = 0
        tails = i % 101 == 7
        t[tails] = (i[tails] // 101 % 63 + 1).to(torch.uint8)
        t[-1] = 37
    return t.cuda()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(w, w0, table, covered mask, fp64 squared norm of the covered update): made once, never written."""
    table = _table(shape)
    n = table.numel() * 64
    g = torch.Generator(device="cuda").manual_seed(n % 1013)
    w0 = torch.randn(n, device="cuda", generator=g)
    w = w0 + 0.01 * torch.randn(n, device="cuda", generator=g)
    cov = (torch.arange(64, device="cuda")[None, :] < table.long()[:, None]).reshape(-1)
    ss64 = float(((w.double() - w0.double()) ** 2)[cov].sum())
    return w, w0, table, cov, ss64


@functools.lru_cache(maxsize=None)
def _noise(shape):
    """(kernel draws g = dp_apply(0, 0, C = 1, z = 1), table) at (SEED, ROUND)."""
    table = _table(shape)
    zero = torch.zeros(table.numel() * 64, device="cuda")
    ss = ops.dp_delta_sqnorm(zero, zero.clone(), table)
    assert float(ss) == 0.0
    return ops.dp_apply(zero, torch.zeros_like(zero), table, ss, 1.0, 1.0, SEED, ROUND), table


def _on_side_stream(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = fn()
    torch.cuda.current_stream().wait_stream(s)
    return out


# ---------------------------------------------------------------------------
# norm pass
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_sqnorm_vs_fp64_and_deterministic(shape):
    w, w0, table, _, ss64 = _case(shape)
    ss = ops.dp_delta_sqnorm(w, w0, table)
    assert ss.shape == (1,) and ss.dtype == torch.float32 and ss.is_cuda
    print(f"dp_delta_sqnorm {shape}: kernel {float(ss):.9g} fp64 {ss64:.9g} rel {abs(float(ss) - ss64) / ss64:.2e}")
    assert abs(float(ss) - ss64) <= 1e-5 * ss64
    assert torch.equal(ops.dp_delta_sqnorm(w, w0, table), ss)  # fixed-order reductions, no atomics
    assert torch.equal(_on_side_stream(lambda: ops.dp_delta_sqnorm(w, w0, table)), ss)


def test_sqnorm_skips_what_the_table_skips():
    """NaN in padding and in exempt blocks never reaches the sum; integers are summed exactly."""
    w, w0, table, cov, _ = _case("synthetic")
    g = torch.Generator(device="cuda").manual_seed(1)
    wi = torch.randint(-2, 3, (w.numel(),), device="cuda", generator=g).float()
    w0i = torch.randint(-2, 3, (w.numel(),), device="cuda", generator=g).float()
    want = float(((wi - w0i) ** 2)[cov].double().sum())  # an integer < 2^24: exact in any order
    wi[~cov] = float("nan")
    assert float(ops.dp_delta_sqnorm(wi, w0i, table)) == want


# ---------------------------------------------------------------------------
# apply pass without noise: bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("clipped", [False, True], ids=["identity", "clipped"])
@pytest.mark.parametrize("shape", SHAPES)
def test_apply_without_noise_is_bitwise_the_reference(shape, clipped):
    w, w0, table, cov, ss64 = _case(shape)
    ss = ops.dp_delta_sqnorm(w, w0, table)
    clip = math.sqrt(ss64) * (0.37 if clipped else 1.5)
    out = ops.dp_apply(w, w0, table, ss, clip, 0.0, SEED, ROUND)
    assert out.data_ptr() != w.data_ptr() and out.dtype == torch.float32 and out.shape == w.shape
    ref = ops.dp_apply_reference(w.cpu(), w0.cpu(), table.cpu(), ss.cpu(), clip, 0.0, SEED, ROUND)
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(out[~cov], w[~cov])  # padding and exempt blocks
    if clipped:
        norm = math.sqrt(float(((out.double() - w0.double()) ** 2)[cov].sum()))
        # each output is rounded at its own magnitude (|w0| < 8): 2^-24 * 8 * sqrt(n) at the most
        assert norm <= clip * (1 + 1e-6) + 2.0**-24 * 8 * math.sqrt(w.numel())
        assert bool((out != w)[cov].any())
    else:
        assert torch.equal(out, w)
    given = torch.empty_like(w)
    assert ops.dp_apply(w, w0, table, ss, clip, 0.0, SEED, ROUND, out=given) is given and torch.equal(given, out)


def test_apply_error_paths():
    w, w0, table, _, _ = _case("synthetic")
    ss = ops.dp_delta_sqnorm(w, w0, table)
    with pytest.raises((ValueError, RuntimeError), match="overlap"):
        ops.dp_apply(w, w0, table, ss, 1.0, 0.0, 1, 0, out=w)
    with pytest.raises((ValueError, RuntimeError), match="overlap"):
        ops.dp_apply(w, w0, table, ss, 1.0, 0.0, 1, 0, out=w0)
    with pytest.raises(ValueError):
        ops.dp_apply(w, w0, table[:-1], ss, 1.0, 0.0, 1, 0)
    with pytest.raises(ValueError):
        ops.dp_delta_sqnorm(w[:96], w0[:96], table[:1])
    with pytest.raises(ValueError):
        ops.dp_apply(w, w0, table.cpu(), ss, 1.0, 0.0, 1, 0)
    with pytest.raises(ValueError):
        ops.dp_apply(w, w0, table, ss, 1.0, 1.0, 1 << 64, 0)


# ---------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_noise_vs_fp64_reference(shape):
    """w = w0 = 0, C = 1, z = 1: out is g itself.  Against fp64 Box-Muller from the same bits:
    16 ulp at the largest radius 5.77 (3 / 3 / 4 ulp for log, sqrt, sincospi) = 1.2e-5."""
    g, table = _noise(shape)
    n = g.numel()
    cov = (torch.arange(64, device="cuda")[None, :] < table.long()[:, None]).reshape(-1)
    assert not g[~cov].any()  # not covered: out = w = 0
    # the reference of a large arena costs seconds: 32 spans of 16 384 elements spread evenly over it,
    # the first at element 0 and the last ending at n, so that every grid-stride trip is sampled
    m = 1 << 14
    spans = [(0, n)] if n <= 1 << 21 else [((n - m) * i // 31 // 64 * 64, m) for i in range(32)]
    worst = 0.0
    for first, m in spans:
        ref = torch.from_numpy(ops.dp_noise_reference(m, SEED, ROUND, first=first)).cuda()
        err = (g[first : first + m].double() - ref)[cov[first : first + m]].abs()
        worst = max(worst, float(err.max())) if err.numel() else worst
    print(f"dp noise {shape}: max |g_kernel - g_fp64| = {worst:.3e} over {sum(m for _, m in spans)} elements")
    assert worst <= 1.2e-5
    assert float(g.abs().max()) <= ops.DP_NOISE_MAX * (1 + 1e-6)


def test_noise_distribution():
    g, table = _noise(1_048_640)
    n = 1 << 20
    # every element, covered by the shared case's table or not: a table of full blocks
    zero = torch.zeros(n, device="cuda")
    all64 = torch.full((n // 64,), 64, dtype=torch.uint8, device="cuda")
    x = ops.dp_apply(zero, torch.zeros_like(zero), all64, torch.zeros(1, device="cuda"), 1.0, 1.0, SEED, ROUND).double()
    cov = (torch.arange(64, device="cuda")[None, :] < table.long()[:, None]).reshape(-1)[:n]
    assert torch.equal(x.float()[cov], g[:n][cov])  # the draws do not depend on the table
    mean, var = float(x.mean()), float(x.var(unbiased=False))
    s = x.sort().values
    cdf = 0.5 * (1.0 + torch.erf(s / math.sqrt(2.0)))
    i = torch.arange(n, device="cuda", dtype=torch.float64)
    ks = float(torch.maximum(((i + 1) / n - cdf).max(), (cdf - i / n).max()))
    print(f"dp noise n=2^20 seed={SEED} round={ROUND}: mean {mean:.5f} var {var:.5f} KS {ks:.5f}")
    assert abs(mean) <= 4 / math.sqrt(n)
    assert abs(var - 1) <= 4 * math.sqrt(2 / n)
    assert ks <= 1.95 / math.sqrt(n)


@pytest.mark.parametrize("shape", SHAPES)
def test_noised_apply_is_reproducible(shape):
    w, w0, table, cov, ss64 = _case(shape)
    ss = ops.dp_delta_sqnorm(w, w0, table)
    clip = math.sqrt(ss64) * 0.5
    run = lambda rnd=ROUND, seed=SEED: ops.dp_apply(w, w0, table, ss, clip, 0.8, seed, rnd)  # noqa: E731
    a = run()
    assert a.data_ptr() != w.data_ptr()
    assert torch.equal(run(), a)
    assert torch.equal(_on_side_stream(run), a)
    assert torch.equal(a[~cov], w[~cov])
    for other in (run(rnd=ROUND + 1), run(seed=SEED + 1), run(seed=SEED + (1 << 32))):
        assert float((other != a)[cov].float().mean()) > 0.99
    # base + sigma * g, singly rounded: the noise-free kernel output plus the kernel's own draws
    base = ops.dp_apply(w, w0, table, ss, clip, 0.0, SEED, ROUND)
    g, _ = _noise(shape)
    sigma = torch.tensor(0.8 * clip, dtype=torch.float32, device="cuda")
    assert torch.equal(a[cov], (base + sigma * g)[cov])


# ---------------------------------------------------------------------------
# mechanism and nodes
# ---------------------------------------------------------------------------
def test_mechanism_on_cuda_arenas():
    from p2pfl_amd.learning.arena import FlatParams

    layout = synthetic_layout()
    w, w0, table, cov, ss64 = _case("synthetic")
    live, start = FlatParams.from_flat(w, layout), FlatParams.from_flat(w0, layout)
    m = GaussianMechanism(0.5 * math.sqrt(ss64), 0.0, seed=3)
    out = m.privatize(live, start, 4)
    assert isinstance(out, FlatParams) and out.flat.is_cuda and out.flat.data_ptr() != w.data_ptr()
    ss = ops.dp_delta_sqnorm(w, w0, table)
    assert torch.equal(out.flat, ops.dp_apply(w, w0, table, ss, m.clip_norm, 0.0, 3, 4))
    assert math.isclose(m.last_update_norm(), math.sqrt(ss64), rel_tol=1e-5) and m.releases == 1


def test_two_nodes_one_private_round():
    from p2pfl_amd.communication.memory import InMemoryCommunicationProtocol
    from p2pfl_amd.data import MnistFederatedDM
    from p2pfl_amd.learning.torch_learner import TorchLearner
    from p2pfl_amd.models import MLP
    from p2pfl_amd.node import Node
    from p2pfl_amd.utils import check_equal_models, wait_4_results, wait_convergence

    nodes = []
    try:
        for i in range(2):
            nd = Node(MLP(seed=i), MnistFederatedDM(sub_id=i, number_sub=30), protocol=InMemoryCommunicationProtocol,
                      learner=TorchLearner, privacy=GaussianMechanism(1.0, 0.1, seed=i))
            nd.start()
            nodes.append(nd)
        nodes[1].connect(nodes[0].addr)
        wait_convergence(nodes, 1, only_direct=True)
        nodes[0].set_start_learning(rounds=1, epochs=1)
        wait_4_results(nodes, timeout=300)
        check_equal_models(nodes, atol=1e-6)
        for nd in nodes:
            params = nd.state.learner.get_parameters()
            assert params.flat.is_cuda and bool(torch.isfinite(params.flat).all())
            m = nd.state.privacy
            norm = m.last_update_norm()
            assert norm is not None and math.isfinite(norm) and norm > 0
            assert m.releases == 1 and m.epsilon() == gaussian_epsilon(1, 0.1, 1e-5)
            a = 2.0 / 0.1**2
            assert math.isclose(m.epsilon(), a + 2 * math.sqrt(a * math.log(1e5)), rel_tol=1e-12)
    finally:
        for nd in nodes:
            nd.stop()
