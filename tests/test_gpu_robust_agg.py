"""Robust-aggregation HIP kernels (order statistics, pairwise distances) vs
fp64 references, and FedMedian / TrimmedMean / Krum end to end on one MI355X."""

from __future__ import annotations

import functools

import pytest
import torch

from p2pfl_amd import ops
from p2pfl_amd.communication.memory import InMemoryCommunicationProtocol
from p2pfl_amd.data import MnistFederatedDM
from p2pfl_amd.learning.aggregators import FedAvg, FedMedian, Krum, TrimmedMean
from p2pfl_amd.learning.aggregators.robust import krum_select
from p2pfl_amd.learning.arena import FlatParams, flatten
from p2pfl_amd.learning.torch_learner import TorchLearner
from p2pfl_amd.models import MLP
from p2pfl_amd.node import Node
from p2pfl_amd.settings import Settings
from p2pfl_amd.utils import check_equal_models, wait_4_results, wait_convergence

pytestmark = pytest.mark.gpu

CNN_ARENA = 6_497_216  # the grid-stride loop runs more than one trip at 2048 blocks
GRID = [(k, n) for k in (1, 2, 3, 4, 5, 8, 15, 16) for n in (64, 4099, 1_048_580)] + [(3, CNN_ARENA), (16, CNN_ARENA)]


@pytest.fixture(autouse=True)
def _require_ext():
    ops.ext()  # fail loudly if the native extension is missing on a GPU box


@functools.lru_cache(maxsize=None)
def _case(k: int, n: int):
    """(fp32 inputs, their fp64 coordinate-wise sort), computed once per shape and never written."""
    g = torch.Generator(device="cuda").manual_seed(k * 1009 + n % 1013)
    flats = tuple(torch.randn(n, device="cuda", generator=g) for _ in range(k))
    return flats, torch.stack(flats).double().sort(0).values


def _trims(k: int):
    return sorted({0, min(1, (k - 1) // 2), (k - 1) // 2})


@pytest.mark.parametrize("k,n", [(k, n) for k, n in GRID if k % 2])
def test_median_of_odd_k_is_a_selected_input(k, n):
    flats, _ = _case(k, n)
    out = ops.trimmed_mean(list(flats), (k - 1) // 2)
    assert torch.equal(out, torch.stack(flats).sort(0).values[k // 2])  # no arithmetic: no rounding
    assert torch.equal(ops.coordinate_median(list(flats)), out)


@pytest.mark.parametrize("k,n", GRID)
def test_trimmed_mean_vs_fp64(k, n):
    flats, srt = _case(k, n)
    for b in _trims(k):
        ref = srt[b : k - b].mean(0)
        out = ops.trimmed_mean(list(flats), b)
        assert out.dtype == torch.float32
        torch.testing.assert_close(out, ref.float(), atol=1e-5, rtol=1e-5)
        out16 = ops.trimmed_mean(list(flats), b, out_dtype=torch.bfloat16)
        assert out16.dtype == torch.bfloat16
        torch.testing.assert_close(out16, ref.to(torch.bfloat16), atol=1e-2, rtol=8e-3)


@pytest.mark.parametrize("in_dtypes", ["f32", "bf16", "mixed"])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("k,n", [(3, 4099), (8, 1 << 20)])
def test_trimmed_mean_dtypes(in_dtypes, out_dtype, k, n):
    """bf16 arenas are widened in registers: fp64 reference of the same (bf16-valued) inputs."""
    flats = []
    for i, f in enumerate(_case(k, n)[0]):
        flats.append(f.to(torch.bfloat16) if in_dtypes == "bf16" or (in_dtypes == "mixed" and i % 2) else f)
    srt = torch.stack([f.double() for f in flats]).sort(0).values
    for b in _trims(k):
        ref = srt[b : k - b].mean(0)
        out = ops.trimmed_mean(flats, b, out_dtype=out_dtype)
        assert out.dtype == out_dtype
        if out_dtype == torch.bfloat16:
            torch.testing.assert_close(out, ref.to(torch.bfloat16), atol=1e-2, rtol=8e-3)
        else:
            torch.testing.assert_close(out, ref.float(), atol=1e-5, rtol=1e-5)
        given = torch.empty(n, dtype=out_dtype, device="cuda")
        assert ops.trimmed_mean(flats, b, out=given) is given and torch.equal(given, out)


@pytest.mark.parametrize("k", [7, 8])
def test_trimmed_mean_permutation_invariant(k):
    """Kept values are added in sorted order: the arena order cannot matter, ties included."""
    n = 4099
    g = torch.Generator(device="cuda").manual_seed(k)
    values = torch.tensor([-1.5, 0.1, 0.3, 0.7, 2.9], device="cuda")
    flats = [values[torch.randint(0, 5, (n,), device="cuda", generator=g)] for _ in range(k)]
    pg = torch.Generator().manual_seed(100 + k)
    for b in _trims(k):
        base = ops.trimmed_mean(flats, b)
        for _ in range(3):
            perm = torch.randperm(k, generator=pg).tolist()
            assert torch.equal(ops.trimmed_mean([flats[i] for i in perm], b), base)


def _sqdist_fp64(flats):
    k = len(flats)
    x = [f.double() for f in flats]
    d = torch.zeros(k, k, dtype=torch.float64, device=flats[0].device)
    for i in range(k):
        for j in range(i + 1, k):
            d[i, j] = d[j, i] = (x[i] - x[j]).square().sum()
    return d


@pytest.mark.parametrize("k,n,dtype", [(k, n, torch.float32) for k in (2, 3, 8, 16) for n in (64, 4099, 1_048_580)]
                         + [(8, 4099, torch.bfloat16)])
def test_pairwise_sqdist_exact_on_integers(k, n, dtype):
    """Integers in [-2, 2]: every distance is an integer <= 16 n < 2^24, exact in fp32 in any order."""
    g = torch.Generator(device="cuda").manual_seed(k * 31 + n % 17)
    flats = [torch.randint(-2, 3, (n,), device="cuda", generator=g).to(dtype) for _ in range(k)]
    d = ops.pairwise_sqdist(flats)
    assert d.shape == (k, k) and d.dtype == torch.float32 and d.is_cuda
    assert torch.equal(d.double(), _sqdist_fp64(flats))
    assert torch.equal(d, d.t()) and torch.equal(d.diagonal(), torch.zeros(k, device="cuda"))


@pytest.mark.parametrize("k,n", [(5, CNN_ARENA), (16, 1_048_580)])
def test_pairwise_sqdist_randn(k, n):
    flats = list(_case(k, n)[0])
    d = ops.pairwise_sqdist(flats)
    torch.testing.assert_close(d.double(), _sqdist_fp64(flats), rtol=1e-5, atol=0)
    assert torch.equal(d, d.t()) and torch.equal(d.diagonal(), torch.zeros(k, device="cuda"))
    assert torch.equal(ops.pairwise_sqdist(flats), d)  # fixed-order reductions, no atomics


def test_error_paths():
    x = [torch.zeros(64, device="cuda") for _ in range(17)]
    with pytest.raises(ValueError, match="16"):
        ops.trimmed_mean(x, 0)
    with pytest.raises(ValueError, match="16"):
        ops.pairwise_sqdist(x)
    with pytest.raises(ValueError):
        ops.trimmed_mean([x[0], torch.zeros(68, device="cuda")], 0)
    with pytest.raises(ValueError):
        ops.pairwise_sqdist([x[0], torch.zeros(68, device="cuda")])
    with pytest.raises(ValueError):
        ops.trimmed_mean([x[0], torch.zeros(64)], 0)  # device mismatch
    with pytest.raises(ValueError):
        ops.trimmed_mean(x[:5], 3)
    with pytest.raises(ValueError):
        ops.trimmed_mean(x[:5], -1)


# ---------------------------------------------------------------------------
# aggregators on CUDA arenas
# ---------------------------------------------------------------------------
def _poisoned_set():
    base = flatten(MLP(seed=0).to("cuda").state_dict(), device=torch.device("cuda"))
    g = torch.Generator(device="cuda").manual_seed(5)
    models = {}
    for i in range(4):
        flat = base.flat + 0.01 * torch.randn(base.flat.numel(), device="cuda", generator=g)
        models[f"node-{i}"] = (FlatParams.from_flat(flat, base.layout), 100 + i)
    models["node-2b"] = (FlatParams.from_flat(torch.full_like(base.flat, 100.0), base.layout), 5000)
    return models


def test_aggregators_resist_a_poisoned_model():
    models = _poisoned_set()
    keys = sorted(models)
    flats = [models[k][0].flat for k in keys]
    honest = [models[k][0].flat for k in keys if k != "node-2b"]
    reversed_arrival = dict(reversed(list(models.items())))

    sel = krum_select(ops.pairwise_sqdist_reference(flats).tolist(), 1, 1)
    refs = {
        FedMedian: ops.trimmed_mean_reference(flats, 2),
        TrimmedMean: ops.trimmed_mean_reference(flats, 1),
        Krum: flats[sel[0]],
    }
    for cls, ref in refs.items():
        res = cls("me").aggregate(models)
        assert isinstance(res, FlatParams) and res.flat.is_cuda and list(res.keys()) == list(models[keys[0]][0].keys())
        assert float(res.flat.abs().max()) < 10
        torch.testing.assert_close(res.flat, ref, atol=1e-5, rtol=1e-5)
        assert torch.equal(cls("me").aggregate(reversed_arrival).flat, res.flat)
    # the control: the sample-weighted mean is dragged away
    assert float(FedAvg("me").aggregate(models).flat.abs().max()) > 10
    # Krum hands back one honest model, bitwise
    res = Krum("me", f=1, m=1).aggregate(models)
    assert any(torch.equal(res.flat, h) for h in honest)
    # Multi-Krum: the sample-weighted mean of honest models only
    multi = Krum("me", f=1, m=3).aggregate(models)
    assert float(multi.flat.abs().max()) < 10


# ---------------------------------------------------------------------------
# virtual peers, one of them poisoned
# ---------------------------------------------------------------------------
class PoisonedLearner(TorchLearner):
    """Trains normally, then replaces its weights by the constant 100."""

    def fit(self) -> None:
        super().fit()
        own = self.get_parameters()
        self.set_parameters(FlatParams.from_flat(torch.full_like(own.flat, 100.0), own.layout))


def _federation(n, aggregator, poisoned=(), chain=False, train_set_size=None):
    old = Settings.TRAIN_SET_SIZE
    if train_set_size is not None:
        Settings.TRAIN_SET_SIZE = train_set_size
    nodes = []
    try:
        for i in range(n):
            nd = Node(MLP(seed=i), MnistFederatedDM(sub_id=i, number_sub=30), protocol=InMemoryCommunicationProtocol,
                      aggregator=aggregator, learner=PoisonedLearner if i in poisoned else TorchLearner)
            nd.start()
            nodes.append(nd)
        for j in range(1, n):
            for i in ([j - 1] if chain else range(j)):
                nodes[j].connect(nodes[i].addr)
        wait_convergence(nodes, n - 1, only_direct=not chain)
        nodes[0].set_start_learning(rounds=2, epochs=1)
        wait_4_results(nodes, timeout=300)
        check_equal_models(nodes, atol=1e-6)
        for nd in nodes:
            assert isinstance(nd.aggregator, aggregator.func if isinstance(aggregator, functools.partial) else aggregator)
            params = nd.state.learner.get_parameters()
            assert params.flat.is_cuda
            assert float(params.flat.abs().max()) < 10
    finally:
        Settings.TRAIN_SET_SIZE = old
        for nd in nodes:
            nd.stop()


def test_fedmedian_peers_with_one_poisoned():
    _federation(4, FedMedian, poisoned={1})


def test_krum_peers_with_one_poisoned():
    _federation(5, functools.partial(Krum, f=1), poisoned={3}, train_set_size=5)


def test_trimmed_mean_peers_on_a_chain():
    """Honest peers on a line: single models are relayed over a non-full mesh."""
    _federation(3, TrimmedMean, chain=True)
