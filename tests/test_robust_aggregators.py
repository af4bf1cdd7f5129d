"""Byzantine-robust aggregators on the torch path: reference math, the
one-by-one protocol rule of non-decomposable aggregators, a CPU federation."""

from __future__ import annotations

import os
import subprocess
import sys
from collections import OrderedDict

import pytest
import torch

from p2pfl_amd import ops
from p2pfl_amd.communication.memory import InMemoryCommunicationProtocol
from p2pfl_amd.data import MnistFederatedDM
from p2pfl_amd.learning.aggregators import Aggregator, FedAvg, FedMedian, Krum, TrimmedMean
from p2pfl_amd.learning.aggregators.robust import krum_select
from p2pfl_amd.models import MLP
from p2pfl_amd.node import Node
from p2pfl_amd.utils import check_equal_models, wait_4_results, wait_convergence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _m(*vals: float) -> OrderedDict:
    return OrderedDict(w=torch.tensor(vals, dtype=torch.float32))


# ---------------------------------------------------------------------------
# reference functions, hand-computed
# ---------------------------------------------------------------------------
def test_trimmed_mean_reference_small_cases():
    # columns: (1, 5, 3 | 9), (-2, 0, 7 | 1), (4, 4, 4 | 4)
    a, b, c, d = (torch.tensor(v) for v in ([1.0, -2.0, 4.0], [5.0, 0.0, 4.0], [3.0, 7.0, 4.0], [9.0, 1.0, 4.0]))
    # odd k: median is the middle value, trim 0 the mean
    assert ops.trimmed_mean_reference([a, b, c], 1).tolist() == [3.0, 0.0, 4.0]
    assert ops.coordinate_median([a, b, c]).tolist() == [3.0, 0.0, 4.0]
    assert ops.trimmed_mean([a, b, c], 0).tolist() == [3.0, pytest.approx(5.0 / 3.0), 4.0]
    # even k: mean of the two middle values (numpy's median, not torch.median's lower one)
    assert ops.coordinate_median([a, b, c, d]).tolist() == [4.0, 0.5, 4.0]
    assert ops.trimmed_mean([a, b, c, d], 1).tolist() == [4.0, 0.5, 4.0]
    assert ops.trimmed_mean([a, b, c, d], 0).tolist() == [4.5, 1.5, 4.0]
    assert ops.coordinate_median([a, d]).tolist() == [5.0, -0.5, 4.0]
    assert ops.coordinate_median([b]).tolist() == [5.0, 0.0, 4.0]
    # k = 5, trim = 1: the three middle values
    e = torch.tensor([-100.0, 100.0, 4.0])
    assert ops.trimmed_mean([a, b, c, d, e], 1).tolist() == [3.0, pytest.approx(8.0 / 3.0), 4.0]
    # order of the inputs is irrelevant, bf16 inputs and output are accepted
    assert torch.equal(ops.trimmed_mean([d, b, e, a, c], 1), ops.trimmed_mean([a, b, c, d, e], 1))
    out = ops.coordinate_median([a.to(torch.bfloat16), b, c], out_dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.tolist() == [3.0, 0.0, 4.0]
    buf = torch.empty(3)
    assert ops.trimmed_mean([a, b, c], 1, out=buf) is buf and buf.tolist() == [3.0, 0.0, 4.0]


def test_ops_error_paths_cpu():
    x = [torch.zeros(8) for _ in range(17)]
    with pytest.raises(ValueError, match="16"):
        ops.trimmed_mean(x, 0)
    with pytest.raises(ValueError, match="16"):
        ops.coordinate_median(x)
    with pytest.raises(ValueError, match="16"):
        ops.pairwise_sqdist(x)
    with pytest.raises(ValueError):
        ops.trimmed_mean([torch.zeros(8), torch.zeros(9)], 0)
    with pytest.raises(ValueError):
        ops.pairwise_sqdist([torch.zeros(8), torch.zeros(9)])
    with pytest.raises(ValueError):
        ops.trimmed_mean(x[:4], 2)  # (4 - 1) // 2 = 1
    with pytest.raises(ValueError):
        ops.trimmed_mean(x[:4], -1)
    with pytest.raises(ValueError):
        ops.trimmed_mean([], 0)


def test_pairwise_sqdist_reference_small_case():
    a, b, c = torch.tensor([0.0, 0.0]), torch.tensor([3.0, 4.0]), torch.tensor([1.0, 0.0]).to(torch.bfloat16)
    d = ops.pairwise_sqdist([a, b, c])
    assert d.dtype == torch.float32
    assert d.tolist() == [[0.0, 25.0, 1.0], [25.0, 0.0, 20.0], [1.0, 20.0, 0.0]]
    assert ops.pairwise_sqdist([a]).tolist() == [[0.0]]


def test_krum_scores_and_tie_break():
    # points on a line: 0, 1, 2, 10, 11  (k = 5, f = 1: 2 nearest neighbours each)
    pts = [0.0, 1.0, 2.0, 10.0, 11.0]
    dist = [[(p - q) ** 2 for q in pts] for p in pts]
    # scores: 0 -> 1 + 4, 1 -> 1 + 1, 2 -> 1 + 4, 10 -> 1 + 64, 11 -> 1 + 81
    assert krum_select(dist, f=1, m=1) == [1]
    # tie between index 0 and 2 (score 5 each) goes to the lower index
    assert krum_select(dist, f=1, m=2) == [0, 1]
    assert krum_select(dist, f=1, m=3) == [0, 1, 2]
    assert krum_select(dist, f=1, m=9) == [0, 1, 2, 3]  # at most k - f
    # f is clamped to (k - 3) // 2: k = 3 scores by the single nearest neighbour
    d3 = [[0.0, 1.0, 9.0], [1.0, 0.0, 4.0], [9.0, 4.0, 0.0]]
    assert krum_select(d3, f=5, m=1) == [0]  # scores 1, 1, 4: tie -> index 0
    # k = 4, f = 1 -> f_eff = 0: the two nearest
    pts4 = [0.0, 1.0, 3.0, 100.0]
    d4 = [[(p - q) ** 2 for q in pts4] for p in pts4]
    assert krum_select(d4, f=1, m=1) == [1]  # scores 1+9, 1+4, 4+9, ...


def test_aggregators_on_cpu_models():
    honest = {f"n{i}": (_m(float(i), 1.0, -float(i)), 10 * (i + 1)) for i in range(4)}
    models = dict(honest, n9=(_m(100.0, 100.0, 100.0), 1000))
    assert FedMedian().aggregate(models)["w"].tolist() == [2.0, 1.0, -1.0]
    assert TrimmedMean(trim=1).aggregate(models)["w"].tolist() == [2.0, 1.0, pytest.approx(-1.0)]
    assert TrimmedMean("me").trim == 1
    # Krum picks one honest model, bitwise; Multi-Krum a sample-weighted mean of honest ones
    res = Krum(f=1).aggregate(models)
    assert any(torch.equal(res["w"], m["w"]) for m, _ in honest.values())
    multi = Krum(f=1, m=2).aggregate(models)["w"]
    assert float(multi.abs().max()) < 10
    assert float(FedAvg().aggregate(models)["w"].abs().max()) > 10  # the control: FedAvg is poisoned
    # the caller's key names survive, the result is a flat arena
    assert list(res.keys()) == ["w"] and res.flat.numel() >= 3
    # arrival order does not matter
    rev = OrderedDict(reversed(list(models.items())))
    for cls in (FedMedian, TrimmedMean, Krum):
        assert torch.equal(cls().aggregate(models)["w"], cls().aggregate(rev)["w"])
    with pytest.raises(Exception):
        FedMedian().aggregate({})


# ---------------------------------------------------------------------------
# protocol rule: models of a non-decomposable aggregator travel one by one
# ---------------------------------------------------------------------------
def test_partial_aggregation_flag():
    assert Aggregator.partial_aggregation is True and FedAvg.partial_aggregation is True
    assert not FedMedian.partial_aggregation and not TrimmedMean.partial_aggregation and not Krum.partial_aggregation


@pytest.mark.parametrize("cls", [FedMedian, TrimmedMean, Krum])
def test_single_entries_never_combined(cls):
    agg = cls("me")
    agg.set_nodes_to_aggregate(["a", "b", "c", "d"])
    mb, ma = _m(3.0, 3.0), _m(1.0, 1.0)
    assert agg.add_model(mb, ["b"], 3) == ["b"]
    assert agg.add_model(ma, ["a"], 1) == ["b", "a"]
    calls = []
    agg.aggregate = lambda models: calls.append(models)  # must never run for gossip
    m, contrib, w = agg.get_partial_aggregation([])
    assert m is ma and contrib == ["a"] and w == 1  # the smallest key, as stored
    m, contrib, w = agg.get_partial_aggregation(["a"])
    assert m is mb and contrib == ["b"] and w == 3  # honours except_nodes
    assert agg.get_partial_aggregation(["c", "a"])[0] is mb
    assert agg.get_partial_aggregation(["a", "b"]) == (None, None, None)
    assert not calls and not agg._partial_cache
    # a pre-averaged partial (a misconfigured FedAvg peer) is rejected ...
    assert not agg.would_accept(["c", "d"])
    assert agg.add_model(_m(9.0, 9.0), ["c", "d"], 2) == []
    assert agg.would_accept(["c"])
    # ... a full aggregate is still accepted and supersedes the single models
    assert agg.would_accept(["a", "b", "c", "d"])
    full = _m(7.0, 7.0)
    assert sorted(agg.add_model(full, ["d", "c", "b", "a"], 4)) == ["a", "b", "c", "d"]
    del agg.aggregate
    assert agg.wait_and_get_aggregation(timeout=1) is full
    agg.clear()


def test_full_aggregate_of_live_members_accepted():
    agg = FedMedian("me")
    agg.set_nodes_to_aggregate(["a", "b", "c"])
    agg.mark_lost(["c"])
    assert agg.would_accept(["a", "b"])  # covers every live member: a full aggregate
    assert agg.add_model(_m(1.0), ["a", "b"], 2) == ["a", "b"]
    agg.clear()
    # waiting for the diffused aggregate (a non-member): unchanged
    agg.set_waiting_aggregated_model(["a", "b"])
    assert not agg.would_accept(["a"]) and agg.would_accept(["a", "b"])
    assert agg.add_model(_m(2.0), ["a", "b"], 1) == ["a", "b"]
    assert agg.wait_and_get_aggregation(timeout=1)["w"].tolist() == [2.0]
    agg.clear()


def test_fedavg_still_combines_and_caches():
    agg = FedAvg("me")
    agg.set_nodes_to_aggregate(["a", "b", "c", "d"])
    agg.add_model(_m(1.0), ["a"], 1)
    agg.add_model(_m(3.0), ["b"], 3)
    m, contrib, w = agg.get_partial_aggregation(["c"])
    assert sorted(contrib) == ["a", "b"] and w == 4 and m["w"].tolist() == [2.5]
    assert agg.get_partial_aggregation(["c"])[0] is m
    assert agg.would_accept(["c", "d"])
    assert sorted(agg.add_model(_m(5.0), ["c", "d"], 2)) == ["a", "b", "c", "d"]
    agg.clear()


@pytest.mark.parametrize("make", [lambda: Krum("me", f=1), lambda: TrimmedMean("me", trim=1), lambda: FedMedian("me")])
def test_fewer_models_than_expected(make):
    """A member's model never arrives: the timeout aggregates the k = 2 on hand."""
    agg = make()
    agg.set_nodes_to_aggregate(["a", "b", "c", "d"])
    agg.add_model(_m(1.0, -4.0), ["b"], 5)
    agg.add_model(_m(3.0, 0.0), ["a"], 1)
    res = agg.wait_and_get_aggregation(timeout=0.05)
    assert res["w"].tolist() == [2.0, -2.0]  # unweighted mean of the two
    agg.clear()
    agg.set_nodes_to_aggregate(["a", "b", "c"])
    agg.add_model(_m(1.0, -4.0), ["b"], 5)
    assert agg.wait_and_get_aggregation(timeout=0.05)["w"].tolist() == [1.0, -4.0]
    agg.clear()


# ---------------------------------------------------------------------------
# end to end on the CPU
# ---------------------------------------------------------------------------
def test_three_cpu_nodes_fedmedian():
    nodes = []
    for i in range(3):
        nd = Node(MLP(seed=i), MnistFederatedDM(sub_id=i, number_sub=30), protocol=InMemoryCommunicationProtocol,
                  aggregator=FedMedian, device="cpu")
        nd.start()
        nodes.append(nd)
    try:
        for i in range(2):
            nodes[i + 1].connect(nodes[i].addr)
        wait_convergence(nodes, 2, only_direct=False)
        nodes[0].set_start_learning(rounds=2, epochs=1)
        wait_4_results(nodes, timeout=240)
        check_equal_models(nodes, atol=1e-6)
        assert all(isinstance(nd.aggregator, FedMedian) for nd in nodes)
    finally:
        for nd in nodes:
            nd.stop()


def test_mnist_example_aggregator_flag():
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-m", "p2pfl_amd.examples.mnist", "--aggregator", "fedmedian", "--nodes", "2",
                          "--rounds", "1", "--fast", "--device", "cpu"], env=env, capture_output=True, text=True,
                         timeout=200)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
