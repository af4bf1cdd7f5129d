"""Aggregation strategies."""

from p2pfl_amd.learning.aggregators.aggregator import Aggregator, NoModelsToAggregateError
from p2pfl_amd.learning.aggregators.fedavg import FedAvg
from p2pfl_amd.learning.aggregators.robust import FedMedian, Krum, TrimmedMean

__all__ = ["Aggregator", "NoModelsToAggregateError", "FedAvg", "FedMedian", "TrimmedMean", "Krum"]
