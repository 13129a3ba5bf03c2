"""Aggregators: FedAvg, FedMedian, SCAFFOLD, FedProx, robust (Krum, trimmed mean, geometric median, Bulyan, DnC), decentralised NeighborAvg and its robust form ClippedGossip."""

from myfyp_amd.learning.aggregators.aggregator import Aggregator, NoModelsToAggregateError
from myfyp_amd.learning.aggregators.bulyan import Bulyan
from myfyp_amd.learning.aggregators.clipped_gossip import ClippedGossip
from myfyp_amd.learning.aggregators.dnc import DnC
from myfyp_amd.learning.aggregators.fedavg import FedAvg
from myfyp_amd.learning.aggregators.fedmedian import FedMedian
from myfyp_amd.learning.aggregators.fedprox import FedProx
from myfyp_amd.learning.aggregators.geometric_median import GeometricMedian
from myfyp_amd.learning.aggregators.krum import Krum
from myfyp_amd.learning.aggregators.neighbor_avg import NeighborAvg
from myfyp_amd.learning.aggregators.scaffold import Scaffold
from myfyp_amd.learning.aggregators.trimmed_mean import TrimmedMean

__all__ = ["Aggregator", "NoModelsToAggregateError", "Bulyan", "ClippedGossip", "DnC", "FedAvg", "FedMedian", "FedProx", "GeometricMedian", "Krum", "NeighborAvg", "Scaffold", "TrimmedMean"]
