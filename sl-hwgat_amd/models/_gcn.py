"""What the ST-GCN and DecoupledGCN baselines share: the head, the ten-row width plan, the refusals both state and one
base class on `DeviceSeeds, nn.Module`.

A model of the pair is  data_bn -> ten blocks (one autograd node each) -> mean pool with the head dropout -> classifier.
The base owns the input check with the `data_bn` stem, the pool tail, `frames_out`, `set_activation_dtype` and `forward`;
a subclass constructs its modules in its own order (registration order is the `state_dict` key order of the reference
class), builds its adjacency, runs its block loop, and takes `_next_step_seed()` at its own moment: the seed advance is a
launch, so where it sits is part of the model's launch sequence.
"""
import math

import torch
from torch import nn

from .. import functional as HF
from ..seeding import DeviceSeeds
from ..stgcn_block import batch_norm_rows, mean_pool

TEMPORAL_TAPS = 9
HEAD_SITE = 0          # the head dropout's site: _site_seeds(0)[0]


def width_plan(in_channels, n_out_features):
    """(C_in, C_out, temporal stride) of the ten blocks"""
    return [(in_channels, 64, 1), (64, 64, 1), (64, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 128, 1),
            (128, 256, 2), (256, 256, 1), (256, n_out_features, 1)]


# The clauses of a model's `shape_problem` that both state, in the order each model asks them.  `backend`: "ST-GCN" or
# "DecoupledGCN", as the messages name it.
def stem_problem(backend, in_channels, num_nodes, batch_norm):
    if batch_norm:
        return ("batch_norm=True: the reference's head fails on it (FC reads self.n_features before it exists), so there "
                f"is no behaviour to reproduce; the {backend} backend takes batch_norm=False only")
    if not 1 <= in_channels <= 4:
        return f"in_channels {in_channels}: the {backend} backend takes 1 to 4 coordinates per joint"
    if not 1 <= num_nodes <= HF.STGCN_MAX_NODES:
        return f"num_nodes {num_nodes}: the graph aggregation kernels take at most {HF.STGCN_MAX_NODES} joints"
    return None


def width_problem(backend, n_out_features):
    if n_out_features <= 0 or n_out_features % 64 or n_out_features > 1024:
        return f"n_out_features {n_out_features}: the {backend} backend takes multiples of 64 up to 1024"
    return None


def edge_problem(num_nodes, edges):
    for e in edges or ():
        if len(e) != 2 or not (0 <= e[0] < num_nodes and 0 <= e[1] < num_nodes):
            return f"edge {list(e)}: not a pair of joints of a {num_nodes}-joint graph"
    return None


class Head(nn.Module):
    """the reference's FC head: dropout (fused into the pool kernel here) and `classifier`"""

    def __init__(self, n_features, num_class, dropout_ratio):
        super().__init__()
        self.dropout_ratio = float(dropout_ratio)
        self.classifier = nn.Linear(n_features, num_class)
        nn.init.normal_(self.classifier.weight, 0, math.sqrt(2.0 / num_class))


class GCNModel(DeviceSeeds, nn.Module):
    _backend = None             # "ST-GCN" / "DecoupledGCN"
    _bf16_needs = None          # what a bf16 form of the subclass would have to bring, for set_activation_dtype's refusal

    def __init__(self, problem, in_channels, num_nodes, n_out_features, dropout_ratio):
        """`problem`: the subclass's shape_problem of its arguments.  The subclass goes on to register its modules and
        ends with _finish."""
        super().__init__()
        if problem is not None:
            raise NotImplementedError(problem)
        if not 0.0 <= float(dropout_ratio) < 1.0:
            raise ValueError(f"dropout_ratio {dropout_ratio}: must be in [0, 1)")
        self.in_channels, self.num_nodes, self.n_out_features = in_channels, num_nodes, n_out_features

    def _finish(self):
        self.activation_dtype = torch.float32
        self.block_tap = None              # a list: every block's output (N, T, V, C) is appended to it (tests, debugging)
        self._init_device_seeds(clips_independent_in_train=False)      # BatchNorm's batch statistics couple the clips

    def _blocks(self):
        """the ten containers, in order"""
        raise NotImplementedError

    def set_activation_dtype(self, dtype):
        if dtype != torch.float32:
            raise NotImplementedError(
                f"activation dtype {dtype}: the {self._backend} backend runs in fp32 only (bf16 needs its own parity "
                f"contract for {self._bf16_needs})")
        return self

    def frames_out(self, T):
        for blk in self._blocks():
            T = (T - 1) // blk.stride + 1
        return T

    def _check_input(self, x):
        if x.dim() != 4 or x.shape[2] != self.num_nodes or x.shape[3] != self.in_channels:
            raise ValueError(f"expected (N, T, {self.num_nodes}, {self.in_channels}), got {tuple(x.shape)}")

    def _stem(self, x):
        """data_bn on the (N T, V C) view of a checked input"""
        N, T, V, C = x.shape
        if T < 1:
            raise ValueError("at least one frame")
        x = self._input_view(x.contiguous().float())
        return batch_norm_rows(x.view(N * T, V * C), self.data_bn, self.training).view(N, T, V, C)

    def _tap(self, h):
        if self.block_tap is not None:
            self.block_tap.append(h.detach())

    def _pool(self, h, seed_base):
        """mean over (T, V) with the head dropout of the train mode"""
        p = self.head.dropout_ratio if self.training else 0.0
        return mean_pool(h.view(h.shape[0], -1, h.shape[-1]), p, self._site_seeds(HEAD_SITE)[0], seed_base)

    def forward(self, x, *args, **kwargs):
        return self._classify(self.head.classifier, self.forward_features(x, *args, **kwargs))
