"""MI355X (gfx950) backend of the ST-GCN baseline.

Drop-in for the reference's `hwgat/models/STGCN.py`: class `Model` takes the same positional arguments (in_channels,
num_nodes, center, inward_edges, edge_importance_weighting, n_out_features, n_classes, dropout_ratio, batch_norm), as
`STGCNParams.get_model_params()` returns them, and its `state_dict()` has the reference's keys, order, shapes and dtypes
(`A`, `data_bn.*`, `st_gcn_networks.i.{gcn.conv, tcn.0, tcn.2, tcn.3, residual.0, residual.1}.*`, `edge_importance.i`,
`head.classifier.*`, every running statistic and `num_batches_tracked`), so checkpoints and optimizer state interchange.
Input (N, T, V, C), output (N, n_classes).  The forward runs on HIP kernels only, fp32, channels-last:

    data_bn    stgcn_block.batch_norm_rows on the (N T, V C) view (channel index v C + c, as the reference's BatchNorm1d)
    blocks     stgcn_block.st_gcn_block: one autograd node per block
    pool+drop  stgcn_block.mean_pool: mean over (T, V) with the head dropout fused (hash mask, device seed)
    classifier nn.Linear, as in the other models

train() normalises with batch statistics and advances running_mean / running_var / num_batches_tracked on the device (no
host synchronisation in forward); eval() normalises with the running values.  No kernel uses an atomic, so
`deterministic_train` / `deterministic_eval` are honoured by construction: every run is bit-reproducible.

Supported: in_channels 1..4, num_nodes <= 32, n_out_features a multiple of 64 up to 1024, edge_importance_weighting True
or False, any T >= 1.  `batch_norm=True` is refused (the reference's head crashes on it: no behaviour to match).
"""
import math

import numpy as np
import torch
from torch import nn

from .. import functional as HF
from ..seeding import DeviceSeeds
from ..stgcn_block import st_gcn_block, batch_norm_rows, mean_pool, RES_NONE, RES_IDENTITY, RES_CONV

TEMPORAL_TAPS = 9
HEAD_SITE = 0          # the head dropout's site: _site_seeds(0)[0]


def shape_problem(in_channels, num_nodes, n_out_features, batch_norm, center=0, inward_edges=()):
    """None, or the message naming the rule a configuration breaks"""
    if batch_norm:
        return ("batch_norm=True: the reference's head fails on it (FC reads self.n_features before it exists), so there "
                "is no behaviour to reproduce; the ST-GCN backend takes batch_norm=False only")
    if not 1 <= in_channels <= 4:
        return f"in_channels {in_channels}: the ST-GCN backend takes 1 to 4 coordinates per joint"
    if not 1 <= num_nodes <= HF.STGCN_MAX_NODES:
        return f"num_nodes {num_nodes}: the graph aggregation kernels take at most {HF.STGCN_MAX_NODES} joints"
    if n_out_features <= 0 or n_out_features % 64 or n_out_features > 1024:
        return f"n_out_features {n_out_features}: the ST-GCN backend takes multiples of 64 up to 1024"
    if not 0 <= center < num_nodes:
        return f"center {center}: not a joint of a {num_nodes}-joint graph"
    for e in inward_edges or ():
        if len(e) != 2 or not (0 <= e[0] < num_nodes and 0 <= e[1] < num_nodes):
            return f"edge {list(e)}: not a pair of joints of a {num_nodes}-joint graph"
    return None


def spatial_adjacency(num_nodes, center, inward_edges):
    """The (3, V, V) float64 adjacency of the 'spatial configuration' partition with neighbours at most one hop away
    (ST-GCN, arXiv 1801.07455, section 3.4): the column-normalised one-hop adjacency D^-1-scaled per column, split by how
    far the two joints of an entry are from `center` -- [0] self loops, [1] same distance or the row joint farther from
    the centre, [2] the row joint nearer.  "Distance to the centre" only tells 0 hops, 1 hop and unreachable-in-one-hop
    (infinity) apart, as the reference does."""
    V = num_nodes
    link = np.eye(V)
    for i, j in inward_edges:
        link[i, j] = 1
        link[j, i] = 1
    hop = np.full((V, V), np.inf)
    hop[link > 0] = 1
    hop[np.eye(V) > 0] = 0
    near = np.zeros((V, V))
    near[hop <= 1] = 1
    deg = near.sum(0)
    scale = np.zeros((V, V))
    for i in range(V):
        if deg[i] > 0:
            scale[i, i] = deg[i] ** (-1)
    norm = np.dot(near, scale)
    same = hop[:, center][:, None] == hop[:, center][None, :]          # [j, i]: d(j) == d(i)
    farther = hop[:, center][:, None] > hop[:, center][None, :]        # [j, i]: d(j) > d(i)
    self_part = np.where(hop == 0, norm, 0.0)
    one = hop == 1
    root = np.where(one & same, norm, 0.0)
    close = np.where(one & farther, norm, 0.0)
    further = np.where(one & ~same & ~farther, norm, 0.0)
    return np.stack([self_part, root + close, further])


class GraphConv(nn.Module):
    """parameter container of the reference's ConvTemporalGraphical: `conv`, C_in -> 3 C_out, 1x1, with bias"""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        self.kernel_size = kernel_size
        self.conv = nn.Conv2d(in_channels, out_channels * kernel_size, kernel_size=(1, 1))


class Block(nn.Module):
    """parameter container of one reference STGCN_BLOCK (same attribute names and order, torch's own initialisation);
    the arithmetic is stgcn_block.st_gcn_block.  The torch modules only hold parameters and running statistics."""

    def __init__(self, in_channels, out_channels, stride=1, residual=True):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride
        self.gcn = GraphConv(in_channels, out_channels, 3)
        self.tcn = nn.Sequential(
            nn.BatchNorm2d(out_channels),
            nn.ReLU(inplace=True),
            nn.Conv2d(out_channels, out_channels, (TEMPORAL_TAPS, 1), (stride, 1), ((TEMPORAL_TAPS - 1) // 2, 0)),
            nn.BatchNorm2d(out_channels),
            nn.Dropout(0, inplace=True),
        )
        if not residual:
            self.residual_kind = RES_NONE
        elif in_channels == out_channels and stride == 1:
            self.residual_kind = RES_IDENTITY
        else:
            self.residual_kind = RES_CONV
            self.residual = nn.Sequential(
                nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=(stride, 1)),
                nn.BatchNorm2d(out_channels),
            )


class Head(nn.Module):
    """the reference's FC head: dropout (fused into the pool kernel here) and `classifier`"""

    def __init__(self, n_features, num_class, dropout_ratio):
        super().__init__()
        self.dropout_ratio = float(dropout_ratio)
        self.classifier = nn.Linear(n_features, num_class)
        nn.init.normal_(self.classifier.weight, 0, math.sqrt(2.0 / num_class))


class Model(DeviceSeeds, nn.Module):
    def __init__(self, in_channels=2, num_nodes=29, center=0, inward_edges=None, edge_importance_weighting=True,
                 n_out_features=256, n_classes=1000, dropout_ratio=0.05, batch_norm=False):
        super().__init__()
        problem = shape_problem(in_channels, num_nodes, n_out_features, batch_norm, center, inward_edges)
        if problem is not None:
            raise NotImplementedError(problem)
        if not 0.0 <= float(dropout_ratio) < 1.0:
            raise ValueError(f"dropout_ratio {dropout_ratio}: must be in [0, 1)")
        self.in_channels, self.num_nodes, self.n_out_features = in_channels, num_nodes, n_out_features
        A = torch.tensor(spatial_adjacency(num_nodes, center, inward_edges or []), dtype=torch.float32, requires_grad=False)
        self.register_buffer("A", A)
        self.data_bn = nn.BatchNorm1d(in_channels * num_nodes)
        widths = [(in_channels, 64, 1), (64, 64, 1), (64, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 128, 1),
                  (128, 256, 2), (256, 256, 1), (256, n_out_features, 1)]
        self.st_gcn_networks = nn.ModuleList([Block(ci, co, s, residual=i > 0) for i, (ci, co, s) in enumerate(widths)])
        if edge_importance_weighting:
            self.edge_importance = nn.ParameterList([nn.Parameter(torch.ones(self.A.size())) for _ in self.st_gcn_networks])
        else:
            self.edge_importance = [None] * len(self.st_gcn_networks)
        self.head = Head(n_out_features, n_classes, dropout_ratio)
        self.activation_dtype = torch.float32
        self.block_tap = None              # a list: every block's output (N, T, V, C) is appended to it (tests, debugging)
        self._init_device_seeds(clips_independent_in_train=False)      # BatchNorm's batch statistics

    def set_activation_dtype(self, dtype):
        if dtype != torch.float32:
            raise NotImplementedError(
                f"activation dtype {dtype}: the ST-GCN backend runs in fp32 only (bf16 needs its own parity contract for "
                f"the BatchNorm statistics and bf16 MFMA temporal-convolution kernels)")
        return self

    def frames_out(self, T):
        for blk in self.st_gcn_networks:
            T = (T - 1) // blk.stride + 1
        return T

    def forward_features(self, x):
        if x.dim() != 4 or x.shape[2] != self.num_nodes or x.shape[3] != self.in_channels:
            raise ValueError(f"expected (N, T, {self.num_nodes}, {self.in_channels}), got {tuple(x.shape)}")
        N, T, V, C = x.shape
        if T < 1:
            raise ValueError("at least one frame")
        training = self.training
        h = batch_norm_rows(x.contiguous().float().view(N * T, V * C), self.data_bn, training).view(N, T, V, C)
        for blk, importance in zip(self.st_gcn_networks, self.edge_importance):
            h = st_gcn_block(h, blk, self.A, importance, training)
            if self.block_tap is not None:
                self.block_tap.append(h.detach())
        p = self.head.dropout_ratio if training else 0.0
        seed_base = self._next_step_seed() if training else None
        return mean_pool(h.view(N, -1, h.shape[-1]), p, self._site_seeds(HEAD_SITE)[0], seed_base)

    def forward(self, x):
        return self._classify(self.head.classifier, self.forward_features(x))
