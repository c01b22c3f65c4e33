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
import numpy as np
import torch
from torch import nn

from ..stgcn_block import st_gcn_block, RES_NONE, RES_IDENTITY, RES_CONV
from ._gcn import (GCNModel, Head, TEMPORAL_TAPS, HEAD_SITE, width_plan, stem_problem, width_problem,  # noqa: F401
                   edge_problem)


def shape_problem(in_channels, num_nodes, n_out_features, batch_norm, center=0, inward_edges=()):
    """None, or the message naming the rule a configuration breaks"""
    problem = stem_problem("ST-GCN", in_channels, num_nodes, batch_norm) or width_problem("ST-GCN", n_out_features)
    if problem is None and not 0 <= center < num_nodes:
        problem = f"center {center}: not a joint of a {num_nodes}-joint graph"
    return problem or edge_problem(num_nodes, inward_edges)


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


class Model(GCNModel):
    _backend = "ST-GCN"
    _bf16_needs = "the BatchNorm statistics and bf16 MFMA temporal-convolution kernels"

    def __init__(self, in_channels=2, num_nodes=29, center=0, inward_edges=None, edge_importance_weighting=True,
                 n_out_features=256, n_classes=1000, dropout_ratio=0.05, batch_norm=False):
        super().__init__(shape_problem(in_channels, num_nodes, n_out_features, batch_norm, center, inward_edges),
                         in_channels, num_nodes, n_out_features, dropout_ratio)
        A = torch.tensor(spatial_adjacency(num_nodes, center, inward_edges or []), dtype=torch.float32, requires_grad=False)
        self.register_buffer("A", A)
        self.data_bn = nn.BatchNorm1d(in_channels * num_nodes)
        self.st_gcn_networks = nn.ModuleList([Block(ci, co, s, residual=i > 0)
                                              for i, (ci, co, s) in enumerate(width_plan(in_channels, n_out_features))])
        if edge_importance_weighting:
            self.edge_importance = nn.ParameterList([nn.Parameter(torch.ones(self.A.size())) for _ in self.st_gcn_networks])
        else:
            self.edge_importance = [None] * len(self.st_gcn_networks)
        self.head = Head(n_out_features, n_classes, dropout_ratio)
        self._finish()

    def _blocks(self):
        return self.st_gcn_networks

    def forward_features(self, x):
        self._check_input(x)
        h = self._stem(x)
        for blk, importance in zip(self.st_gcn_networks, self.edge_importance):
            h = st_gcn_block(h, blk, self.A, importance, self.training)
            self._tap(h)
        return self._pool(h, self._next_step_seed() if self.training else None)
