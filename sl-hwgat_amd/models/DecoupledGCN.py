"""MI355X (gfx950) backend of the DecoupledGCN baseline (SAM-SLR: decoupled graph convolution, attention gates, DropGraph).

Drop-in for the reference's `hwgat/models/DecoupledGCN.py`: class `Model` takes the same positional arguments
(in_channels, num_nodes, edges, groups, block_size, n_out_features, n_classes, dropout_ratio, batch_norm), as
`DecoupledGCNParams.get_model_params()` returns them, and its `state_dict()` has the reference's keys, order, shapes and
dtypes (`data_bn.*`, per unit `lN.A`, `lN.gcn1.{decoupled_A, linear_weight, linear_bias, eye_list, down.0, down.1, bn0,
bn}.*`, `lN.tcn1.{conv, bn}.*`, `lN.residual.{conv, bn}.*` where the reference has them, `lN.{conv_ta, conv_sa, fc1c,
fc2c}.*`, `head.classifier.*`); `lN.A` and `eye_list` are frozen parameters, as there.  Checkpoints and optimizer state
interchange.  Input (N, T, V, C), output (N, n_classes).  The forward runs on HIP kernels, fp32, channels-last:

    data_bn    stgcn_block.batch_norm_rows on the (N T, V C) view (channel index v C + c, as the reference's BatchNorm1d)
    l1 .. l10  dgcn_block.dgcn_unit: one autograd node per unit
    pool+drop  stgcn_block.mean_pool: mean over (T, V) with the head dropout fused (hash mask, device seed)
    classifier nn.Linear, as in the other models

`forward(x, keep_prob=0.9)`: units l1-l6 never drop, l7-l10 run DropGraph with `keep_prob` in train mode; eval mode and
keep_prob == 1 make it the identity.  The Bernoulli seeds of a draw come from the project's hash with the device-resident
seed (one site per draw, `_site_seeds(unit)`; the head dropout has site `_site_seeds(0)[0]`), so no torch RNG state is
consumed and a captured train step replays with fresh masks.

train() normalises with batch statistics and advances running_mean / running_var / num_batches_tracked on the device (no
host synchronisation in forward); eval() normalises with the running values.  No kernel uses an atomic: every run is
bit-reproducible.

`eye_list` stays in the state_dict for interchange only.  The reference multiplies the column normaliser into it
(`A diag(1 / (column sum + 0.001))`); the arithmetic here divides the columns directly, i.e. it ASSUMES eye_list is the
stack of identity matrices it is constructed as (it is frozen, so training never changes it).

Supported: in_channels 1..4, num_nodes <= 32, groups dividing 64, odd block_size, n_out_features a multiple of 64 up to
1024, any T >= 1.  `batch_norm=True` is refused (the reference's head crashes on it: no behaviour to match).

Test hooks, in the manner of STGCN.block_tap: `block_tap` (a list that receives every unit's output), `drop_tap` (a list
that receives, per draw, a dict with the unit, the site 0..3, the probabilities `p`, the `seeds`, the mask `scale` and
the scaled mask `factor`) and `drop_seeds` (a mapping (unit, site) -> seed tensor used in place of the hash draw).
"""
import math

import numpy as np
import torch
from torch import nn

from ..stgcn_block import RES_NONE, RES_IDENTITY, RES_CONV
from ..dgcn_block import dgcn_unit
from ._gcn import (GCNModel, Head, TEMPORAL_TAPS, HEAD_SITE, width_plan, stem_problem, width_problem,  # noqa: F401
                   edge_problem)

FIRST_DROP_UNIT = 7    # l1-l6 run at keep_prob 1; unit N (1..10) draws with _site_seeds(N), the head with HEAD_SITE


def shape_problem(in_channels, num_nodes, edges, groups, block_size, n_out_features, batch_norm):
    """None, or the message naming the rule a configuration breaks"""
    problem = stem_problem("DecoupledGCN", in_channels, num_nodes, batch_norm)
    if problem is not None:
        return problem
    if groups < 1 or 64 % groups:
        return f"groups {groups}: must divide 64, the narrowest unit's width"
    if block_size < 1 or block_size % 2 == 0:
        return (f"block_size {block_size}: must be odd (the reference's max-pool widening returns T + 1 frames for an even "
                f"block and fails)")
    problem = width_problem("DecoupledGCN", n_out_features)
    if problem is None and edges is None:
        problem = "edges None: an edge list is required for the decoupled GCN"
    return problem or edge_problem(num_nodes, edges)


def spatial_graph(num_nodes, edges):
    """The (3, V, V) float64 adjacency of the 'spatial' strategy with equal weights: [0] the self loops, [1] the inward
    links and [2] the outward (reversed) links, a link (i, j) being the entry [j, i], the two link matrices with every
    non-empty column divided by its sum."""
    V = num_nodes

    def links(pairs):
        m = np.zeros((V, V))
        for i, j in pairs:
            m[j, i] = 1
        return m

    def column_normalised(m):
        total = np.sum(m, 0)
        scale = np.zeros((V, V))
        for i in range(V):
            if total[i] > 0:
                scale[i, i] = total[i] ** (-1)
        return np.dot(m, scale)

    inward = [(e[0], e[1]) for e in edges]
    outward = [(j, i) for i, j in inward]
    return np.stack((links([(i, i) for i in range(V)]), column_normalised(links(inward)), column_normalised(links(outward))))


def find_drop_size(num_nodes, num_edges, K=1):
    """the expected number of joints a spatial DropGraph seed takes with it: the K-hop neighbourhood size of a graph with
    the average degree 2 E / V"""
    degree = 2 * num_edges / num_nodes
    return sum(degree * math.pow(degree - 1, i - 1) for i in range(1, K + 1))


def _conv_init(conv):
    nn.init.kaiming_normal_(conv.weight, mode="fan_out")
    nn.init.constant_(conv.bias, 0)


def _bn_init(bn, scale):
    nn.init.constant_(bn.weight, scale)
    nn.init.constant_(bn.bias, 0)


class Gcn(nn.Module):
    """parameter container of the reference's DecoupledGCNUnit"""

    def __init__(self, in_channels, out_channels, A, groups, num_points, num_subset=3):
        super().__init__()
        self.groups = groups
        self.decoupled_A = nn.Parameter(
            torch.tensor(np.reshape(A, [3, 1, num_points, num_points]), dtype=torch.float32).repeat(1, groups, 1, 1))
        if in_channels != out_channels:
            self.down = nn.Sequential(nn.Conv2d(in_channels, out_channels, 1), nn.BatchNorm2d(out_channels))
            _conv_init(self.down[0])
            _bn_init(self.down[1], 1)
        self.bn0 = nn.BatchNorm2d(out_channels * num_subset)
        self.bn = nn.BatchNorm2d(out_channels)
        _bn_init(self.bn0, 1)
        _bn_init(self.bn, 1e-6)
        self.linear_weight = nn.Parameter(torch.zeros(in_channels, out_channels * num_subset))
        self.linear_bias = nn.Parameter(torch.zeros(1, out_channels * num_subset, 1, 1))
        self.eye_list = nn.Parameter(torch.stack([torch.eye(num_points) for _ in range(out_channels)]), requires_grad=False)
        nn.init.normal_(self.linear_weight, 0, math.sqrt(0.5 / (out_channels * num_subset)))
        nn.init.constant_(self.linear_bias, 1e-6)


class Tcn(nn.Module):
    """parameter container of the reference's TCNUnit: `conv` (kernel_size x 1, temporal stride) and `bn`"""

    def __init__(self, in_channels, out_channels, kernel_size=TEMPORAL_TAPS, stride=1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, (kernel_size, 1), (stride, 1), ((kernel_size - 1) // 2, 0))
        self.bn = nn.BatchNorm2d(out_channels)
        _conv_init(self.conv)
        _bn_init(self.bn, 1)


class Unit(nn.Module):
    """parameter container of one reference DecoupledGCN_TCN_unit (same attribute names and order, the reference's
    initialisation); the arithmetic is dgcn_block.dgcn_unit"""

    def __init__(self, in_channels, out_channels, A, groups, num_points, stride=1, residual=True):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride
        self.gcn1 = Gcn(in_channels, out_channels, A, groups, num_points)
        self.tcn1 = Tcn(out_channels, out_channels, stride=stride)
        self.A = nn.Parameter(torch.tensor(np.sum(np.reshape(A.astype(np.float32), [3, num_points, num_points]), axis=0),
                                           dtype=torch.float32), requires_grad=False)
        if not residual:
            self.residual_kind = RES_NONE
        elif in_channels == out_channels and stride == 1:
            self.residual_kind = RES_IDENTITY
        else:
            self.residual_kind = RES_CONV
            self.residual = Tcn(in_channels, out_channels, kernel_size=1, stride=stride)
        self.conv_ta = nn.Conv1d(out_channels, 1, 9, padding=4)
        nn.init.constant_(self.conv_ta.weight, 0)
        nn.init.constant_(self.conv_ta.bias, 0)
        ker = num_points - 1 if not num_points % 2 else num_points
        self.conv_sa = nn.Conv1d(out_channels, 1, ker, padding=(ker - 1) // 2)
        nn.init.xavier_normal_(self.conv_sa.weight)
        nn.init.constant_(self.conv_sa.bias, 0)
        self.fc1c = nn.Linear(out_channels, out_channels // 2)
        self.fc2c = nn.Linear(out_channels // 2, out_channels)
        nn.init.kaiming_normal_(self.fc1c.weight)
        nn.init.constant_(self.fc1c.bias, 0)
        nn.init.constant_(self.fc2c.weight, 0)
        nn.init.constant_(self.fc2c.bias, 0)


class Model(GCNModel):
    _backend = "DecoupledGCN"
    _bf16_needs = "the BatchNorm statistics and the DropGraph statistics"

    def __init__(self, in_channels=2, num_nodes=29, edges=None, groups=8, block_size=41, n_out_features=256, n_classes=1000,
                 dropout_ratio=0.1, batch_norm=False):
        super().__init__(shape_problem(in_channels, num_nodes, edges, groups, block_size, n_out_features, batch_norm),
                         in_channels, num_nodes, n_out_features, dropout_ratio)
        self.groups, self.block_size = groups, block_size
        self.drop_size = find_drop_size(num_nodes, len(edges))
        A = spatial_graph(num_nodes, edges)
        self.data_bn = nn.BatchNorm1d(in_channels * num_nodes)
        for i, (ci, co, s) in enumerate(width_plan(in_channels, n_out_features)):
            setattr(self, f"l{i + 1}", Unit(ci, co, A, groups, num_nodes, stride=s, residual=i > 0))
        self.head = Head(n_out_features, n_classes, dropout_ratio)
        _bn_init(self.data_bn, 1)
        self.drop_tap = None               # a list: every DropGraph draw's record is appended to it
        self.drop_seeds = None             # {(unit, site): seed tensor} used in place of the hash draw
        self._finish()                     # (DropGraph's batch-wide normalisers couple the clips too)

    @property
    def units(self):
        return [getattr(self, f"l{i}") for i in range(1, 11)]

    def _blocks(self):
        return self.units

    def forward_features(self, x, keep_prob=0.9):
        self._check_input(x)
        if not 0.0 < float(keep_prob) <= 1.0:
            raise ValueError(f"keep_prob {keep_prob}: must be in (0, 1]")
        training = self.training
        seed_base = self._next_step_seed() if training else None
        h = self._stem(x)
        for i, unit in enumerate(self.units, start=1):
            drop = None
            if training and i >= FIRST_DROP_UNIT and float(keep_prob) != 1.0:
                drop = (float(keep_prob), self.drop_size, self.block_size, self._site_seeds(i), seed_base, self.drop_seeds,
                        self.drop_tap, i)
            h = dgcn_unit(h, unit, training, drop)
            self._tap(h)
        return self._pool(h, seed_base)
