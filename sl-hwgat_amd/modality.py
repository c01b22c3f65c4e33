"""Input modalities: the four views of a keypoint clip that multi-stream skeleton recognisers train on.

The 2s-AGCN / CTR-GCN line and the SL-GCN sign-language entries train one network per view -- joints, bones (a joint minus
the joint it hangs on), joint motion (the next frame minus this one) and bone motion -- and add the four models' scores
(ensemble.Ensemble).  A `Modality` is the view as an object: one launch of csrc/modality.hip (formulas:
include/hwgat_hip.h, "input modalities") in front of a model's first kernel.

    modality = importlib.import_module("sl-hwgat_amd.modality")
    parents = modality.parents_from_edges(hw.STGCNParams(ds, 2).edges_, 29)
    model.set_input_modality(modality.Modality("bone_motion", parents))
    logits = model(x)                      # x: the raw joints, left alone; the model reads their bone motion

The input tensor is never written: train.GraphedTrainStep's static `x`, which the mixer and the device loader fill in
place, holds the joints after the forward as before it.  The modality is part of the model's forward and so a node of
whatever graph captures that forward.
"""
from collections import deque

import torch

from . import functional as HF

KINDS = HF.MOD_KINDS
BONE_KINDS = ("bone", "bone_motion")


def parents_from_edges(edges, num_joints, roots=(0,)):
    """a parent per joint from an undirected edge list: breadth-first from each root in turn, neighbours in ascending
    index, so a graph with cycles (the graphs of models/model_params.py have them) gives its spanning tree of shortest
    paths.  A joint no root reaches becomes the root of its own component, lowest index first.  parent[j] == j marks a
    root.  Returns a list of `num_joints` ints"""
    J = int(num_joints)
    if J < 1:
        raise ValueError(f"num_joints must be positive, got {num_joints}")
    near = [set() for _ in range(J)]
    for e in edges:
        if len(e) != 2:
            raise ValueError(f"edge {list(e)}: not a pair of joints")
        a, b = int(e[0]), int(e[1])
        if not (0 <= a < J and 0 <= b < J):
            raise ValueError(f"edge {[a, b]}: not a pair of joints of a {J}-joint graph")
        if a != b:
            near[a].add(b)
            near[b].add(a)
    starts = [int(r) for r in roots]
    for r in starts:
        if not 0 <= r < J:
            raise ValueError(f"root {r}: not a joint of a {J}-joint graph")
    parent = [-1] * J
    for r in starts + list(range(J)):
        if parent[r] != -1:
            continue
        parent[r] = r
        queue = deque([r])
        while queue:
            a = queue.popleft()
            for b in sorted(near[a]):
                if parent[b] == -1:
                    parent[b] = a
                    queue.append(b)
    return parent


class Modality:
    """`kind` of KINDS; `parents` (a sequence of J joint indices, parents[j] == j a root) is needed by the two bone kinds;
    `pad_value` marks padded frames by their first word (None: no frame is padding).  A padded frame passes through
    unchanged and the motion kinds give 0 in front of one.  Everything is checked on the host; the table is kept as an
    int32 tensor that `to(device)` moves"""

    def __init__(self, kind, parents=None, pad_value=None):
        if kind not in KINDS:
            raise ValueError(f"Modality: kind must be one of {KINDS}, got {kind!r}")
        if parents is not None:
            parents = [int(p) for p in (parents.tolist() if isinstance(parents, torch.Tensor) else parents)]
            bad = [p for p in parents if not 0 <= p < len(parents)]
            if not parents or bad:
                raise ValueError(f"Modality: every parent must be a joint index in [0, {len(parents)}), got {bad or parents}")
        elif kind in BONE_KINDS:
            raise ValueError(f"Modality: kind {kind!r} needs the parent table (modality.parents_from_edges)")
        if pad_value is not None:
            pad_value = float(pad_value)
            if pad_value != pad_value:
                raise ValueError("Modality: pad_value must be a number that compares equal to itself, got NaN")
        self.kind, self.parents, self.pad_value = kind, parents, pad_value
        self.table = None if parents is None else torch.tensor(parents, dtype=torch.int32)

    def to(self, device):
        if self.table is not None:
            self.table = self.table.to(device)
        return self

    def apply(self, x, table=None, pad_value=None):
        """the view of x (B, T, J, C) fp32 on the device.  `table`: a copy of the parent table that lives elsewhere (a
        model's buffer); `pad_value`: the caller's padding marker when this object has none"""
        table = self.table if table is None else table
        if self.parents is not None and x.dim() == 4 and x.shape[2] != len(self.parents):
            raise ValueError(f"Modality: the parent table is for {len(self.parents)} joints, the input has {x.shape[2]}")
        if table is not None and table.device != x.device:
            table = self.table = self.table.to(x.device)
        return HF.modality(x, table, self.kind, self.pad_value if self.pad_value is not None else pad_value)

    __call__ = apply

    def state(self):
        return {"kind": self.kind, "parents": None if self.parents is None else list(self.parents),
                "pad_value": self.pad_value}

    @classmethod
    def from_state(cls, d):
        return cls(d["kind"], d.get("parents"), d.get("pad_value"))

    def __eq__(self, other):
        return isinstance(other, Modality) and self.state() == other.state()

    def __hash__(self):
        return hash((self.kind, None if self.parents is None else tuple(self.parents), self.pad_value))

    def __repr__(self):
        return f"Modality({self.kind!r}, parents={self.parents}, pad_value={self.pad_value})"
