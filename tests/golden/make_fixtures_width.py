#!/usr/bin/env python3
"""Golden vectors for HWGATE models whose stage widths are odd multiples of 64, from the REFERENCE (development
container only).

Run:  python tests/golden/make_fixtures_width.py [name ...]       (needs /root/reference)

Built like make_fixtures_window.py (the same `import_reference`, `oracle.hwgat_oracle.synth_params` parameters and
`record` fields), with embed_dim 64, 192, 320 or 960:

  width_d64.npz      T = 16, K = 64,  C = 2, W = 16, heads (2, 4, 8),  d0 = 64   -> widths 64 / 128 / 256, head_dim 32
  width_d64_w8.npz   the same with W = 8 ("pwin" attention), head_dim 32
  width_d192.npz     T = 16, K = 112, C = 3, W = 16, heads (3, 6, 12), d0 = 192  -> widths 192 / 384 / 768, head_dim 64
  width_d320.npz     T = 16, K = 64,  C = 2, W = 16, heads (5, 10),    d0 = 320  -> widths 320 / 640, head_dim 64,
                     two stages of two blocks each
  width_d960.npz     T = 16, K = 64,  C = 3, W = 16, heads (15,),      d0 = 960  -> one stage of two blocks, head_dim 64

each with inputs, eval logits, the loss and gradient digests of one eval-mode backward, the same under train mode with
forced thresholds (HWGATE.py:94-100), the `attn_mask` buffers and the state_dict structure (keys and shapes); the last
two also carry `depths` (the first three keep the reference's default (2, 2, 4); two blocks per stage, so that every
stage has a shifted block and its `attn_mask`), and their forced thresholds (`train.thr`) are moved from the nominal
values to the nearest gap of the fp64 oracle's probabilities, so that fp32 rounding cannot flip the selector.  With
names given only those files are written; the inputs of every case are still drawn, in order, so a file does not depend
on which others are written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

from make_fixtures import import_reference  # noqa: E402
from make_fixtures_window import THRESHOLDS, build, record  # noqa: E402
from helpers import oracle_tie_free_thresholds  # noqa: E402

# (name, T, K, W, C, heads, d0, classes, batch, parameter seed, depths)
CASES = (("width_d64", 16, 64, 16, 2, (2, 4, 8), 64, 7, 2, 41, None),
         ("width_d64_w8", 16, 64, 8, 2, (2, 4, 8), 64, 7, 2, 42, None),
         ("width_d192", 16, 112, 16, 3, (3, 6, 12), 192, 5, 2, 43, None),
         ("width_d320", 16, 64, 16, 2, (5, 10), 320, 7, 2, 44, (2, 2)),
         ("width_d960", 16, 64, 16, 3, (15,), 960, 5, 2, 45, (2,)))


def main(only=()):
    Model, HWGATEParams, Loss = import_reference()
    torch.manual_seed(1004)
    crit = Loss()
    g = torch.Generator().manual_seed(37)
    for name, T, K, W, C, heads, d0, nc, B, seed, depths in CASES:
        x = torch.rand(B, T, K, C, generator=g)
        y = torch.randint(0, nc, (B,), generator=g)
        if only and name not in only:
            continue
        model, hp = build(Model, HWGATEParams, T=T, K=K, W=W, C=C, d0=d0, nc=nc, heads=heads, seed=seed, depths=depths)
        thr = THRESHOLDS
        if depths is not None:
            # thresholds no probability of the fp64 oracle comes close to (helpers.oracle_tie_free_thresholds): at the
            # nominal values a probability of width_d960's first block sits 8e-6 (relative) from 0.3, inside fp32 rounding
            params = {k: v for k, v in model.state_dict().items() if not k.endswith("attn_mask")}
            thr, margin = oracle_tie_free_thresholds(params, x, THRESHOLDS[:sum(depths)], num_kps=K, temporal_dim=T,
                                                     depths=depths, num_heads=heads, adj=hp.adj_mat)
            print(name, "thresholds", thr, "margin", margin)
            assert margin > 5e-5
        fx = record(model, hp, x, y, crit, [T, K, C, d0, nc, B, seed, W], thr)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **fx)
        print(name, os.path.getsize(os.path.join(HERE, name + ".npz")) // 1024, "KiB")


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
