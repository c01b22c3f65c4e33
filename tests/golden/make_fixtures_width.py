#!/usr/bin/env python3
"""Golden vectors for HWGATE models whose stage widths are odd multiples of 64, from the REFERENCE (development
container only).

Run:  python tests/golden/make_fixtures_width.py        (needs /root/reference)

Built like make_fixtures_window.py (the same `import_reference`, `oracle.hwgat_oracle.synth_params` parameters and
`record` fields), with embed_dim 64 or 192:

  width_d64.npz      T = 16, K = 64,  C = 2, W = 16, heads (2, 4, 8),  d0 = 64   -> widths 64 / 128 / 256, head_dim 32
  width_d64_w8.npz   the same with W = 8 ("pwin" attention), head_dim 32
  width_d192.npz     T = 16, K = 112, C = 3, W = 16, heads (3, 6, 12), d0 = 192  -> widths 192 / 384 / 768, head_dim 64

each with inputs, eval logits, the loss and gradient digests of one eval-mode backward, the same under train mode with
forced thresholds (HWGATE.py:94-100), the `attn_mask` buffers and the state_dict structure (keys and shapes).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_fixtures import import_reference  # noqa: E402
from make_fixtures_window import build, record  # noqa: E402

# (name, T, K, W, C, heads, d0, classes, batch, parameter seed)
CASES = (("width_d64", 16, 64, 16, 2, (2, 4, 8), 64, 7, 2, 41),
         ("width_d64_w8", 16, 64, 8, 2, (2, 4, 8), 64, 7, 2, 42),
         ("width_d192", 16, 112, 16, 3, (3, 6, 12), 192, 5, 2, 43))


def main():
    Model, HWGATEParams, Loss = import_reference()
    torch.manual_seed(1004)
    crit = Loss()
    g = torch.Generator().manual_seed(37)
    for name, T, K, W, C, heads, d0, nc, B, seed in CASES:
        model, hp = build(Model, HWGATEParams, T=T, K=K, W=W, C=C, d0=d0, nc=nc, heads=heads, seed=seed)
        x = torch.rand(B, T, K, C, generator=g)
        y = torch.randint(0, nc, (B,), generator=g)
        fx = record(model, hp, x, y, crit, [T, K, C, d0, nc, B, seed, W])
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **fx)
        print(name, os.path.getsize(os.path.join(HERE, name + ".npz")) // 1024, "KiB")


if __name__ == "__main__":
    main()
