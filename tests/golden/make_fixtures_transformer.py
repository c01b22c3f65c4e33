#!/usr/bin/env python3
"""Golden vectors for the Transformer baseline, from the REFERENCE (development container only).

Run:  python tests/golden/make_fixtures_transformer.py        (needs the reference checkout, see make_fixtures.py)

For each config of tests/transformer_helpers.CONFIGS -- (a) the TransformerParams defaults at T = 64, B = 4 with a
tail-padded, a scattered-padded and an entirely padded clip; (b) d 128, 2 heads, FF 256, 2 layers, C = 3 (F = 87),
T = 37, 'concat'; (c) the same with 'max' -- the reference `Model` gets the seeded weights of
transformer_helpers.recipe_weights (so the files hold no weight tensors) and records, in eval mode on the CPU:
eval logits, every 8th frame of each encoder layer's output, the smoothed-CE loss and the gradient digests
(gh. / gn. / gp., helpers.grad_digest_check) of one backward, and the state_dict structure.  The fp64 restatement of
transformer_helpers is checked against the reference here as well.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_fixtures import REF, grad_digest  # noqa: E402
import transformer_helpers as TH  # noqa: E402


def main():
    sys.path.insert(0, REF)
    from models.Transformer import Model                               # noqa
    from losses.SmoothCrossEntropy import SmoothedCrossEntropyLoss      # noqa
    crit = SmoothedCrossEntropyLoss()
    torch.manual_seed(1005)
    for name, cfg in TH.CONFIGS.items():
        model = Model(*TH.model_args(cfg))
        w = TH.recipe_weights(model.state_dict(), cfg["seed"])
        model.load_state_dict(w, strict=False)
        model.eval()
        x, y = TH.make_input(cfg)
        outs = []
        hooks = [lay.register_forward_hook(lambda m, i, o: outs.append(o.detach()))
                 for lay in model.transformer_encoder.layers]
        logits = model(x)
        for hk in hooks:
            hk.remove()
        loss = crit(logits, y)
        loss.backward()
        ref_layers = []
        mine = TH.restate(w, x, cfg, per_layer=ref_layers)
        err = ((mine - logits.double()).abs().max() / logits.double().abs().max()).item()
        assert err < 1e-5, (name, err)
        assert abs(TH.smoothed_ce(logits.detach(), y).item() - loss.item()) < 1e-6
        fx = {"x": x.numpy(), "y": y.numpy(), "logits": logits.detach().numpy(), "loss": np.array(loss.item())}
        for i, o in enumerate(outs):
            fx[f"layer{i}"] = o[:, ::8].numpy()
        fx.update(grad_digest(model))
        fx.update({"sd." + k: v for k, v in TH.structure(model).items()})
        path = os.path.join(HERE, f"transformer_{name}.npz")
        np.savez_compressed(path, **fx)
        print(name, os.path.getsize(path) // 1024, "KiB", "restatement err", err)


if __name__ == "__main__":
    main()
