#!/usr/bin/env python3
"""Golden vectors for the ST-GCN baseline, from the REFERENCE (development container only).

Run:  python tests/golden/make_fixtures_stgcn.py [names]        (needs the reference checkout, see make_fixtures.py)

For each config of tests/stgcn_helpers.CONFIGS the reference `Model` gets the seeded weights of
stgcn_helpers.fixture_weights (the files hold no weight tensors) and records, in fp32 on the CPU:
  eval.*   eval-mode logits, smoothed-CE loss and gradient digests (gh. / gn. / gp., helpers.grad_digest_check)
  train.*  the same in train mode (head dropout 0, batch statistics), strided samples of the ten block outputs
           (train.block{i}) and the running statistics after the step (train.stat.<key>)
  refdev.* the reference's own fp32-vs-fp64 deviation of every recorded quantity (relative L2; zero-gradient biases
           relative to the matching weight gradient's norm)
  margin   the smallest |ReLU input| over all 20 ReLUs of the fp64 reference (forward pre-hooks), train and eval forward
  sd.*     the state_dict structure
The fp64 restatement of stgcn_helpers is asserted against the fp64 reference (< 1e-9) on every recorded quantity.

Tight fixtures (a, b, c) walk 60 input seeds (and on, 60 at a time up to 600, while none qualifies), rank them by margin
and keep the best one whose margin is >= 2e-6 and whose gradient refdev is < 2e-5 (refusing to write the fixture
otherwise); ranking and margins are stored.  The wide fixture (d)
takes the first seed and also measures, over 20 input seeds of its shape, the largest gradient refdev (ReLU flips
included): `wiring_bound` = 4 x that.  Fixture (a) also carries the fp32-vs-fp64 drift of 20 AdamW steps (worst of 5
input seeds): `adamw.loss_dev`, `adamw.w_dev`.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_fixtures import REF, grad_digest  # noqa: E402
import stgcn_helpers as SH  # noqa: E402

N_SEEDS_TIGHT, N_SEEDS_MAX, N_SEEDS_WIDE, MIN_MARGIN, MAX_REFDEV = 60, 600, 20, 2e-6, 2e-5


def rel(a, b, floor=0.0):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), floor, 1e-300))


def run(model, x, y, crit, training, want_blocks=False):
    """(logits, loss, {name: grad}, margin, block outputs (N, T, V, C), state after) of one forward + backward"""
    model.train(training)
    model.zero_grad()
    state = {"margin": float("inf")}
    blocks = []

    def pre(_m, inp):
        state["margin"] = min(state["margin"], float(inp[0].detach().abs().min()))

    hooks = [m.register_forward_pre_hook(pre) for m in model.modules() if isinstance(m, torch.nn.ReLU)]
    if want_blocks:
        hooks += [b.register_forward_hook(lambda _m, _i, o: blocks.append(o[0].detach().permute(0, 2, 3, 1).clone()))
                  for b in model.st_gcn_networks]
    logits = model(x)
    for h in hooks:
        h.remove()
    loss = crit(logits, y)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    return logits.detach(), loss.detach(), grads, state["margin"], blocks


def grad_refdev(g32, g64):
    zero = SH.zero_grad_biases(g64)
    out = {}
    for n in g64:
        floor = float(g64[zero[n]].double().norm()) if n in zero else 0.0
        out[n] = rel(g32[n], g64[n], floor)
    return out


def build(Model, cfg):
    model = Model(*SH.model_args(cfg, dropout=0.0))
    w = SH.fixture_weights(model.state_dict(), cfg)
    missing = model.load_state_dict(w, strict=False)
    assert missing.missing_keys == ["A"] and not missing.unexpected_keys, missing
    return model, w


def both(model, w, x, y, crit, training, want_blocks=False):
    """fp32 and fp64 runs from the recipe weights (the running statistics are restored before each)"""
    out = []
    for dt in (torch.float32, torch.float64):
        m = copy.deepcopy(model).to(dt)
        out.append(run(m, x.to(dt), y, crit, training, want_blocks) + (m.state_dict(),))
    return out


def check_restatement(w, A, x, y, cfg, training, r64):
    logits, loss, grads, margin, blocks, sd = r64
    rec = SH.Record()
    params = dict(w, A=A)
    lg, ls, gs = SH.grads_of(params, x, y, cfg, training, rec=rec)
    assert rel(lg, logits) < 1e-9 and abs(float(ls) - float(loss)) < 1e-9, ("logits", rel(lg, logits))
    zero = SH.zero_grad_biases(grads)
    for n, g in grads.items():
        floor = float(grads[zero[n]].norm()) if n in zero else 0.0
        assert rel(gs[n], g, floor) < 1e-9, (n, rel(gs[n], g, floor))
    assert abs(rec.margin - margin) <= 1e-9 * max(1.0, margin), (rec.margin, margin)
    for a, b in zip(rec.blocks, blocks):
        assert rel(a, b) < 1e-9
    if training:
        for k, v in rec.stats.items():
            assert rel(v, sd[k]) < 1e-9, k
    # masks fed back: the same gradients
    _, _, gs2 = SH.grads_of(params, x, y, cfg, training, masks=rec.masks)
    assert all(torch.equal(gs[n], gs2[n]) for n in gs)


def adamw_drift(Model, cfg, crit, steps=20, lr=3e-4, seeds=5):
    worst_loss = worst_w = 0.0
    for s in range(seeds):
        x, y = SH.make_input(cfg, seed=100 + s)
        model, _ = build(Model, cfg)
        ms = [copy.deepcopy(model).to(dt).train() for dt in (torch.float32, torch.float64)]
        opts = [torch.optim.AdamW(m.parameters(), lr=lr) for m in ms]
        for _ in range(steps):
            losses = []
            for m, o, dt in zip(ms, opts, (torch.float32, torch.float64)):
                o.zero_grad()
                loss = crit(m(x.to(dt)), y)
                loss.backward()
                o.step()
                losses.append(float(loss))
            worst_loss = max(worst_loss, abs(losses[0] - losses[1]) / max(1.0, abs(losses[1])))
        for (n, p), (_, q) in zip(ms[0].named_parameters(), ms[1].named_parameters()):
            worst_w = max(worst_w, rel(p.detach(), q.detach()))
    return worst_loss, worst_w


def main():
    sys.path.insert(0, REF)
    from models.STGCN import Model                                      # noqa
    from losses.SmoothCrossEntropy import SmoothedCrossEntropyLoss      # noqa
    crit = SmoothedCrossEntropyLoss()
    torch.manual_seed(1006)
    names = sys.argv[1:] or list(SH.CONFIGS)
    for name in names:
        cfg = SH.CONFIGS[name]
        model, w = build(Model, cfg)
        A = model.A.clone()
        fx = {}
        if cfg["tight"]:
            m64 = copy.deepcopy(model).double()
            margins = []
            s = -1
            while len(margins) < N_SEEDS_TIGHT or (max(margins) < MIN_MARGIN and len(margins) < N_SEEDS_MAX):
                s += 1
                x, y = SH.make_input(cfg, seed=s)
                with torch.no_grad():
                    mg = float("inf")
                    for training in (True, False):
                        mm = copy.deepcopy(m64).train(training)
                        st = {"m": float("inf")}
                        hooks = [r.register_forward_pre_hook(
                            lambda _m, inp, st=st: st.__setitem__("m", min(st["m"], float(inp[0].abs().min()))))
                            for r in mm.modules() if isinstance(r, torch.nn.ReLU)]
                        mm(x.double())
                        for h in hooks:
                            h.remove()
                        mg = min(mg, st["m"])
                margins.append(mg)
            order = sorted(range(len(margins)), key=lambda s: -margins[s])[:N_SEEDS_TIGHT]
            fx["seed_ranking"] = np.array(order, dtype=np.int64)
            fx["seed_margins"] = np.array([margins[s] for s in order])
            candidates = order
        else:
            candidates = [7]
        chosen = None
        for s in candidates:
            x, y = SH.make_input(cfg, seed=s)
            res = {t: both(model, w, x, y, crit, t, want_blocks=t) for t in (True, False)}
            margin = min(res[True][1][3], res[False][1][3])
            dev = {t: grad_refdev(res[t][0][2], res[t][1][2]) for t in (True, False)}
            worst = max(max(d.values()) for d in dev.values())
            print(name, "seed", s, "margin", margin, "worst gradient refdev", worst, flush=True)
            if not cfg["tight"] or (margin >= MIN_MARGIN and worst < MAX_REFDEV):
                chosen = s
                break
        if chosen is None:
            raise SystemExit(f"{name}: no input seed with margin >= {MIN_MARGIN} and gradient refdev < {MAX_REFDEV}")
        fx.update({"y": y.numpy(), "input_seed": np.array(chosen), "margin": np.array(margin), "A": A.numpy()})
        if cfg["tight"]:                       # short clips are stored; stgcn_helpers.fixture_input redraws the long one
            fx["x"] = x.numpy()
        for t, tag in ((True, "train"), (False, "eval")):
            (lg, ls, gs, _, blocks, sd), r64 = res[t][0], res[t][1]
            check_restatement(w, A.double(), x, y, cfg, t, r64)
            fx[f"{tag}.logits"], fx[f"{tag}.loss"] = lg.numpy(), np.array(float(ls))
            fx[f"refdev.{tag}.logits"] = np.array(rel(lg, r64[0]))
            fx[f"refdev.{tag}.loss"] = np.array(abs(float(ls) - float(r64[1])))
            m = copy.deepcopy(model)
            for (n, p) in m.named_parameters():
                p.grad = gs[n]
            fx.update({f"{tag}.{k}": v for k, v in grad_digest(m).items()})
            for n, d in dev[t].items():
                fx[f"refdev.{tag}.g.{n}"] = np.array(d)
            if t:
                for i, (b32, b64) in enumerate(zip(blocks, r64[4])):
                    fx[f"train.block{i}"] = SH.block_samples(b32).numpy()
                    fx[f"refdev.train.block{i}"] = np.array(rel(b32, b64))
                for k, v in sd.items():
                    if "running_" in k or k.endswith("num_batches_tracked"):
                        fx["train.stat." + k] = v.numpy()
                        if v.is_floating_point():
                            fx["refdev.train.stat." + k] = np.array(rel(v, r64[5][k]))
        if not cfg["tight"]:
            worst = 0.0
            for s in range(N_SEEDS_WIDE):
                xs, ys = SH.make_input(cfg, seed=s)
                for t in (True, False):
                    r = both(model, w, xs, ys, crit, t)
                    d = max(grad_refdev(r[0][2], r[1][2]).values())
                    worst = max(worst, d)
                    print(name, "wide seed", s, "train" if t else "eval", "worst gradient refdev", d, flush=True)
            fx["wiring_refdev"] = np.array(worst)
            fx["wiring_bound"] = np.array(4.0 * worst)
        if name == "a":
            ld, wd = adamw_drift(Model, cfg, crit)
            fx["adamw.loss_dev"], fx["adamw.w_dev"] = np.array(ld), np.array(wd)
            print(name, "AdamW drift: loss", ld, "weights", wd, flush=True)
        fx.update({"sd." + k: v for k, v in SH.structure(model).items()})
        path = os.path.join(HERE, f"stgcn_{name}.npz")
        np.savez_compressed(path, **fx)
        print(name, os.path.getsize(path) // 1024, "KiB", "margin", margin, flush=True)


if __name__ == "__main__":
    main()
