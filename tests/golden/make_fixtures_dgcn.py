#!/usr/bin/env python3
"""Golden vectors for the DecoupledGCN baseline, from the REFERENCE (development container only).

Run:  python tests/golden/make_fixtures_dgcn.py [names]        (needs the reference checkout, see make_fixtures.py)

For each config of tests/dgcn_helpers.CONFIGS the reference `Model` gets the seeded weights of
dgcn_helpers.fixture_weights (the files hold no weight tensors) and records, in fp32 on the CPU:
  eval.*   eval-mode logits, smoothed-CE loss and gradient digests (gh. / gn. / gp., helpers.grad_digest_check)
  train.*  the same in train mode (head dropout 0, batch statistics, keep_prob 0.9), strided samples of the ten unit
           outputs (train.block{i}), the running statistics after the step (train.stat.<key>) and the sixteen DropGraph
           probability tensors (train.p.<unit>.<site>)
  refdev.* the reference's own fp32-vs-fp64 deviation of every recorded quantity (relative L2; zero-gradient biases and
           each gate convolution's single bias relative to the absolute sum of its own terms,
           <tag>.gs.<name>, dgcn_helpers.gate_biases; refdev.*.gh.<name>: of a gradient's 48-entry head alone)
  margin   the smallest non-zero |ReLU input| over all 30 ReLUs of the fp64 reference (forward pre-hooks), train and eval
           forward (inputs a DropGraph mask zeroes are exactly 0 in every precision: dgcn_helpers.nonzero_margin)
  A, A_sum the (3, V, V) adjacency of the graph and the frozen lN.A
  sd.*     the state_dict structure
In train runs `torch.bernoulli` is replaced by a function that returns dgcn_helpers.drop_seed_pattern for the draw at hand
and records the probability tensor it was handed.  The fp64 restatement of dgcn_helpers is asserted against the fp64
reference (< 1e-9) on every recorded quantity, the probabilities included, and the adjacency bit for bit; every DropGraph
mask is checked to drop something and to keep something.

Tight fixtures (a, b, c) walk input seeds 0, 1, 2, ... (the first 60, then 480 at a time, up to 30 000; the margins in
parallel worker processes) and take the first seed, in order of margin within what has been walked, whose margin is
>= 2e-6 and whose gradient refdev is < 2e-5 (refusing to write the fixture if there is none); the 60 best margins and
the number of seeds walked are stored.  a and b find theirs within the first 60.  c (T 48) has about 7 million ReLU
inputs over its two forwards, three times those of a: of its first 540 seeds the best margin is 1.40e-6; seed 894
(margin 3.61e-6, gradient refdev 4.1e-6) is the first that qualifies, found with 1020 seeds walked.
The wide fixture (d) takes the first seed and also measures, over 20 input seeds of its shape, the largest
gradient refdev (ReLU flips included): `wiring_bound` = 4 x that.  Fixture (a) also carries the fp32-vs-fp64 drift of 20
AdamW steps (worst of 5 input seeds): `adamw.loss_dev`, `adamw.w_dev`.
"""
import contextlib
import copy
import importlib
import multiprocessing
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_fixtures import REF, grad_digest  # noqa: E402
import dgcn_helpers as DH  # noqa: E402

N_SEEDS_TIGHT, N_SEEDS_CHUNK, N_SEEDS_MAX, N_SEEDS_WIDE, MIN_MARGIN, MAX_REFDEV = 60, 480, 30000, 20, 2e-6, 2e-5
WORKERS = min(8, os.cpu_count() or 1)
_W = {}


def rel(a, b, floor=0.0):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), floor, 1e-300))


@contextlib.contextmanager
def pattern_bernoulli(cfg, probs):
    """torch.bernoulli -> the seed pattern of the draw at hand (four per unit, l7 first); `probs` receives each p"""
    real = torch.bernoulli

    def fake(p, *a, **k):
        unit, site = DH.FIRST_DROP_UNIT + len(probs) // 4, len(probs) % 4
        probs.append(p.detach().clone())
        return DH.drop_seed_pattern(cfg, unit, site, tuple(p.shape)).to(p.dtype)

    torch.bernoulli = fake
    try:
        yield
    finally:
        torch.bernoulli = real


def forward(model, x, cfg, training, probs):
    with pattern_bernoulli(cfg, probs):
        return model(x, DH.KEEP_PROB)


def margin_of(model, x, cfg, training):
    st = {"m": float("inf")}
    hooks = [r.register_forward_pre_hook(lambda _m, inp: st.__setitem__("m", min(st["m"], DH.nonzero_margin(inp[0]))))
             for r in model.modules() if isinstance(r, torch.nn.ReLU)]
    model.train(training)
    out = forward(model, x, cfg, training, [])
    for h in hooks:
        h.remove()
    return st["m"], out


def _init_worker(name):
    """a margin worker: one thread, its own fp64 reference model with the fixture weights"""
    torch.set_num_threads(1)
    sys.path.insert(0, REF)
    from models.DecoupledGCN import Model                               # noqa
    _W["cfg"] = DH.CONFIGS[name]
    _W["m64"] = build(Model, _W["cfg"])[0].double()


def _seed_margin(s):
    x, _ = DH.make_input(_W["cfg"], seed=s)
    with torch.no_grad():
        return min(margin_of(copy.deepcopy(_W["m64"]), x.double(), _W["cfg"], t)[0] for t in (True, False))


def run(model, x, y, crit, cfg, training, want_blocks=False):
    """(logits, loss, {name: grad}, margin, unit outputs (N, T, V, C), probabilities, {gate bias: sum |terms|}) of one
    forward + backward"""
    model.train(training)
    model.zero_grad()
    state = {"margin": float("inf")}
    blocks, probs, terms = [], [], {}

    def pre(_m, inp):
        state["margin"] = min(state["margin"], DH.nonzero_margin(inp[0]))

    hooks = [m.register_forward_pre_hook(pre) for m in model.modules() if isinstance(m, torch.nn.ReLU)]
    if want_blocks:
        hooks += [getattr(model, f"l{i}").register_forward_hook(
            lambda _m, _i, o: blocks.append(o.detach().permute(0, 2, 3, 1).clone())) for i in range(1, 11)]
    # a gate convolution's bias gradient is the plain sum of the gradient at its output: keep the sum of the absolute terms
    hooks += [m.register_full_backward_hook(
        lambda _m, _gi, go, k=n + ".bias": terms.__setitem__(k, float(go[0].detach().double().abs().sum())))
        for n, m in model.named_modules() if n.endswith(("conv_sa", "conv_ta"))]
    logits = forward(model, x, cfg, training, probs)
    loss = crit(logits, y)
    loss.backward()
    for h in hooks:
        h.remove()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return logits.detach(), loss.detach(), grads, state["margin"], blocks, probs, terms


def grad_refdev(r32, r64, training):
    """the fp32 run's deviation from the fp64 run, per gradient (r32, r64: what `both` returns)"""
    g32, g64, terms = r32[2], r64[2], r64[6]
    zero, gate = DH.gradient_floors(g64, training), DH.gate_biases(g64)
    out = {}
    for n in g64:
        if n in gate:
            out[n] = DH.gate_bias_error(g32[n], g64[n], terms[n])[0]
        else:
            out[n] = rel(g32[n], g64[n], float(g64[zero[n]].double().norm()) if n in zero else 0.0)
    return out


def head_refdev(g32, g64):
    """the fp32-vs-fp64 deviation of the 48-entry head of every gradient, measured the way helpers.grad_digest_check
    compares a head (relative to the head's own norm, floored): a gradient whose first entries nearly cancel -- the
    identity partition's share of bn0.bias behind a batch-statistics BatchNorm -- has a head far noisier than its norm"""
    out = {}
    for n in g64:
        a, b = g32[n].double().flatten(), g64[n].double().flatten()
        floor = 1e-3 * max(float(a.norm()), 1e-12) / max(a.numel(), 1) ** 0.5
        out[n] = float((a[:48] - b[:48]).norm() / max(float(a[:48].norm()), floor, 1e-30))
    return out


def build(Model, cfg):
    model = Model(*DH.model_args(cfg, dropout=0.0))
    w = DH.fixture_weights(model.state_dict(), cfg)
    model.load_state_dict(w, strict=True)
    return model, w


def both(model, x, y, crit, cfg, training, want_blocks=False):
    """fp32 and fp64 runs from the recipe weights (the running statistics are restored before each)"""
    out = []
    for dt in (torch.float32, torch.float64):
        m = copy.deepcopy(model).to(dt)
        out.append(run(m, x.to(dt), y, crit, cfg, training, want_blocks) + (m.state_dict(),))
    return out


def check_restatement(w, x, y, cfg, training, r64):
    logits, loss, grads, margin, blocks, probs, terms, sd = r64
    rec, log = DH.Record(), []
    seeds = DH.all_drop_seeds(cfg, x.shape[0], x.shape[1])
    lg, ls, gs = DH.grads_of(w, x, y, cfg, training, rec=rec, seeds=seeds, log=log)
    assert rel(lg, logits) < 1e-9 and abs(float(ls) - float(loss)) < 1e-9, ("logits", rel(lg, logits))
    zero, gate = DH.gradient_floors(grads, training), DH.gate_biases(grads)
    assert set(gs) == set(grads), set(gs) ^ set(grads)
    assert set(rec.terms) == set(terms) == set(gate) and len(gate) == 20
    for n, g in grads.items():
        if n in gate:
            assert abs(rec.terms[n] - terms[n]) < 1e-9 * terms[n], (n, rec.terms[n], terms[n])
            assert DH.gate_bias_error(gs[n], g, terms[n])[0] < 1e-9, n
            continue
        floor = float(grads[zero[n]].norm()) if n in zero else 0.0
        assert rel(gs[n], g, floor) < 1e-9, (n, rel(gs[n], g, floor))
    assert abs(rec.margin - margin) <= 1e-9 * max(1.0, margin), (rec.margin, margin)
    assert len(rec.masks) == 30
    for a, b in zip(rec.blocks, blocks):
        assert rel(a, b) < 1e-9
    if training:
        for k, v in rec.stats.items():
            assert rel(v, sd[k]) < 1e-9, k
        assert len(log) == len(probs) == 16
        for (unit, site, p, s, mask, scale), q in zip(log, probs):
            assert rel(p, q.reshape(p.shape)) < 1e-9, (unit, site)
        assert DH.masks_are_sound(log)
    # masks fed back: the same gradients
    _, _, gs2 = DH.grads_of(w, x, y, cfg, training, masks=rec.masks, seeds=seeds)
    assert all(torch.equal(gs[n], gs2[n]) for n in gs)


def adamw_drift(Model, cfg, crit, steps=20, lr=3e-4, seeds=5):
    worst_loss = worst_w = 0.0
    for s in range(seeds):
        x, y = DH.make_input(cfg, seed=100 + s)
        model, _ = build(Model, cfg)
        ms = [copy.deepcopy(model).to(dt).train() for dt in (torch.float32, torch.float64)]
        opts = [torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=lr) for m in ms]
        for _ in range(steps):
            losses = []
            for m, o, dt in zip(ms, opts, (torch.float32, torch.float64)):
                o.zero_grad()
                loss = crit(forward(m, x.to(dt), cfg, True, []), y)
                loss.backward()
                o.step()
                losses.append(float(loss))
            worst_loss = max(worst_loss, abs(losses[0] - losses[1]) / max(1.0, abs(losses[1])))
        ps, qs = (dict(m.named_parameters()) for m in ms)
        for n, p in ps.items():
            worst_w = max(worst_w, rel(p.detach(), qs[n].detach()))
    return worst_loss, worst_w


def main():
    sys.path.insert(0, REF)
    from models.DecoupledGCN import Model                               # noqa
    from losses.SmoothCrossEntropy import SmoothedCrossEntropyLoss      # noqa
    crit = SmoothedCrossEntropyLoss()
    torch.manual_seed(1007)
    names = sys.argv[1:] or list(DH.CONFIGS)
    hw = None
    for name in names:
        cfg = DH.CONFIGS[name]
        model, w = build(Model, cfg)
        A = np.asarray(model.graph.A)
        fx = {}
        def evaluate(s):
            """fp32 and fp64 reference runs of input seed s in both modes; its margin and worst gradient refdev"""
            x, y = DH.make_input(cfg, seed=s)
            res = {t: both(model, x, y, crit, cfg, t, want_blocks=t) for t in (True, False)}
            margin = min(res[True][1][3], res[False][1][3])
            dev = {t: grad_refdev(res[t][0], res[t][1], t) for t in (True, False)}
            worst = max(max(d.values()) for d in dev.values())
            print(name, "seed", s, "margin", margin, "worst gradient refdev", worst, flush=True)
            return x, y, res, margin, dev, worst

        chosen = None
        if cfg["tight"]:
            margins, tried = {}, set()
            with multiprocessing.get_context("spawn").Pool(WORKERS, _init_worker, (name,)) as pool:
                while chosen is None and len(margins) < N_SEEDS_MAX:
                    todo = range(len(margins), len(margins) + (N_SEEDS_TIGHT if not margins else N_SEEDS_CHUNK))
                    margins.update(zip(todo, pool.map(_seed_margin, todo, chunksize=4)))
                    print(name, len(margins), "seeds walked, best margin", max(margins.values()), flush=True)
                    fresh = sorted((s for s in margins if margins[s] >= MIN_MARGIN and s not in tried), key=lambda s: -margins[s])
                    for s in fresh:
                        tried.add(s)
                        x, y, res, margin, dev, worst = evaluate(s)
                        if margin >= MIN_MARGIN and worst < MAX_REFDEV:
                            chosen = s
                            break
            order = sorted(margins, key=lambda s: -margins[s])[:N_SEEDS_TIGHT]
            fx["seed_ranking"] = np.array(order, dtype=np.int64)
            fx["seed_margins"] = np.array([margins[s] for s in order])
            fx["seeds_walked"] = np.array(len(margins))
        else:
            chosen = 7
            x, y, res, margin, dev, worst = evaluate(chosen)
        if chosen is None:
            raise SystemExit(f"{name}: no input seed with margin >= {MIN_MARGIN} and gradient refdev < {MAX_REFDEV}")
        fx.update({"y": y.numpy(), "input_seed": np.array(chosen), "margin": np.array(margin), "A": A,
                   "A_sum": model.l1.A.detach().numpy()})
        if cfg["tight"]:                       # short clips are stored; fixture_input redraws the long one
            fx["x"] = x.numpy()
        for t, tag in ((True, "train"), (False, "eval")):
            (lg, ls, gs, _, blocks, probs, _, sd), r64 = res[t][0], res[t][1]
            check_restatement(w, x, y, cfg, t, r64)
            fx[f"{tag}.logits"], fx[f"{tag}.loss"] = lg.numpy(), np.array(float(ls))
            fx[f"refdev.{tag}.logits"] = np.array(rel(lg, r64[0]))
            fx[f"refdev.{tag}.loss"] = np.array(abs(float(ls) - float(r64[1])))
            m = copy.deepcopy(model)
            for (n, p) in m.named_parameters():
                p.grad = gs.get(n)
            fx.update({f"{tag}.{k}": v for k, v in grad_digest(m).items()})
            for n, d in dev[t].items():
                fx[f"refdev.{tag}.g.{n}"] = np.array(d)
            for n in DH.gate_biases(gs):
                fx[f"{tag}.gs.{n}"] = np.array(r64[6][n])
            for n, d in head_refdev(gs, r64[2]).items():
                fx[f"refdev.{tag}.gh.{n}"] = np.array(d)
            if t:
                for i, (b32, b64) in enumerate(zip(blocks, r64[4])):
                    fx[f"train.block{i}"] = DH.block_samples(b32).numpy()
                    fx[f"refdev.train.block{i}"] = np.array(rel(b32, b64))
                for k, v in sd.items():
                    if "running_" in k or k.endswith("num_batches_tracked"):
                        fx["train.stat." + k] = v.numpy()
                        if v.is_floating_point():
                            fx["refdev.train.stat." + k] = np.array(rel(v, r64[7][k]))
                for j, (p32, p64) in enumerate(zip(probs, r64[5])):
                    key = f"{DH.FIRST_DROP_UNIT + j // 4}.{j % 4}"
                    fx["train.p." + key] = p32.reshape(p32.shape[0], -1).numpy()
                    fx["refdev.train.p." + key] = np.array(rel(p32, p64))
        if not cfg["tight"]:
            worst = 0.0
            for s in range(N_SEEDS_WIDE):
                xs, ys = DH.make_input(cfg, seed=s)
                for t in (True, False):
                    r = both(model, xs, ys, crit, cfg, t)
                    d = max(grad_refdev(r[0], r[1], t).values())
                    worst = max(worst, d)
                    print(name, "wide seed", s, "train" if t else "eval", "worst gradient refdev", d, flush=True)
            fx["wiring_refdev"] = np.array(worst)
            fx["wiring_bound"] = np.array(4.0 * worst)
        if name == "a":
            ld, wd = adamw_drift(Model, cfg, crit)
            fx["adamw.loss_dev"], fx["adamw.w_dev"] = np.array(ld), np.array(wd)
            print(name, "AdamW drift: loss", ld, "weights", wd, flush=True)
        # the structure record without the bulky constructed entries: frozen parameters are not buffers, so only the
        # running statistics travel
        fx.update({"sd." + k: v for k, v in DH.structure(model).items()})
        # the adjacency, bit for bit, against this backend's own construction
        if hw is None:
            hw = importlib.import_module("sl-hwgat_amd")
        mine = hw.DecoupledGCNModel(*DH.model_args(cfg))
        assert np.array_equal(importlib.import_module("sl-hwgat_amd.models.DecoupledGCN").spatial_graph(cfg["V"], cfg["edges"]), A)
        assert all(torch.equal(v, model.state_dict()[k]) for k, v in mine.state_dict().items() if DH.is_constructed(k))
        assert torch.equal(mine.l3.gcn1.decoupled_A, Model(*DH.model_args(cfg)).l3.gcn1.decoupled_A)
        path = os.path.join(HERE, f"dgcn_{name}.npz")
        np.savez_compressed(path, **fx)
        print(name, os.path.getsize(path) // 1024, "KiB", "margin", margin, flush=True)


if __name__ == "__main__":
    main()
