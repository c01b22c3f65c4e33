#!/usr/bin/env python3
"""Bit-for-bit A/B of the cross-entropy family (csrc/loss_eval.hip and its launchers) between this tree and another built
tree (argv[1], e.g. the parent commit's, built in a scratch copy), one child process per run on one GPU.  Each child
imports the package of ITS tree and records, from fixed seeds, the SHA-256 of every output's bytes:

  kernels  the eight entry points through the public launchers (sce_* / bsce_* / mbsce_* / kd_* forward and backward),
           every output buffer handed in prefilled, so what a launch leaves unwritten is compared as well.  Shapes: the
           KERNEL_CASES of the tests (logits on and one float past a 16-byte boundary), (64, 2002), (300, 10) and rows one
           and four floats longer than each LDS staging limit; (offset, n_rows) in (0, b), (3, b + 1), (0, b + 4); eps in
           0 / 0.01 / 0.3; (alpha, tau) of the tests' HYPER and (0, 4), with and without a pair; and one batch with two bad
           targets and a NaN logit
  steps    two eager and two graphed steps (a full and a short batch) of the tiny HGATE model under
           FusedSmoothedCrossEntropyLoss, ragged=True, mixer=, distiller= and mixer= + distiller=: the loss, the counts and
           every parameter

The driver runs the other tree twice and this tree once, compares other against other (the floor: it must be 0) and other
against this, and writes the entry counts and "N differ" for both.

  python tools/loss_args_ab.py OTHER_TREE [--other-label "the parent commit"] [--txt profiles/loss_args_ab.txt]
"""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 420                                  # seconds per child
CASES = [(3, 7, 0), (5, 2002, 0), (4, 2003, 1), (3, 2004, 0), (3, 2004, 1),                  # tests/test_gpu_graph_micro.py
         (4, 5, 0), (3, 67, 1), (2, 4095, 1), (2, 4096, 0), (2, 4100, 0),                    # tests/test_gpu_distill.py
         (64, 2002, 0), (300, 10, 0),
         (2, 4097, 0), (2, 8193, 0), (2, 8196, 0), (2, 8196, 1)]                             # past KD_ / SCE_LDS_FLOATS
EPS = [0.0, 0.01, 0.3]
HYPER = [(0.5, 0.25), (0.5, 1.0), (1.0, 4.0), (0.3, 32.0), (0.0, 4.0)]
MIXED = dict(mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.8, cutmix_share=0.5, seed=5)
B_STEP, FEED = 6, [6, 5]


def child(root, out_path):
    import torch
    sys.path.insert(0, root)
    hw = importlib.import_module("sl-hwgat_amd")
    train = importlib.import_module("sl-hwgat_amd.train")
    optim = importlib.import_module("sl-hwgat_amd.optim")
    HF = hw.functional
    dev = torch.device("cuda:0")
    dump = {}

    def put(name, *tensors):
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().reshape(-1).cpu().view(torch.uint8).numpy().tobytes())
        assert name not in dump, name
        dump[name] = h.hexdigest()

    def word(n):
        return torch.tensor([n], device=dev, dtype=torch.int32)

    def shifted(t, shift):
        flat = torch.zeros(t.numel() + 4, device=dev)
        v = flat[shift:shift + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    def outs(b, form):
        """prefilled output tuples in the launchers' order"""
        f = lambda n=b: torch.full((n,), 7.5, device=dev)                                      # noqa: E731
        i = lambda n=b: torch.full((n,), -9, device=dev, dtype=torch.int32)                    # noqa: E731
        l = lambda: torch.full((1,), -9, device=dev, dtype=torch.int64)                        # noqa: E731
        out = (f(1), f(), f(), i(), i())
        if form >= 1:
            out += (l(), i(1))
        if form >= 2:
            out += (f(), i())
        if form >= 3:
            out += (f(), f(), f(), i(), f(1), l(), l())
        return out

    def kernels(tag, z, u, y, y_b, lam, conds):
        b, C = z.shape
        g_up = torch.tensor([0.37], device=dev)
        state = HF.kd_state(dev)
        dz = lambda: torch.full((b, C), 7.5, device=dev)                                       # noqa: E731
        for eps in EPS:
            for nv in [None] + sorted({max(0, min(b, n - o)) for o, n in conds}):
                t = f"{tag} eps {eps} n_valid {nv}"
                w = None if nv is None else word(nv)
                out = HF.sce_forward(z, y, eps, w, out=outs(b, 0))
                put(t + " sce fwd", *out)
                put(t + " sce bwd", HF.sce_backward(z, y, out[2], g_up, eps, w, out=dz()))
            for o, n in conds:
                t = f"{tag} eps {eps} offset {o} n_rows {n}"
                out = HF.bsce_forward(z, y, eps, word(n), o, out=outs(b, 1))
                put(t + " bsce fwd", *out)
                put(t + " bsce bwd", HF.bsce_backward(z, y, out[2], g_up, eps, word(n), o, out=dz()))
                out = HF.mbsce_forward(z, y, y_b, lam, eps, word(n), o, out=outs(b, 2))
                put(t + " mbsce fwd", *out)
                put(t + " mbsce bwd", HF.mbsce_backward(z, y, y_b, lam, out[2], g_up, eps, word(n), o, out=dz()))
                for alpha, tau in HYPER:
                    HF.kd_set(state, alpha, tau)
                    for pair in ((None, None), (y_b, lam)):
                        tt = f"{t} alpha {alpha} tau {tau} pair {pair[0] is not None}"
                        out = HF.kd_forward(z, u, y, *pair, state, eps, word(n), o, out=outs(b, 3))
                        put(tt + " kd fwd", *out)
                        put(tt + " kd bwd", HF.kd_backward(z, u, y, *pair, state, out[2], out[9], out[10], g_up, eps, word(n), o,
                                                           out=dz()))

    for b, C, shift in CASES:
        g = torch.Generator().manual_seed(1000 * b + C + shift)
        z = shifted(torch.randn(b, C, generator=g), shift)
        u = shifted(torch.randn(b, C, generator=g) * 1.5, shift)
        y = torch.randint(0, C, (b,), generator=g).to(dev)
        y_b = torch.randint(0, C, (b,), generator=g).to(dev)
        lam = torch.rand(b, generator=g).to(dev)
        lam[0] = 1.0
        kernels(f"{b}x{C}+{shift}", z, u, y, y_b, lam, [(0, b), (3, b + 1), (0, b + 4)])
    # bad targets (rows 1 and 3; the partner's in row 0) and a NaN logit (row 2)
    b, C = 5, 2002
    g = torch.Generator().manual_seed(77)
    z, u = torch.randn(b, C, generator=g), torch.randn(b, C, generator=g)
    z[2, 4] = float("nan")
    y = torch.randint(0, C, (b,), generator=g)
    y_b = torch.randint(0, C, (b,), generator=g)
    y[1], y[3], y_b[0] = -1, C, C + 5
    kernels("bad", z.to(dev), u.to(dev), y.to(dev), y_b.to(dev), torch.rand(b, generator=g).to(dev), [(0, b)])

    # ---- whole steps of the tiny HGATE model
    def tiny(seed):
        torch.manual_seed(seed)
        hp = hw.HGATEParams({"src_len": 16, "num_class": 7}, 2, dev)
        m = hw.HGATEModel(*hp.get_model_params()).to(dev).train()
        m.deterministic_train = True
        return m

    def steps(tag, graphed, **kw):
        m = tiny(11)
        gen = torch.Generator(device=dev).manual_seed(3)
        x = torch.rand(B_STEP, m.temporal_dim, m.num_kps, m.kp_dim, device=dev, generator=gen)
        y = torch.randint(0, 7, (B_STEP,), device=dev, generator=gen)
        opt = optim.DeviceAdamW(list(m.parameters()), lr=5e-4)
        if kw.pop("distill", False):
            kw["distiller"] = train.Distiller(tiny(23), alpha=0.5, temperature=4.0)
        if kw.pop("mix", False):
            kw["mixer"] = train.BatchMixer(**MIXED)
        ragged = kw.pop("ragged", False)
        torch.manual_seed(11)
        if graphed:
            s = train.GraphedTrainStep(m, opt, x, y, ragged=ragged, **kw)
        else:
            s = train.TrainStep(m, opt, pad_to=B_STEP if ragged else None, **kw)
        for k, n in enumerate(FEED if ragged else [B_STEP] * 2):
            put(f"{tag} step {k} loss", s(x[:n], y[:n]))
            for name in ("correct", "kd", "agree", "teacher_correct"):
                v = getattr(s, name, None)
                if torch.is_tensor(v):
                    put(f"{tag} step {k} {name}", v)
        for name, p in m.named_parameters():
            put(f"{tag} param {name}", p)

    for graphed in (False, True):
        how = "graphed" if graphed else "eager"
        steps(f"{how} fused", graphed, criterion=train.FusedSmoothedCrossEntropyLoss())
        steps(f"{how} ragged", graphed, micro_batch=4, ragged=True)
        steps(f"{how} mixer", graphed, micro_batch=4, ragged=True, mix=True)
        steps(f"{how} distiller", graphed, micro_batch=4, ragged=True, distill=True)
        steps(f"{how} mixer distiller", graphed, micro_batch=4, ragged=True, mix=True, distill=True)
    torch.cuda.synchronize()
    with open(out_path, "w") as fh:
        json.dump(dump, fh)
    return 0


def compare(a, b):
    """(entries compared, the names that differ)"""
    if list(a) != list(b):
        return 0, sorted(set(a) ^ set(b)) or ["the same entries in another order"]
    return len(a), [k for k in a if a[k] != b[k]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other", nargs="?", help="the other tree's directory (built)")
    ap.add_argument("--other-label", help="what to call the other tree in the report (default: its path from this tree)")
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "loss_args_ab.txt"))
    ap.add_argument("--child", nargs=2, metavar=("TREE", "OUT"), help="(internal) dump TREE's results into OUT")
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if not args.other:
        ap.error("the other tree's directory is required")
    import tempfile
    tmp = tempfile.mkdtemp(prefix="loss_ab_")
    other = os.path.abspath(args.other)
    dumps = []
    for name, root in (("other1", other), ("other2", other), ("this", ROOT)):        # this process never opens the GPU
        out = os.path.join(tmp, name + ".json")
        res = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", root, out],
                             capture_output=True, text=True)
        if res.returncode != 0:
            print(f"the child of {root} ended with status {res.returncode}; nothing was started after it\n" + res.stderr[-3000:])
            return 1
        with open(out) as fh:
            dumps.append(json.load(fh))
    text = [f"loss_args_ab: {args.other_label or 'the tree at ' + os.path.relpath(other, ROOT)} against this tree, one child "
            "process per run, other / other / this"]
    bad = 0
    for what, (a, b) in (("other run 1 vs other run 2", dumps[:2]), ("other vs this tree", dumps[1:])):
        n, diff = compare(a, b)
        kern = sum(k.endswith(("fwd", "bwd")) for k in a)
        text.append(f"{what}: {n} entries compared ({kern} kernel outputs, {n - kern} step losses / counts / parameters), "
                    f"{len(diff)} differ")
        text += [f"  DIFFERS {k}" for k in diff[:20]]
        bad += len(diff)
    print("\n".join(text))
    with open(args.txt, "w") as fh:
        fh.write("\n".join(text) + "\n")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
