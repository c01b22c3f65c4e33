#!/usr/bin/env python3
"""Byte-for-byte A/B of the two GCN baselines (ST-GCN, DecoupledGCN) between this tree and another built tree (argv[1],
e.g. the parent commit's, built in a scratch copy), one child process per tree on one GPU.  Each child imports the package
of ITS tree and dumps, from fixed seeds:

  kernels  stgcn_aggregate / _backward and dgcn_aggregate / _backward at the shapes of the tests and at the three stage
           shapes of the labs (B 64, T 128 / 64 / 32, V 29, C 64 / 128 / 256; 8 groups for DecoupledGCN)
  models   each model from its Params.get_model_params() at B 8, T 32: logits, loss and every gradient of one eager train
           step; all parameters and buffers and the eval logits after two eager TrainStep calls, and the same after two
           GraphedTrainStep replays from the same start.  DecoupledGCN runs at its default keep_prob 0.9 (DropGraph
           draws), and its eager step once more at keep_prob 1
  calls    the ordered (entry point, non-pointer arguments) list that the library saw for the eager train step and for
           one eval forward

The driver compares the two dumps and prints the tensor count, the byte count and "all equal", or the first difference.

  python tools/gcn_unify_ab.py OTHER_TREE [--txt profiles/gcn_unify_ab.txt]
"""
import argparse
import ctypes
import importlib
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300                                  # seconds per child
B, T, V, NCLASS = 8, 32, 29, 2002
STGCN_SHAPES = [(10, 29, 64), (10, 32, 128), (10, 17, 64), (513, 29, 64), (64 * 128, 29, 64), (64 * 64, 29, 128),
                (64 * 32, 29, 256)]                                           # (frames, V, C)
DGCN_SHAPES = [(1, 29, 64, 8), (58, 32, 128, 4), (58, 17, 64, 1), (58, 29, 256, 8), (129, 29, 64, 8), (300, 32, 128, 4),
               (64 * 128, 29, 64, 8), (64 * 64, 29, 128, 8), (64 * 32, 29, 256, 8)]      # (frames, V, C, groups)


def child(root, out_path):
    sys.path.insert(0, root)
    hw = importlib.import_module("sl-hwgat_amd")
    train = importlib.import_module("sl-hwgat_amd.train")
    HF, lib = hw.functional, hw._lib
    dev = torch.device("cuda:0")
    dump, log = {}, None

    def put(name, t):
        dump[name] = t.detach().cpu().clone()

    plain_call = lib.call

    def logged_call(name, *args):
        if log is not None:
            log.append((name, tuple(a for a, c in zip(args, lib._SIGS[name]) if c is not ctypes.c_void_p)))
        return plain_call(name, *args)

    lib.call = logged_call

    # ---- the aggregation pairs
    g = torch.Generator().manual_seed(1)
    for NT, Vn, C in STGCN_SHAPES:
        y = torch.randn(1, NT, Vn, 3 * C, generator=g).to(dev)
        d = torch.randn(1, NT, Vn, C, generator=g).to(dev)
        A = (torch.rand(3, Vn, Vn, generator=g) * (torch.rand(3, Vn, Vn, generator=g) < 0.3).float()).to(dev)
        E = (1.0 + 0.3 * torch.randn(3, Vn, Vn, generator=g)).to(dev)
        tag = f"stgcn agg {NT}x{Vn}x{C}"
        put(tag + " fwd", HF.stgcn_aggregate(y, A, E))
        put(tag + " fwd no E", HF.stgcn_aggregate(y, A, None))
        dy, dE = HF.stgcn_aggregate_backward(y, d, A, E, True)
        put(tag + " dy", dy)
        put(tag + " dE", dE)
    for NT, Vn, C, G in DGCN_SHAPES:
        y = torch.randn(1, NT, Vn, 3 * C, generator=g).to(dev)
        d = torch.randn(1, NT, Vn, C, generator=g).to(dev)
        An = (torch.rand(3, G, Vn, Vn, generator=g) * (torch.rand(3, G, Vn, Vn, generator=g) < 0.3).float()).to(dev)
        tag = f"dgcn agg {NT}x{Vn}x{C}/{G}"
        put(tag + " fwd", HF.dgcn_aggregate(y, An, G))
        dy, dAn = HF.dgcn_aggregate_backward(y, d, An, G, True)
        put(tag + " dy", dy)
        put(tag + " dAn", dAn)

    # ---- the models
    x = torch.rand(B, T, V, 2, generator=g).to(dev)
    target = torch.randint(0, NCLASS, (B,), generator=g).to(dev)
    crit = train.SmoothedCrossEntropyLoss()

    def fresh(kind):
        torch.manual_seed(0)
        cls, par = (hw.STGCNModel, hw.STGCNParams) if kind == "stgcn" else (hw.DecoupledGCNModel, hw.DecoupledGCNParams)
        m = cls(*par({"num_class": NCLASS}, 2).get_model_params()).to(dev).train()
        opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
        return m, opt

    def state(tag, m):
        for k, v in m.state_dict().items():
            put(f"{tag} state {k}", v)
        m.eval()
        with torch.no_grad():
            put(f"{tag} eval logits", m(x))
        m.train()

    for kind, extra in (("stgcn", ()), ("dgcn", ()), ("dgcn keep 1", (1.0,))):
        m, opt = fresh(kind.split()[0])
        log = []
        logits = m(x, *extra)
        loss = crit(logits, target)
        loss.backward()
        dump[f"{kind} calls train step"], log = log, None
        put(f"{kind} logits", logits)
        put(f"{kind} loss", loss)
        for k, p in m.named_parameters():
            if p.grad is not None:
                put(f"{kind} grad {k}", p.grad)
        if extra:
            continue
        m.eval()
        log = []
        with torch.no_grad():
            m(x)
        dump[f"{kind} calls eval forward"], log = log, None
        m, opt = fresh(kind)
        step = train.TrainStep(m, opt)
        for _ in range(2):
            step(x, target)
        state(f"{kind} eager x2", m)
        m, opt = fresh(kind)
        step = train.GraphedTrainStep(m, opt, x, target)
        for _ in range(2):
            step(x, target)
        state(f"{kind} graphed x2", m)
    torch.cuda.synchronize()
    torch.save(dump, out_path)
    return 0


def compare(a, b):
    """(tensors, bytes, None) or (.., .., the first difference)"""
    if list(a) != list(b):
        return 0, 0, f"the dumps hold different entries: {sorted(set(a) ^ set(b))[:6]}"
    n = nbytes = 0
    for k in a:
        u, v = a[k], b[k]
        if isinstance(u, list):
            if u != v:
                i = next((i for i, (p, q) in enumerate(zip(u, v)) if p != q), min(len(u), len(v)))
                return n, nbytes, f"{k}: call {i} differs: {u[i:i + 1]} against {v[i:i + 1]} ({len(u)} / {len(v)} calls)"
            continue
        if u.dtype != v.dtype or u.shape != v.shape:
            return n, nbytes, f"{k}: {u.dtype} {tuple(u.shape)} against {v.dtype} {tuple(v.shape)}"
        ub, vb = u.contiguous().view(-1).view(torch.uint8), v.contiguous().view(-1).view(torch.uint8)
        if not torch.equal(ub, vb):
            i = int((u.reshape(-1) != v.reshape(-1)).nonzero()[0]) if u.numel() else 0
            return n, nbytes, f"{k}: differs first at flat index {i}: {u.reshape(-1)[i].item()!r} against {v.reshape(-1)[i].item()!r}"
        n, nbytes = n + 1, nbytes + ub.numel()
    return n, nbytes, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other", nargs="?", help="the other tree's directory (built)")
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "gcn_unify_ab.txt"))
    ap.add_argument("--child", nargs=2, metavar=("TREE", "OUT"), help="(internal) dump TREE's results into OUT")
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if not args.other:
        ap.error("the other tree's directory is required")
    import tempfile
    tmp = tempfile.mkdtemp(prefix="gcn_ab_")
    dumps = []
    for name, root in (("other", os.path.abspath(args.other)), ("this", ROOT)):      # this process never opens the GPU
        out = os.path.join(tmp, name + ".pt")
        res = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", root, out],
                             capture_output=True, text=True)
        if res.returncode != 0:
            print(f"the child of {root} ended with status {res.returncode}; nothing was started after it\n" + res.stderr[-3000:])
            return 1
        dumps.append(torch.load(out, weights_only=False))
    n, nbytes, diff = compare(*dumps)
    calls = {k: len(v) for k, v in dumps[1].items() if isinstance(v, list)}
    text = [f"gcn_unify_ab: the tree at {os.path.relpath(args.other, ROOT)} against this tree, one child process each",
            f"tensors compared {n}, bytes compared {nbytes}",
            "call lists: " + ", ".join(f"{k} {v}" for k, v in calls.items()),
            "all equal" if diff is None else "FIRST DIFFERENCE " + diff]
    print("\n".join(text))
    with open(args.txt, "w") as fh:
        fh.write("\n".join(text) + "\n")
    return 0 if diff is None else 1


if __name__ == "__main__":
    sys.exit(main())
