#!/usr/bin/env python3
"""Generate the checkpoint-interchange fixture `checkpoint_ref.npz` from the REFERENCE model (development container only).

Run:  python tests/golden/make_fixtures_checkpoint.py        (needs the reference tree, see make_fixtures.py)

The checkpoint tests (tests/test_checkpoint_cpu.py, tests/test_host_cpu.py) compare this backend's state_dict, optimizer
state and training trajectory with the reference's.  What the reference contributes to them is recorded here as data,
so the tests run without the reference tree:

  <tag>.keys / .ndim / .dims / .dtypes      state_dict key order, shapes and dtypes of a reference `Model`
  <tag>.params / .requires_grad            named_parameters() order and which parameters train
  <tag>.buf.<key>                          the derived buffers (attention masks, PE table, adjacency mask)
  <tag>.adj_mat / .arg_types               the Params object's adjacency and the types of get_model_params()
  traj.*                                   a 20-step AdamW + CosineAnnealingLR run of the reference model: loss and
                                           learning rate per step, and a digest of every trainable parameter after
                                           the last step (norm and sum, 4 +-1 projections, a fixed sample of entries)
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_fixtures import forced_thresholds, import_reference, probe_vectors  # noqa: E402
from oracle import hwgat_oracle as O  # noqa: E402

# (tag, family, src_len, num_class): the T=64 models of test_host_cpu.py, the T=16 pair of test_checkpoint_cpu.py
STRUCTURES = (("HWGATE_T64", "HWGATE", 64, 11), ("HGATE_T64", "HGATE", 64, 11), ("WGATE_T64", "WGATE", 64, 11),
              ("HWGATE_T16_nc11", "HWGATE", 16, 11), ("HWGATE_T16_nc7", "HWGATE", 16, 7))
SAMPLE = 1024          # entries per parameter kept by the trajectory digest


def sample_index(name, n, k=SAMPLE):
    """the fixed entries of a flattened parameter the digest keeps (a function of the name and size only)"""
    import zlib
    if n <= k:
        return np.arange(n)
    rs = np.random.RandomState((zlib.crc32(name.encode()) ^ 0x5A5A5A5A) & 0x7FFFFFFF)
    return np.sort(rs.choice(n, k, replace=False))


def structure(tag, family, T, nc):
    mod = importlib.import_module("models." + family)
    par = importlib.import_module("models.model_params")
    rp = getattr(par, family + "Params")({"src_len": T, "num_class": nc}, 2, torch.device("cpu"))
    model = mod.Model(*rp.get_model_params())
    sd = model.state_dict()
    params = dict(model.named_parameters())
    out = {f"{tag}.keys": np.array(list(sd)),
           f"{tag}.ndim": np.array([v.dim() for v in sd.values()], dtype=np.int64),
           f"{tag}.dims": np.array([d for v in sd.values() for d in v.shape], dtype=np.int64),
           f"{tag}.dtypes": np.array([str(v.dtype).replace("torch.", "") for v in sd.values()]),
           f"{tag}.params": np.array(list(params)),
           f"{tag}.requires_grad": np.array([p.requires_grad for p in params.values()]),
           f"{tag}.adj_mat": rp.adj_mat.numpy(),
           f"{tag}.arg_types": np.array([type(a).__name__ for a in rp.get_model_params()])}
    for k, v in sd.items():
        if k not in params:
            out[f"{tag}.buf.{k}"] = v.numpy()
    return out


def trajectory():
    """the reference side of test_checkpoint_cpu.py::test_twenty_adamw_cosine_steps_reference_equals_oracle"""
    Model, Params, Loss = import_reference()
    T, nW, C, nc, B, steps = 16, 2, 2, 6, 4, 20
    cfg = dict(kp_dim=C, temporal_dim=T, num_classes=nc, embed_dim=128, num_kps=nW * 16)
    params = O.synth_params(31, **cfg)
    rp = Params({"src_len": T, "num_class": nc}, C, torch.device("cpu"))
    rp.num_kps, rp.drop_rate = nW * 16, 0.0
    rp.edges = [rp.edges[0]] * nW
    rp.adj_mat = torch.tensor(rp.get_adj_mat(), dtype=torch.float32)
    ref = Model(*rp.get_model_params())
    ref.load_state_dict(params, strict=False)
    ref.train()
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, T, nW * 16, C, generator=g)
    y = torch.randint(0, nc, (B,), generator=g)
    thr = [[0.25 + 0.03 * ((s + k) % 7) for k in range(8)] for s in range(steps)]
    crit = Loss()
    opt = torch.optim.AdamW(ref.parameters(), lr=5e-4)                                          # utils.py:76
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=20, last_epoch=-1)              # utils.py:86
    loss_l, lr_l = [], []
    for s in range(steps):
        opt.zero_grad()
        with forced_thresholds(thr[s]):
            loss = crit(ref(x), y)
        loss.backward()
        opt.step()
        lr_l.append(opt.param_groups[0]["lr"])
        sch.step()
        loss_l.append(loss.item())
    out = {"traj.loss": np.array(loss_l, dtype=np.float64), "traj.lr": np.array(lr_l, dtype=np.float64)}
    for name, p in ref.named_parameters():
        if not p.requires_grad:
            continue
        w = p.detach().double().flatten()
        out["traj.pn." + name] = np.array([w.norm().item(), w.sum().item()], dtype=np.float64)
        out["traj.pp." + name] = probe_vectors(name, w.numel()) @ w.numpy()
        out["traj.ps." + name] = w.numpy()[sample_index(name, w.numel())].astype(np.float32)
    return out


def main():
    torch.manual_seed(1001)
    fx = trajectory()                       # first: puts the reference tree on sys.path
    for s in STRUCTURES:
        fx.update(structure(*s))
    path = os.path.join(HERE, "checkpoint_ref.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
