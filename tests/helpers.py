"""Shared helpers for the parity tests (oracle side only)."""
import os

import numpy as np
import torch

from oracle import hwgat_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# every stage width models/HWGATE.py::width_problem accepts (test_width_cpu.py holds the rule to exactly this list; the
# GPU width tests run the LayerNorm family at every entry)
ALL_WIDTHS = list(range(64, 1025, 64))


def load_fixture(name):
    return dict(np.load(os.path.join(GOLDEN, name)))


def cfg_of(fx, **over):
    T, nW, C, d0, nc, B, seed = [int(v) for v in fx["cfg"]]
    cfg = dict(kp_dim=C, temporal_dim=T, num_classes=nc, embed_dim=d0,
               depths=(2, 2, 4), ff_ratio=2.0, use_pe=True, num_kps=nW * 16, tp=2)
    cfg.update(over)
    return cfg, seed, B


def oracle_from_fixture(fx, dtype=torch.float32):
    cfg, seed, _ = cfg_of(fx)
    wstd = float(fx["wstd"]) if "wstd" in fx else 0.08
    params = {k: v.to(dtype) for k, v in O.synth_params(seed, weight_std=wstd, **cfg).items()}
    model = O.OracleHWGAT(params, num_kps=cfg["num_kps"], temporal_dim=cfg["temporal_dim"])
    return model, params, cfg


def sub(t):
    return t[:, ::5, ::3, ::7]


def natural(t, d):
    """a block output in natural token order (B,F,K,d): the last block of a stage may hand it over already in the
    TemporalMerging layout (B,F/2,K,2d) (fc2 epilogue store, reference HWGATE.py:55-63) -- undo that for comparison"""
    if t.shape[-1] == d:
        return t
    B, f, K, d2 = t.shape
    assert d2 == 2 * d
    return t.view(B, f, K, 2, d).permute(0, 1, 3, 2, 4).reshape(B, 2 * f, K, d)


def rel_err(a, b):
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def entrywise(a, b):
    """largest entry-wise error relative to the largest reference entry"""
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


ATTN_PARTS = ("o", "dq", "dk", "dv")


def attn_parity(out, ref_out, dqkv, ref_dqkv, d, tol_norm, tol_entry, what="", floor=None):
    """Parity of one attention forward + backward against its fp64 reference, part by part: the output o and the three
    gradient parts dq, dk, dv (columns [0, d), [d, 2d), [2d, 3d) of dqkv) are each checked
      - in norm, against that part's own reference norm (< tol_norm), and
      - entry by entry, relative to that part's largest reference entry (< tol_entry),
    so an error confined to one part, one head, one tile or one frame segment cannot hide in a norm over everything.
    tol_norm / tol_entry: a number, or a {part: bound} dict.  floor: {part: tensor} whose norm / largest entry is the
    smallest scale of that part (for parts that are analytically zero).  Returns {part: (norm error, entry error)}."""
    def bound(tol, part):
        return tol[part] if isinstance(tol, dict) else tol

    refs = {"o": ref_out}
    outs = {"o": out}
    for i, part in enumerate(ATTN_PARTS[1:]):
        outs[part] = dqkv[..., i * d:(i + 1) * d]
        refs[part] = ref_dqkv[..., i * d:(i + 1) * d]
    errs = {}
    for part in ATTN_PARTS:
        a = torch.as_tensor(outs[part].detach().cpu(), dtype=torch.float64)
        b = torch.as_tensor(refs[part].detach().cpu(), dtype=torch.float64)
        assert a.shape == b.shape, (what, part, tuple(a.shape), tuple(b.shape))
        norm_scale, entry_scale = b.norm().item(), b.abs().max().item()
        if floor is not None and part in floor:
            fl = torch.as_tensor(floor[part].detach().cpu(), dtype=torch.float64)
            norm_scale, entry_scale = max(norm_scale, fl.norm().item()), max(entry_scale, fl.abs().max().item())
        diff = (a - b).abs()
        e_norm = diff.norm().item() / max(norm_scale, 1e-30)
        flat = int(diff.argmax())
        e_entry = diff.flatten()[flat].item() / max(entry_scale, 1e-30)
        errs[part] = (e_norm, e_entry)
        where = tuple(int(i) for i in np.unravel_index(flat, tuple(a.shape)))
        worst = f"worst entry {where}: {a.flatten()[flat].item():.6g} vs {b.flatten()[flat].item():.6g}"
        tn, te = bound(tol_norm, part), bound(tol_entry, part)
        assert e_norm < tn, f"{what} {part}: norm error {e_norm:.3g} >= {tn:.3g} ({worst})"
        assert e_entry < te, f"{what} {part}: entry-wise error {e_entry:.3g} >= {te:.3g} ({worst})"
    return errs


def tensor_parity(got, ref, *, tol_norm, tol_entry, tol_row=None, tol_col=None, tile=None, tol_tile=None, what=""):
    """Parity of one 2-D result (leading dimensions are flattened) against its fp64 reference, on the reference's device:
      - finite everywhere,
      - in norm over the whole result, as rel_err (< tol_norm),
      - entry by entry, relative to the largest reference entry, as entrywise (< tol_entry),
      - row by row when tol_row is given: the L2 error of each row over the RMS row norm of the reference,
        ref.norm() / sqrt(rows) -- a row that is analytically zero still has a scale (< tol_row),
      - column by column when tol_col is given, in the same way (< tol_col),
      - tile by tile when tile = (th, tw) is given: the error of each th x tw block against that block's own reference
        norm (< tol_tile); ragged edge blocks are checked with what they hold,
    so an error confined to one element, one row (a tail launch), one column (a bias entry) or one tile (a stale or
    misplaced block, a dropped K or M slice) cannot hide in a norm over everything.  Prints the measured values, then
    asserts in the order above; a failure names the metric, the worst row / column / tile / index and the two values
    there.  Returns {"norm", "entry", "row", "col", "tile"} (None where not asked for)."""
    b = torch.as_tensor(ref).detach().to(torch.float64)
    a = torch.as_tensor(got).detach().to(device=b.device, dtype=torch.float64)
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    if a.dim() < 2:
        a, b = a.reshape(1, -1), b.reshape(1, -1)
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    rows, cols = b.shape
    finite = torch.isfinite(a)
    if not bool(finite.all()):
        flat = int((~finite).flatten().int().argmax())
        raise AssertionError(f"{what}: not finite: {int((~finite).sum())} entries, the first at {divmod(flat, cols)}: "
                             f"{a.flatten()[flat].item()} vs {b.flatten()[flat].item():.6g}")
    diff = a - b
    ref_norm = max(b.norm().item(), 1e-30)
    flat = int(diff.abs().argmax())
    at = divmod(flat, cols)
    worst = f"worst entry {at}: {a[at].item():.6g} vs {b[at].item():.6g}"
    errs = dict(norm=diff.norm().item() / ref_norm, entry=diff.abs().flatten()[flat].item() / max(b.abs().max().item(), 1e-30),
                row=None, col=None, tile=None)
    msgs = []
    for key, name, dim, count, tol in (("row", "row", 1, rows, tol_row), ("col", "column", 0, cols, tol_col)):
        if tol is None:
            continue
        e = diff.norm(dim=dim) / (ref_norm / count ** 0.5)
        i = int(e.argmax())
        errs[key] = e[i].item()
        j = int((diff[i] if dim == 1 else diff[:, i]).abs().argmax())
        w = (i, j) if dim == 1 else (j, i)
        msgs.append((key, tol, f"{name} error {errs[key]:.3g} >= {tol:.3g} (worst {name} {i}, its worst entry {w}: "
                               f"{a[w].item():.6g} vs {b[w].item():.6g})"))
    if tile is not None:
        th, tw = tile
        nr, nc = -(-rows // th), -(-cols // tw)
        pad = (0, nc * tw - cols, 0, nr * th - rows)

        def blocks(t):
            return torch.nn.functional.pad(t, pad).view(nr, th, nc, tw).norm(dim=(1, 3))

        e = blocks(diff) / blocks(b).clamp_min(1e-30)
        i = int(e.argmax())
        ti = divmod(i, nc)
        errs["tile"] = e.flatten()[i].item()
        sub = diff[ti[0] * th:(ti[0] + 1) * th, ti[1] * tw:(ti[1] + 1) * tw].abs()
        j = divmod(int(sub.argmax()), sub.shape[1])
        w = (ti[0] * th + j[0], ti[1] * tw + j[1])
        msgs.append(("tile", tol_tile, f"tile error {errs['tile']:.3g} >= {tol_tile:.3g} (worst {th} x {tw} tile {ti}, its worst "
                                       f"entry {w}: {a[w].item():.6g} vs {b[w].item():.6g})"))
    print(f"parity {what}: " + " ".join(f"{k}={v:.3g}" for k, v in errs.items() if v is not None))
    assert errs["norm"] < tol_norm, f"{what}: norm error {errs['norm']:.3g} >= {tol_norm:.3g} ({worst})"
    assert errs["entry"] < tol_entry, f"{what}: entry-wise error {errs['entry']:.3g} >= {tol_entry:.3g} ({worst})"
    for key, tol, msg in msgs:
        assert errs[key] < tol, f"{what}: {msg}"
    return errs


def linear_parity(got, ref, *, tol_norm, tol_entry, tol_row=None, tol_col=None, tile=None, tol_tile=None, what=""):
    """tensor_parity for what one linear launch delivers: C or (C, C2) of an NT launch, dW or (dW, db) of a TN launch.
    got / ref: a tensor or a tuple of them; a bound: one number, or a tuple with one per output.  A vector (db) gets the
    norm and entry checks only.  Returns the list of tensor_parity's results."""
    gots = got if isinstance(got, (tuple, list)) else (got,)
    refs = ref if isinstance(ref, (tuple, list)) else (ref,)
    assert len(gots) == len(refs), (what, len(gots), len(refs))

    def pick(tol, i):
        return tol[i] if isinstance(tol, (tuple, list)) else tol

    out = []
    for i, (g, r) in enumerate(zip(gots, refs)):
        name = f"{what} [{i}]" if len(gots) > 1 else what
        if torch.as_tensor(r).dim() < 2:
            out.append(tensor_parity(g, r, tol_norm=pick(tol_norm, i), tol_entry=pick(tol_entry, i), what=name))
        else:
            out.append(tensor_parity(g, r, tol_norm=pick(tol_norm, i), tol_entry=pick(tol_entry, i), tol_row=pick(tol_row, i),
                                     tol_col=pick(tol_col, i), tile=tile, tol_tile=pick(tol_tile, i), what=name))
    return out


def tie_free_threshold(p0, nominal, span=1.25):
    """A train-mode threshold (reference HWGATE.py:94-100) near `nominal` that no entry of the unmasked softmax `p0`
    (the fp64 oracle's, any shape) comes close to: the geometric centre of the widest relative gap between neighbouring
    values inside [nominal / span, nominal * span].  Returns (thr, margin) with margin = the relative distance from thr
    to the nearest probability.  With it the selector [p0 <= thr] cannot flip under rounding smaller than `margin`, so a
    kernel can be held to its arithmetic tolerance in train mode too."""
    lo, hi = nominal / span, nominal * span
    v = torch.as_tensor(p0, dtype=torch.float64).flatten()
    v = v[(v > lo) & (v < hi)].sort().values
    edges = torch.cat([torch.tensor([lo], dtype=torch.float64), v, torch.tensor([hi], dtype=torch.float64)])
    ratio = edges[1:] / edges[:-1]
    i = int(ratio.argmax())
    return float((edges[i] * edges[i + 1]).sqrt()), float(ratio[i].sqrt() - 1.0)


def oracle_tie_free_thresholds(params, x, nominal, **oracle_kw):
    """One train-mode threshold per block of a whole HWGATE model, near `nominal[block]`, each at the centre of the widest
    gap of that block's own unmasked probabilities (tie_free_threshold) in the fp64 oracle.  Chosen block by block in
    execution order, so that a block sees the activations the earlier choices produce.  `oracle_kw`: OracleHWGAT's
    keywords (num_kps, temporal_dim, depths, num_heads, adj).  Returns (thresholds, smallest margin).
    Why: with ~10^6 probabilities per block a fixed threshold has one within ~10^-6 of it, which is inside what fp32
    rounding (the Fourier embedding's sin / cos of arguments of ~100 rad alone carry ~10^-5) moves a probability by; a
    flipped entry of weight ~0.3 moves a clip's logits by ~10^-3."""
    inner, chosen, margins = O.window_attention, [], []

    def choosing(q, k, v, adj, smask=None, thr=None, attn_keep=None):
        p0 = torch.softmax((q.detach() * q.shape[-1] ** -0.5) @ k.detach().transpose(-2, -1), dim=-1)
        t, _ = tie_free_threshold(p0, thr)
        t = float(np.float32(t))                        # thresholds travel as float32 (fixtures, threshold_override)
        chosen.append(t)
        margins.append(float((p0 / t - 1.0).abs().min()))
        return inner(q, k, v, adj, smask, t, attn_keep)

    O.window_attention = choosing
    try:
        with torch.no_grad():
            oracle = O.OracleHWGAT({k: v.double() for k, v in params.items()}, **oracle_kw)
            oracle.forward(x.double(), thresholds=list(nominal))
    finally:
        O.window_attention = inner
    return chosen, min(margins)


BF16_SELECTOR_BAND = 2.0 ** -6


def oracle_threshold_bracket(run, thresholds, band=BF16_SELECTOR_BAND):
    """Train-mode parity of a WHOLE bf16 model has a discontinuity no threshold can dodge: the selector [P0 <= thr] of
    reference HWGATE.py:94-100 is evaluated on scores formed from bf16 activations (relative error ~2^-8 per layer), so
    a probability within about `band` (relative) of the threshold may fall on either side, and with 10^5..10^7
    probabilities per block some always are that close.  Instead of waiving the assertions, the test BRACKETS the flips:
    `run(thresholds)` -> (logits, {name: grad}) is evaluated by the fp64 oracle at thr, thr * (1 + band) (every entry
    of the band kept) and thr * (1 - band) (every entry of the band dropped).  An implementation whose selector differs
    from the oracle's only inside the band must land within its arithmetic tolerance + the distance the band itself can
    move the result.  Returns (ref_out, ref_grads, width_out, {name: width}) with width = relative L2 distance between
    the two bracket ends; the caller adds 2 x width to its tolerance and asserts that width is small (else the test
    would have no teeth)."""
    ref_out, ref_g = run(list(thresholds))
    hi_out, hi_g = run([t * (1.0 + band) for t in thresholds])
    lo_out, lo_g = run([t * (1.0 - band) for t in thresholds])
    w_out = rel_err(hi_out, lo_out)
    w_g = {k: rel_err(hi_g[k], lo_g[k]) for k in ref_g}
    return ref_out, ref_g, w_out, w_g


def probe_vectors(name, n, k=4):
    """the k fixed +-1 vectors tests/golden/make_fixtures.py::probe_vectors projects a gradient on"""
    import zlib
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    return rs.randint(0, 2, size=(k, n)).astype(np.float64) * 2.0 - 1.0


def grad_digest_check(named_grads, fx, prefix, tol):
    """compare {name: grad} with the `gh.`/`gn.` digests stored in a fixture"""
    worst = 0.0
    n = 0
    for name, g in named_grads.items():
        key = prefix + "gh." + name
        if key not in fx:
            continue
        n += 1
        gd = g.detach().double().flatten().cpu()
        ref_norm, ref_sum = fx[prefix + "gn." + name]
        scale = max(ref_norm, 1e-12)
        e1 = abs(gd.norm().item() - ref_norm) / scale
        e2 = (gd[:48] - torch.from_numpy(fx[key]).double()).norm().item() / \
            max(np.linalg.norm(fx[key]), 1e-3 * scale / max(gd.numel(), 1) ** 0.5, 1e-30)
        worst = max(worst, e1, e2)
        assert e1 < tol, (name, "norm", e1)
        assert e2 < tol * 10, (name, "head", e2)
        pkey = prefix + "gp." + name
        if pkey in fx:          # +-1 projections of the WHOLE gradient: catches misplaced entries anywhere
            proj = probe_vectors(name, gd.numel()) @ gd.numpy()
            e3 = float(np.abs(proj - fx[pkey]).max()) / scale
            worst = max(worst, e3)
            assert e3 < tol * 10, (name, "projection", e3)
    assert n > 0
    return worst


def reference_structure(fx, tag):
    """[(key, shape, dtype, is_parameter, requires_grad)] of a reference `Model` state_dict, in its order, from
    tests/golden/checkpoint_ref.npz (make_fixtures_checkpoint.py)"""
    keys, ndim, dims = fx[tag + ".keys"], fx[tag + ".ndim"], fx[tag + ".dims"]
    grad = dict(zip(fx[tag + ".params"].tolist(), fx[tag + ".requires_grad"].tolist()))
    out, at = [], 0
    for k, n, dt in zip(keys.tolist(), ndim.tolist(), fx[tag + ".dtypes"].tolist()):
        out.append((k, tuple(int(d) for d in dims[at:at + n]), getattr(torch, dt), k in grad, grad.get(k, False)))
        at += n
    return out


def reference_standin(fx, tag, seed=0):
    """an nn.Module with exactly the parameters and buffers of the reference `Model` recorded under `tag` (names,
    order, shapes, dtypes, requires_grad; derived buffers with the reference's values, parameters seeded random):
    what state_dict / load_state_dict / AdamW see of the reference class, without its source"""
    g = torch.Generator().manual_seed(seed)
    root = torch.nn.Module()
    for key, shape, dtype, is_param, requires_grad in reference_structure(fx, tag):
        *path, leaf = key.split(".")
        mod = root
        for part in path:
            if not hasattr(mod, part):
                mod.add_module(part, torch.nn.Module())
            mod = getattr(mod, part)
        if is_param:
            mod.register_parameter(leaf, torch.nn.Parameter((torch.randn(shape, generator=g) * 0.02).to(dtype),
                                                            requires_grad=requires_grad))
        else:
            mod.register_buffer(leaf, torch.from_numpy(np.array(fx[f"{tag}.buf.{key}"])).to(dtype))
    assert list(root.state_dict()) == fx[tag + ".keys"].tolist()
    assert [n for n, _ in root.named_parameters()] == fx[tag + ".params"].tolist()
    return root


def hgate_oracle_from_fixture(fx, dtype=torch.float32):
    """(OracleHGAT, params, cfg) of a tests/golden/hgate_*.npz fixture"""
    from oracle import hgat_oracle as OH
    T, K, C, d0, nc, B, seed = [int(v) for v in fx["cfg"]]
    cfg = dict(kp_dim=C, temporal_dim=T, num_classes=nc, embed_dim=d0, depths=(2, 2, 4), ff_ratio=2.0,
               use_pe=True, num_kps=K, tp=2)
    params = {k: v.to(dtype) for k, v in O.synth_params(seed, weight_std=0.08, **cfg).items()}
    model = OH.OracleHGAT(params, num_kps=K, temporal_dim=T, num_heads=[int(h) for h in fx["heads"]])
    return model, params, cfg


def wgate_oracle_from_fixture(fx, dtype=torch.float32):
    """(OracleWGAT, params, cfg) of a tests/golden/wgate_*.npz fixture"""
    from oracle import wgat_oracle as OW
    T, nW, C, d0, nc, B, heads, depths, seed = [int(v) for v in fx["cfg"]]
    cfg = dict(kp_dim=C, temporal_dim=T, num_classes=nc, embed_dim=d0, depths=depths, ff_ratio=2.0, use_pe=True)
    params = {k: v.to(dtype) for k, v in OW.synth_params(seed, **cfg).items()}
    model = OW.OracleWGAT(params, num_kps=nW * 16, temporal_dim=T, depths=depths, num_heads=heads)
    return model, params, dict(cfg, num_kps=nW * 16, num_heads=heads)
