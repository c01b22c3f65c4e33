"""GPU: explain.AttentionTap on whole models -- the exported maps against what a forward hook on the reference's
`attn.softmax` recorded (tests/golden/attn_maps_hwgate.npz) and against the pinned oracles' `prob` tensors, and the
properties of the tap itself: it changes no logit and no train step, it works with bf16 activations, and a graph captured
while it is armed replays its launches."""
import importlib
import os
import sys

import pytest
import torch

import gate_helpers as GH
from helpers import load_fixture, rel_err, entrywise, hgate_oracle_from_fixture
from oracle import hwgat_oracle as O
from oracle import wgat_oracle as WO

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_fixtures_window import edge_list  # noqa: E402

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
EX = hw.explain
serve = importlib.import_module("sl-hwgat_amd.serve")
train = importlib.import_module("sl-hwgat_amd.train")
DEV = "cuda:0"
# Largest absolute error of an exported probability (entries are <= 1) / of `received` relative to its largest entry, now
# with the model's fp32 activation chain in front of the attention: about 3x the worst value observed on an MI355X (in the
# comments), capped at 2e-5 (DESIGN section 7's fp32 attention contract).  On the same qkv the kernel itself is at 4e-7
# (tests/test_gpu_attn_probs.py); the rest is what the fp32 LayerNorm / linear chain in front of it contributes.
FP32_CAP, BF16_CAP = 2e-5, 1e-2
HWGATE_P = 1.5e-6       # observed 5.1e-7 (block 3 against the reference's hooked tensor)
HGATE_P = FP32_CAP      # observed 1.4e-5 (hgate_a, block 5 of 8, d = 512, against OracleHGAT in fp64): 3x is past the cap
BAND_R = 4e-6           # observed 1.3e-6 (WGATE) / 9.2e-7 (GATE)
BF16_MAP = BF16_CAP     # observed 1.3e-3 (clip_relevance, bf16 against fp32 activations): the cap is the stated bound
assert max(HWGATE_P, HGATE_P, BAND_R) <= FP32_CAP


def _hwgate_attn_fixture(dtype=torch.float32):
    fx = load_fixture("attn_maps_hwgate.npz")
    T, K, C, d0, nc, B, seed = [int(v) for v in fx["cfg"]]
    depths, heads = [int(v) for v in fx["depths"]], [int(v) for v in fx["heads"]]
    hp = hw.HWGATEParams({"src_len": T, "num_class": nc}, C, None, num_kps=K, embed_dim=d0)
    hp.depths, hp.num_heads, hp.drop_rate = depths, heads, 0.0
    assert torch.equal(hp.adj_mat, torch.from_numpy(fx["adj"]))
    model = hw.Model(*hp.get_model_params())
    cfg = dict(kp_dim=C, temporal_dim=T, num_classes=nc, embed_dim=d0, depths=tuple(depths), ff_ratio=hp.ff_ratio,
               use_pe=True, num_kps=K, tp=2)
    res = model.load_state_dict(O.synth_params(seed, weight_std=0.08, **cfg), strict=False)
    assert not res.unexpected_keys and all(k.endswith("attn_mask") for k in res.missing_keys)
    return fx, model.to(DEV).set_activation_dtype(dtype).eval()


def test_hwgate_probs_match_the_reference_hook():
    fx, model = _hwgate_attn_fixture()
    x = torch.from_numpy(fx["x"]).to(DEV)
    tap = EX.AttentionTap(model, probs=True)
    with tap, torch.no_grad():
        logits = model(x)
    assert rel_err(logits.cpu(), fx["eval.logits"]) < 1e-4
    assert sorted(tap.probs) == sorted(tap.received) == [0, 1, 2, 3]
    for k in range(4):
        ref = torch.from_numpy(fx[f"prob{k}"]).double()                 # (B f nW, nH, 32, 32), the reference's own tensor
        got = tap.probs[k].cpu().double()
        assert got.shape[:3] == (x.shape[0], ref.shape[0] // (2 * x.shape[0]), 2) and got.shape[3:] == ref.shape[1:]
        err = float((got.reshape(ref.shape) - ref).abs().max())
        print(f"explain hwgate block {k}: P against the reference hook {err:.2e}")
        assert err < HWGATE_P, (k, err)
        frames = got.shape[1] * 2
        assert tuple(tap.received[k].shape) == (x.shape[0], frames, 32)
        assert abs(float(tap.received[k].double().sum()) - x.shape[0] * frames * 32) < FP32_CAP * x.shape[0] * frames * 32


def test_hgate_probs_match_the_oracle():
    fx = load_fixture("hgate_a.npz")
    oracle, params, cfg = hgate_oracle_from_fixture(fx, torch.float64)
    hp = hw.HGATEParams({"src_len": cfg["temporal_dim"], "num_class": cfg["num_classes"]}, cfg["kp_dim"], DEV,
                        embed_dim=cfg["embed_dim"])
    hp.num_heads, hp.drop_rate = [int(h) for h in fx["heads"]], 0.0
    model = hw.HGATEModel(*hp.get_model_params())
    model.load_state_dict({k: v.float() for k, v in params.items()}, strict=False)
    model.eval()
    x = torch.from_numpy(fx["x"])
    oracle.forward(x.double(), tap=True)
    tap = EX.AttentionTap(model, probs=True, received=False)
    with tap, torch.no_grad():
        logits = model(x.to(DEV))
    assert rel_err(logits.cpu(), fx["eval.logits"]) < 1e-4
    assert not tap.received and len(tap.probs) == len(model.block_list())
    for k, got in tap.probs.items():
        ref = oracle.taps[f"prob{k}"]                                    # (B, f, nH, 2K, 2K)
        assert tuple(got.shape) == (ref.shape[0], ref.shape[1], 1) + tuple(ref.shape[2:])
        err = float((got.cpu().double()[:, :, 0] - ref).abs().max())
        print(f"explain hgate block {k}: P against OracleHGAT {err:.2e}")
        assert err < HGATE_P, (k, err)


def _received_of_dense(prob, F, W):
    """(B, nW, nH, F W, F W) dense probabilities -> (B, F, K) head-mean column sums"""
    Bb, nW = prob.shape[:2]
    return prob.sum(-2).mean(2).view(Bb, nW, F, W).permute(0, 2, 1, 3).reshape(Bb, F, nW * W)


def test_wgate_received_matches_the_oracle_blocks():
    T, C, nc, Bb, depths, heads, K = 8, 2, 5, 2, 2, 8, 32
    cfg = dict(kp_dim=C, temporal_dim=T, num_classes=nc, embed_dim=128, depths=depths, ff_ratio=2.0, use_pe=True)
    params = WO.synth_params(61, **cfg)
    oracle = WO.OracleWGAT({k: v.double() for k, v in params.items()}, num_kps=K, temporal_dim=T, depths=depths,
                           num_heads=heads)
    hp = hw.WGATEParams({"src_len": T, "num_class": nc}, C, DEV, num_kps=K, embed_dim=128)
    hp.num_heads, hp.depths, hp.drop_rate = heads, depths, 0.0
    model = hw.WGATEModel(*hp.get_model_params())
    model.load_state_dict(params, strict=False)
    model.eval()
    assert model._attn_kind == "band"
    x = torch.rand(Bb, T, K, C, generator=torch.Generator().manual_seed(62))
    h = O.fourier_embed(x.double(), oracle.p["B"]) + oracle.p["pos_encoder.pe"][:, :T]
    tap = EX.AttentionTap(model)
    with tap, torch.no_grad():
        model(x.to(DEV))
    for k in range(depths):
        h, prob = oracle.block(h, k)
        err = entrywise(tap.received[k].cpu(), _received_of_dense(prob, T, 16))
        print(f"explain wgate block {k}: received against the oracle block {err:.2e}")
        assert err < BAND_R, (k, err)
    rel = tap.clip_relevance()
    assert tuple(rel.shape) == (Bb, T, K) and float((rel.sum((1, 2)) - 1).abs().max()) < 1e-5


def test_gate_received_matches_the_dense_restatement():
    T, C, nc, Bb, depths, heads, K = 8, 2, 6, 2, 2, 8, 29
    cfg = dict(kp_dim=C, temporal_dim=T, num_kps=K, num_classes=nc, embed_dim=128, depths=depths, ff_ratio=2.0,
               use_pe=True, pool="weighted")
    params = GH.synth_params(63, **cfg)
    hp = hw.GATEParams({"src_len": T, "num_class": nc}, C, DEV)
    hp.depths, hp.num_heads, hp.drop_rate = depths, heads, 0.0
    model = hw.GATEModel(*hp.get_model_params())
    model.load_state_dict(params, strict=False)
    model.eval()
    assert model._attn_kind == "wband"
    P = {k: v.double() for k, v in params.items()}
    adj = hp.adj_mat.cpu().double()
    x = torch.rand(Bb, T, K, C, generator=torch.Generator().manual_seed(64))
    tap = EX.AttentionTap(model)
    with tap, torch.no_grad():
        model(x.to(DEV))
    h = O.fourier_embed(x.double(), P["B"]) + P["pos_encoder.pe"][:, :T]
    for k in range(depths):                                               # gate_helpers.DenseBandModel.block, keeping P
        pre = f"layers.{k}."
        xn = O.layer_norm(h, P[pre + "norm1.weight"], P[pre + "norm1.bias"])
        qkv = xn @ P[pre + "attn.qkv.weight"].t() + P[pre + "attn.qkv.bias"]
        o, prob = GH.dense_band_attention(qkv, adj, heads, K, return_probs=True)
        y = h + (o @ P[pre + "attn.proj.weight"].t() + P[pre + "attn.proj.bias"])
        z = O.gelu(O.layer_norm(y, P[pre + "norm2.weight"], P[pre + "norm2.bias"]) @ P[pre + "ff.fc1.weight"].t()
                   + P[pre + "ff.fc1.bias"])
        h = y + (z @ P[pre + "ff.fc2.weight"].t() + P[pre + "ff.fc2.bias"])
        err = entrywise(tap.received[k].cpu(), _received_of_dense(prob, T, K))
        print(f"explain gate block {k}: received against the dense restatement {err:.2e}")
        assert err < BAND_R, (k, err)


def _hwgate_w8():
    fx = load_fixture("window_w8.npz")
    T, K, C, d0, nc, Bb, seed, W = [int(v) for v in fx["cfg"]]
    hp = hw.HWGATEParams({"src_len": T, "num_class": nc}, C, None, num_kps=K)
    hp.window_size, hp.num_heads, hp.drop_rate = W, [int(h) for h in fx["heads"]], 0.0
    hp.edges = [edge_list(W, w) for w in range(K // W)]
    hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
    model = hw.Model(*hp.get_model_params())
    cfg = dict(kp_dim=C, temporal_dim=T, num_classes=nc, embed_dim=d0, depths=tuple(hp.depths), ff_ratio=hp.ff_ratio,
               use_pe=hp.pe, num_kps=K, tp=2)
    model.load_state_dict(O.synth_params(seed, weight_std=0.08, **cfg), strict=False)
    return fx, model.to(DEV)


def test_hwgate_w8_received_sums_and_the_tap_changes_nothing():
    fx, model = _hwgate_w8()
    assert model._attn_kind == "pwin"
    x = torch.from_numpy(fx["x"]).to(DEV)
    y = torch.from_numpy(fx["y"]).to(DEV)
    crit = train.SmoothedCrossEntropyLoss()

    def train_step():
        model.train()
        model.deterministic_train = True
        model.threshold_override = [float(t) for t in fx["train.thr"]]
        model.zero_grad()
        loss = crit(model(x), y)
        loss.backward()
        return loss.detach().clone(), model.head.weight.grad.clone()

    loss0, grad0 = train_step()
    model.eval()
    with torch.no_grad():
        outside = model(x)
    tap = EX.AttentionTap(model)
    with tap, torch.no_grad():
        inside = model(x)
    assert torch.equal(inside, outside)
    assert model.attention_tap is None and not tap.probs
    Bb, T, K = x.shape[:3]
    stage_frames = [T, T, T // 2, T // 2] + [T // 4] * 4
    for k, r in tap.received.items():
        assert tuple(r.shape) == (Bb, stage_frames[k], K)
        assert abs(float(r.double().sum()) - Bb * stage_frames[k] * K) < FP32_CAP * Bb * stage_frames[k] * K, k
    rel = tap.clip_relevance()
    assert tuple(rel.shape) == (Bb, T, K) and float((rel.sum((1, 2)) - 1).abs().max()) < 1e-5
    with torch.no_grad():
        assert torch.equal(model(x), outside)                           # and after leaving the `with`
    loss1, grad1 = train_step()
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    with pytest.raises(RuntimeError, match="eval"):                     # still in train(): arming raises
        with tap:
            pass


def test_part_table_folds_slots_onto_joints():
    _, model = _hwgate_w8()
    model.use_part_table(hw.part_table(29)).eval()
    x = torch.rand(2, 16, 29, 2, generator=torch.Generator().manual_seed(7)).to(DEV)
    tap = EX.AttentionTap(model, blocks=[0, 7])
    with tap, torch.no_grad():
        model(x)
    assert sorted(tap.received) == [0, 7]
    rel = tap.clip_relevance()
    slots = EX.fold_relevance(tap.received, 16)
    index = model.part_index.long()
    J = int(index.max()) + 1
    assert tuple(rel.shape) == (2, 16, J) and tuple(slots.shape) == (2, 16, 64) and J <= 29
    want = torch.zeros(2, 16, J, device=DEV).index_add_(2, index, slots)
    assert torch.allclose(rel, want / want.sum((1, 2), keepdim=True), rtol=1e-5, atol=0)   # the same fold, normalised after
    assert float((rel.sum((1, 2)) - 1).abs().max()) < 1e-5


def test_bf16_activations_give_the_same_map():
    fx, m32 = _hwgate_attn_fixture()
    _, m16 = _hwgate_attn_fixture(torch.bfloat16)
    x = torch.from_numpy(fx["x"]).to(DEV)
    maps = []
    for model in (m32, m16):
        tap = EX.AttentionTap(model)
        with tap, torch.no_grad():
            model(x)
        assert all(r.dtype == torch.float32 for r in tap.received.values())
        maps.append(tap.clip_relevance().cpu())
    err = entrywise(maps[1], maps[0])
    print(f"explain bf16 activations: clip_relevance against the fp32 run {err:.2e}")
    assert err < BF16_MAP, err


def test_graph_captured_inside_the_tap_replays_it():
    fx, model = _hwgate_attn_fixture()
    x = torch.from_numpy(fx["x"]).to(DEV)
    x2 = torch.rand(x.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    tap = EX.AttentionTap(model, probs=True)
    with tap:
        fast = serve.GraphedEval(model, x)
        held = {k: r.data_ptr() for k, r in tap.received.items()}
        logits = fast(x2)
        graphed_r = {k: r.clone() for k, r in tap.received.items()}
        graphed_p = {k: p.clone() for k, p in tap.probs.items()}
        assert {k: r.data_ptr() for k, r in tap.received.items()} == held      # static buffers, reused
    eager = EX.AttentionTap(model, probs=True)
    with eager, torch.no_grad():
        want = model(x2)
    assert torch.equal(logits, want)
    assert sorted(graphed_r) == [0, 1, 2, 3]
    for k in graphed_r:
        assert torch.equal(graphed_r[k], eager.received[k]) and torch.equal(graphed_p[k], eager.probs[k]), k
