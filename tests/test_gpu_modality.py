"""Input modalities on the device (csrc/modality.hip, functional.modality, modality.Modality, the models' `input_modality`):
the kernel against its fp32 restatement bit for bit (tests/modality_helpers.py: every entry is a copy or one IEEE
subtraction, so there is no tolerance), every model with a modality set against the same model fed the transformed input,
and the graphed train step with a modality in its forward against the eager step."""
import ctypes
import importlib

import pytest
import torch

import dgcn_helpers as DH
import modality_helpers as MH
import stgcn_helpers as SH
import transformer_helpers as TH
import test_gpu_graph_micro as GM

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
modality = importlib.import_module("sl-hwgat_amd.modality")
train = importlib.import_module("sl-hwgat_amd.train")
optim = importlib.import_module("sl-hwgat_amd.optim")
HF = hw.functional
DEV = torch.device("cuda:0")
EINVAL, ESHAPE = -1, -2

# one thread per entry in workgroups of 256, no grid stride: (2, 5, 7, 3) and up span several workgroups, (1, 1, 1, 2) is
# less than one wave, none is a multiple of 256
SHAPES = [(1, 1, 1, 2), (2, 5, 7, 3), (3, 4, 29, 2), (2, 3, 67, 2)]
TABLES = {"identity": MH.identity, "chain": MH.chain, "star": MH.star}


def _clip(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * 3.0


def _tables(J):
    out = {name: make(J) for name, make in TABLES.items()}
    if J == 29:
        out["tree-29"] = MH.PARENTS_29
    return out


def _check(x, parent, kind, pad_value=None, what=""):
    xd = x.to(DEV)
    keep = xd.clone()
    table = None if parent is None else torch.tensor(parent, dtype=torch.int32, device=DEV)
    got = HF.modality(xd, table, kind, pad_value)
    assert torch.equal(xd, keep), ("the input was written", what)
    assert got.data_ptr() != xd.data_ptr() and got.dtype == torch.float32 and got.shape == x.shape
    ref = MH.restate(x, parent, kind, pad_value)
    assert torch.equal(got.cpu(), ref), (what, kind, (got.cpu() != ref).nonzero()[:4].tolist())
    return got


# ------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_restatement_bit_for_bit(shape):
    x = _clip(shape, seed=sum(shape))
    for name, parent in _tables(shape[2]).items():
        for kind in MH.KINDS:
            got = _check(x, parent, kind, what=name)
            assert torch.equal(got, HF.modality(x.to(DEV), torch.tensor(parent, dtype=torch.int32, device=DEV),
                                                MH.KINDS.index(kind)))                 # the code is the name's position
    for kind in ("joint", "motion"):                          # these two read no table
        _check(x, None, kind)
    if shape[1] == 1:                                         # one frame has no successor
        for kind in ("motion", "bone_motion"):
            assert not _check(x, MH.chain(shape[2]), kind).any()


def test_roots_give_positive_zero_and_motion_ends_on_zero():
    x = _clip((2, 4, 7, 3), seed=1)
    x[0, 1, 0, 0] = float("inf")                              # a root holding inf: inf - inf would be NaN
    xd = x.to(DEV)
    table = torch.tensor(MH.chain(7), dtype=torch.int32, device=DEV)
    bone = HF.modality(xd, table, "bone")
    assert torch.equal(bone[:, :, 0].view(torch.int32), torch.zeros(2, 4, 3, dtype=torch.int32, device=DEV))
    for kind in ("motion", "bone_motion"):
        assert not HF.modality(xd, table, kind)[:, -1].any()
    ident = torch.tensor(MH.identity(7), dtype=torch.int32, device=DEV)
    assert not HF.modality(xd, ident, "bone").any() and not HF.modality(xd, ident, "bone_motion").any()


PADDINGS = {"trailing": lambda x: x[:, -2:], "middle": lambda x: x[:, 2:3], "first": lambda x: x[:, :1], "all": lambda x: x}


@pytest.mark.parametrize("where", list(PADDINGS))
def test_padded_frames_pass_through_and_end_the_motion(where):
    x = _clip((3, 6, 29, 2), seed=2)
    PADDINGS[where](x[:2])[...] = -1.0                        # clips 0 and 1 padded, clip 2 not
    x[2, 3, 5, 1] = -1.0                                      # a -1 that is not a frame's first word marks nothing
    pad = x[:, :, 0, 0] == -1.0
    assert pad[:2].any() and not pad[2].any()
    for kind in MH.KINDS:
        got = _check(x, MH.PARENTS_29, kind, pad_value=-1.0, what=where).cpu()
        assert torch.equal(got[pad], x[pad])                  # marker and all
        if kind in ("motion", "bone_motion"):
            before = torch.zeros_like(pad)
            before[:, :-1] = pad[:, 1:]
            assert not got[before & ~pad].any()
    # a frame whose first word is the marker by accident IS padding: the Transformer's rule, word for word
    y = _clip((1, 4, 5, 2), seed=3)
    y[0, 1, 0, 0] = -1.0
    got = _check(y, MH.chain(5), "bone", pad_value=-1.0).cpu()
    assert torch.equal(got[0, 1], y[0, 1])


def test_without_padding_the_marker_is_data():
    x = _clip((2, 5, 7, 3), seed=4)
    x[0, 2:] = -1.0
    x[1, 0] = -1.0
    for kind in MH.KINDS:
        _check(x, MH.star(7), kind, pad_value=None)
    assert not torch.equal(HF.modality(x.to(DEV), None, "motion").cpu(), MH.restate(x, None, "motion", -1.0))


def test_wrapper_refusals_on_the_device():
    x = _clip((2, 3, 5, 2)).to(DEV)
    table = torch.tensor(MH.chain(5), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.modality(x.cpu(), table, "bone")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.modality(x, table.cpu(), "bone")
    with pytest.raises(TypeError, match="fp32"):
        HF.modality(x.bfloat16(), table, "bone")
    with pytest.raises(ValueError, match="contiguous"):
        HF.modality(x.transpose(1, 2), table, "motion")
    with pytest.raises(ValueError, match="alias"):
        HF.modality(x, table, "bone", out=x)
    with pytest.raises(ValueError, match="alias"):
        HF.modality(x[:1], table, "bone", out=x.view(-1)[4:34].view(1, 3, 5, 2))
    out = torch.empty_like(x)
    assert HF.modality(x, table, "bone", out=out) is out and torch.equal(out, HF.modality(x, table, "bone"))


def test_return_codes():
    fn = hw._lib.lib().hwgat_modality
    x = _clip((1, 2, 3, 2)).to(DEV)
    out = torch.empty_like(x)
    table = torch.tensor(MH.chain(3), dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    assert fn(None, p(table), p(out), 1, 2, 3, 2, 1, 0, 0.0, st) == EINVAL
    assert fn(p(x), p(table), None, 1, 2, 3, 2, 1, 0, 0.0, st) == EINVAL
    assert fn(p(x), p(table), p(out), 1, 0, 3, 2, 1, 0, 0.0, st) == EINVAL
    assert fn(p(x), p(table), p(out), 1, 2, 3, 2, 4, 0, 0.0, st) == ESHAPE
    assert fn(p(x), p(table), p(out), 1, 2, 3, 2, -1, 0, 0.0, st) == ESHAPE
    assert fn(p(x), None, p(out), 1, 2, 3, 2, 1, 0, 0.0, st) == EINVAL
    assert fn(p(x), None, p(out), 1, 2, 3, 2, 3, 0, 0.0, st) == EINVAL
    assert fn(p(x), None, p(out), 1, 2, 3, 2, 2, 0, 0.0, st) == 0          # motion reads no table
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), MH.restate(x.cpu(), None, "motion"))


# ------------------------------------------------------------------------------------------ 2. the models
def _family(kind):
    ds = {"src_len": 16, "num_class": 7}
    torch.manual_seed(11)
    if kind == "gate":
        hp = hw.GATEParams(ds, 2, DEV)
        hp.depths = 3
        return hw.GATEModel(*hp.get_model_params()).to(DEV)
    return GM._build(torch.float32, kind)


def _baseline(kind):
    torch.manual_seed(11)
    if kind == "stgcn":
        return hw.STGCNModel(*SH.model_args(SH.CONFIGS["b"])).to(DEV), SH.make_input(SH.CONFIGS["b"])[0]
    if kind == "dgcn":
        return hw.DecoupledGCNModel(*DH.model_args(DH.CONFIGS["b"])).to(DEV), DH.make_input(DH.CONFIGS["b"])[0]
    cfg = TH.CONFIGS["c"]
    m = hw.TransformerModel(*TH.model_args(cfg))
    m.load_state_dict(TH.recipe_weights(m.state_dict(), cfg["seed"]), strict=False)
    g = torch.Generator().manual_seed(7)
    return m.to(DEV), torch.rand(cfg["B"], cfg["T"], cfg["K"], cfg["C"], generator=g)


def _model_and_input(kind):
    if kind in ("stgcn", "dgcn", "transformer"):
        model, x = _baseline(kind)
        return model.eval(), x.to(DEV)
    model = _family(kind).eval()
    g = torch.Generator(device=DEV).manual_seed(3)
    return model, torch.rand(2, model.temporal_dim, model.num_kps, model.kp_dim, device=DEV, generator=g)


def _set_equals_fed(model, x, m, pad_value=None):
    """model with the modality set on x == model without one on m(x), bit for bit; x and the state_dict keys stay"""
    keep, keys = x.clone(), list(model.state_dict())
    with torch.no_grad():
        plain = model(x)
        model.set_input_modality(m)
        assert list(model.state_dict()) == keys
        a = model(x)
        assert torch.equal(x, keep)
        model.set_input_modality(None)
        fed = HF.modality(x, None if m.table is None else m.table.to(DEV), m.kind,
                          m.pad_value if m.pad_value is not None else pad_value)
        b = model(fed)
        assert torch.equal(model(x), plain)                   # None: the model is what it was
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert not torch.equal(a, plain)                          # and the modality is not a no-op
    return a


@pytest.mark.parametrize("kind", ["hwgate", "hgate", "wgate", "gate", "transformer", "stgcn", "dgcn"])
def test_model_with_a_modality_equals_the_model_fed_the_view(kind):
    model, x = _model_and_input(kind)
    J = x.shape[2]
    for m in (modality.Modality("bone_motion", MH.PARENTS_29 if J == 29 else MH.chain(J)), modality.Modality("motion")):
        _set_equals_fed(model, x, m, pad_value=getattr(model, "pad_index", None) if kind == "transformer" else None)


def test_hwgate_with_a_part_table_takes_parents_of_the_raw_joints():
    torch.manual_seed(11)
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 7}, 2, DEV, num_kps=64)
    model = hw.Model(*hp.get_model_params()).to(DEV).use_part_table(hw.part_table(29)).eval()
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.rand(2, 16, 29, 2, device=DEV, generator=g)
    _set_equals_fed(model, x, modality.Modality("bone", MH.PARENTS_29))
    _set_equals_fed(model, x, modality.Modality("bone_motion", MH.PARENTS_29))
    model.set_input_modality(modality.Modality("bone", MH.chain(64)))      # a table over the slots is not one over the joints
    with pytest.raises(ValueError, match="64 joints"), torch.no_grad():
        model(x)


def test_transformer_keeps_padded_frames_masked_under_a_modality():
    """The marker of every padded frame survives the view, so the key-padding words are what they are without a modality,
    and nothing of a padded frame reaches a real one: with other values behind the marker the view's real frames keep their
    bits.  (The logits themselves do move with those values, with or without a modality: the reference pools over ALL
    frames, padded ones included -- tests/transformer_helpers.restate -- and a padded frame is still a query.  The
    statement that holds is the one on the view and on the padding words.)"""
    cfg = TH.CONFIGS["c"]                                     # pool 'max': the padded frames' values would show
    model, _ = _baseline("transformer")
    model.eval()
    x, _ = TH.make_input(cfg)                                 # clip 0 tail-padded, clip 1 scattered padded frames
    x = x.to(DEV)
    pad = x[:, :, 0, 0] == -1.0
    assert pad[0].any() and pad[1].any() and not pad[2].any()
    m = modality.Modality("bone_motion", MH.PARENTS_29)
    a = _set_equals_fed(model, x, m, pad_value=-1.0)
    other = x.clone()
    junk = torch.rand(other[pad].shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)) * 50.0
    junk[:, 0, 0] = -1.0                                      # other values behind the pad marker
    other[pad] = junk
    table = m.table.to(DEV)
    for kind in MH.KINDS:
        va, vb = HF.modality(x, table, kind, -1.0), HF.modality(other, table, kind, -1.0)
        assert torch.equal(va[~pad], vb[~pad]), kind          # no real frame reads a padded one
        assert torch.equal(va[pad], x[pad]) and torch.equal(vb[pad], other[pad])
        assert torch.equal(va[:, :, 0, 0] == -1.0, pad) and torch.equal(vb[:, :, 0, 0] == -1.0, pad)
    # the padding words the attention masks with: the model's own embedding of the view against that of the raw clip
    with torch.no_grad():
        words = model._embed(x.reshape(x.shape[0], x.shape[1], -1))[1]
        for clip in (x, other):
            view = HF.modality(clip, table, "bone_motion", -1.0)
            assert torch.equal(model._embed(view.reshape(x.shape[0], x.shape[1], -1))[1], words)
    model.set_input_modality(m)
    with torch.no_grad():
        b = model(other)
        assert torch.equal(b[2], a[2])                        # the clip without padding is untouched
        with pytest.raises(ValueError, match=r"\(B, T, K, C\)"):
            model(x.reshape(x.shape[0], x.shape[1], -1))
    # a modality that names its own marker: the same marker, the same logits
    model.set_input_modality(modality.Modality("bone_motion", MH.PARENTS_29, pad_value=-1.0))
    with torch.no_grad():
        assert torch.equal(model(x), a)
    # without the marker the motion kinds would difference real frames against padding: the pad_value is what prevents it
    blind = HF.modality(x, table, "bone_motion", None)
    assert not torch.equal(blind[~pad], HF.modality(x, table, "bone_motion", -1.0)[~pad])


# ------------------------------------------------------------------------------------------ 3. the graphed train step
def test_graphed_train_step_with_bone_motion_equals_the_eager_step():
    """tests/test_gpu_graph.py's deterministic comparison (bit equality of every loss and weight) with a modality in the
    forward: the launch is a node of the graph, and the step's static batch keeps what was copied in"""
    steps, runs = 3, []
    for graphed in (False, True):
        m = GM._build(torch.float32, "hwgate")
        m.set_input_modality(modality.Modality("bone_motion", MH.chain(m.num_kps)))
        x, y = GM._batch(m)
        o = optim.DeviceAdamW(list(m.parameters()), lr=5e-4)
        torch.manual_seed(11)
        s = train.GraphedTrainStep(m, o, x, y) if graphed else train.TrainStep(m, o, None)
        losses = [s(x, y).clone() for _ in range(steps)]
        if graphed:
            assert torch.equal(s.x, x)                        # the forward left the static batch alone
        runs.append((losses, {n: p.detach().clone() for n, p in m.named_parameters()}))
    (le, we), (lg, wg) = runs
    for k in range(steps):
        assert torch.equal(le[k], lg[k]), (k, float(le[k]), float(lg[k]))
    for n in we:
        assert torch.equal(we[n], wg[n]), n
    # and the step is not the plain one
    plain = GM._build(torch.float32, "hwgate")
    torch.manual_seed(11)
    first = train.TrainStep(plain, optim.DeviceAdamW(list(plain.parameters()), lr=5e-4), None)(*GM._batch(plain))
    assert not torch.equal(first, le[0])


# ------------------------------------------------------------------------------------------ 4. the epoch loop
def test_epoch_loop_carries_the_modality_and_resume_refuses_another(tmp_path):
    cfg = SH.CONFIGS["a"]
    g = torch.Generator().manual_seed(21)
    x = torch.rand(8, cfg["T"], cfg["V"], cfg["C"], generator=g).to(DEV)
    y = torch.randint(0, cfg["nclass"], (8,), generator=g).to(DEV)
    tr = [(x[:4], y[:4]), (x[4:], y[4:])]
    kw = dict(batch_size=4, example=(x[:4], y[:4]), num_classes=cfg["nclass"], save_interval=1)
    m = modality.Modality("bone_motion", MH.PARENTS_29)

    def build(seed, view):
        torch.manual_seed(seed)
        model = hw.STGCNModel(*SH.model_args(cfg, 0.0)).to(DEV).set_input_modality(view)
        model.deterministic_train = True
        return model, optim.DeviceAdamW(list(model.parameters()), lr=1e-3)

    model, opt = build(3, m)
    first = train.EpochLoop(model, opt, None, out_prefix=str(tmp_path / "bm"), **kw)
    first.run(tr, tr, epochs=0)
    path = str(tmp_path / "bm_best_loss.pt")
    assert path in first.written
    raw = torch.load(path, map_location="cpu", weights_only=True)       # plain values: the safe loader takes them
    assert raw["extra"]["modality"] == m.state()
    assert not any("modality" in k for k in raw["model_state_dict"])

    model, opt = build(4, modality.Modality.from_state(raw["extra"]["modality"]))
    second = train.EpochLoop(model, opt, None, **kw)
    assert second.resume(path) == 1
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), first.model.state_dict().values()))
    second.train_epoch(tr[:1])

    for view in (None, modality.Modality("bone", MH.PARENTS_29)):
        model, opt = build(5, view)
        before = [p.detach().clone() for p in model.parameters()]
        with pytest.raises(ValueError, match="input modality"):
            train.EpochLoop(model, opt, None, **kw).resume(path)
        assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))       # refused before anything was loaded

    model, opt = build(3, None)
    plain = train.EpochLoop(model, opt, None, out_prefix=str(tmp_path / "plain"), **kw)
    plain.run(tr, tr, epochs=0)
    raw = torch.load(str(tmp_path / "plain_best_loss.pt"), map_location="cpu", weights_only=True)
    assert "modality" not in raw["extra"]
    model, opt = build(6, m)
    with pytest.raises(ValueError, match="input modality"):              # a missing entry means None
        train.EpochLoop(model, opt, None, **kw).resume(str(tmp_path / "plain_best_loss.pt"))
