"""The device-resident dropout seed of a model (shared by the graph-attention family, models/_family.py, and the baselines).

Every seeded kernel hashes with  site seed + the call's base seed, which it reads on the device when it runs
(include/hwgat_hip.h, "dropout seeds") from the per-call copy of `_seed_state[1]` that `_next_step_seed` takes, so a train
step captured in a HIP graph (train.GraphedTrainStep) replays with fresh masks and a backward regenerates its own
forward's masks whatever train forwards ran in between.  A model class mixes DeviceSeeds in front of nn.Module and calls
`_init_device_seeds()` in its constructor -- the only place these fields are assigned, there are no class-level
fallbacks; train.TrainStep, train.GraphedTrainStep and serve.GraphedEval use `_seed_state`, `_drop_calls`, `_seeds` and
`device_seed_counter`.
"""
import torch
from torch import nn

from . import functional as HF
from .modality import Modality


class DeviceSeeds:
    def _init_device_seeds(self, clips_independent_in_train=True):
        self._drop_calls = 0
        # False: the train() forward couples the clips of a batch (batch statistics), so a batch must not be zero-padded
        # (train.GraphedTrainStep(ragged=True), train.TrainStep(pad_to=...)); eval() never couples them
        self.clips_independent_in_train = bool(clips_independent_in_train)
        # the dropout seed lives on the DEVICE: {step counter, base seed of the step, initial seed, rank salt}; every
        # seeded kernel adds word 1 to its (host, per-site) seed when it runs, see include/hwgat_hip.h "dropout seeds"
        self.register_buffer("_seed_state", torch.zeros(4, dtype=torch.int32), persistent=False)
        self.device_seed_counter = False                          # True: a captured train step advances the counter itself
        self._call_base = None                                    # the latest train forward's copy of the base seed
        self.deterministic_eval = True                            # eval(): fixed-order sums, bit-reproducible logits
        self.deterministic_train = False                          # train(): the same for the whole step (slower: no float atomics anywhere)
        self.hip_head = False                                     # True: the classifier nn.Linear runs on csrc/head.hip (_classify)
        self.input_modality = None                                # modality.Modality the forward reads its input through (set_input_modality)

    def _site_seeds(self, k):
        """four dropout-SITE seeds of block k (host integers that never change): proj, fc1, fc2 outputs
        (HWGATE.py:116,133,135) and the attention probabilities (HWGATE.py:112).  A kernel hashes with
        site seed + the base seed of the step, which it reads from `_seed_state[1]` on the device."""
        return [((k * 4 + s) * HF.SEED_SITE) & 0xFFFFFFFF for s in range(4)]

    def _seeds(self, k):
        """the four EFFECTIVE seeds of block k for the step whose counter is `_drop_calls` (host mirror of the device
        word: site seed + base; what hwgat_dropout_mask_f32 needs to reproduce a mask in a test)"""
        # rank_salt: data-parallel ranks share torch's seed (identical initial weights) but must not share
        # dropout masks; dist.broadcast_parameters() sets it to the rank
        base = HF.seed_base_value(torch.initial_seed(), self._drop_calls, getattr(self, "rank_salt", 0))
        return [(base + s) & 0xFFFFFFFF for s in self._site_seeds(k)]

    def _seed_base(self):
        """the 1-element device view of the base seed NOW (the latest train forward's); a forward hands its kernels the
        per-call copy `_next_step_seed` returns instead"""
        return self._seed_state[1:2]

    def _next_step_seed(self):
        """once per train-mode forward; returns the base-seed word of THIS call.  Eager: the four state words are rewritten
        from host integers (kernel arguments -- no copy, no sync).  `device_seed_counter` (a captured train step,
        train.GraphedTrainStep): the device increments its own counter, so a graph replay draws fresh masks.  Either way
        the host counter `_drop_calls` goes up with the device one (its mirror, what `_seeds()` reads).

        Per-call rule: every kernel of one forward -- and of its backward, which regenerates the masks instead of storing
        them -- reads the base seed from `_call_base`, a device copy of word 1 taken here (one 4-byte copy, ordered on the
        stream; inside a capture a graph node that every replay refreshes).  `_seed_state[1]` itself is rewritten by the
        next train forward, so a backward that read it would draw that later call's masks when two forwards run before
        their backwards (`loss(model(a)) + loss(model(b))`)."""
        if self.device_seed_counter:
            HF.seed_advance(self._seed_state)
        else:
            HF.seed_set(self._seed_state, self._drop_calls + 1, torch.initial_seed(), getattr(self, "rank_salt", 0))
        self._drop_calls += 1
        self._call_base = self._seed_state[1:2].clone()
        return self._call_base

    def _deterministic(self):
        """bit-reproducible arithmetic for this call: eval() by default (`deterministic_eval`); train() on request
        (`deterministic_train = True`: fixed-order row statistics, pooled sum and parameter gradients -- the reference's
        single-device training repeats itself bit for bit with fixed seeds, this is the mode that does the same)"""
        return bool(self.deterministic_train if self.training else self.deterministic_eval)

    def set_input_modality(self, modality):
        """read the input through `modality` (modality.Modality: bones, motion, bone motion) from the next forward on, or as
        it comes with None (the default: no launch is added and every bit is what it was).  The view is one launch in
        front of the model's first kernel and writes a tensor of its own; the caller's input is left alone.  The parent
        table is a non-persistent buffer (`_modality_parents`, registered here): `state_dict()` keeps its keys and
        `.to(device)` moves it"""
        if modality is not None and not isinstance(modality, Modality):
            raise ValueError(f"set_input_modality takes a modality.Modality or None, got {type(modality).__name__}")
        table = None if modality is None or modality.table is None else modality.table.to(self._seed_state.device)
        self.input_modality = modality
        self.register_buffer("_modality_parents", table, persistent=False)
        return self

    def _input_view(self, x, pad_value=None):
        """the model's input site: x (B, T, J, C) fp32 contiguous as the caller gave it -> what the first kernel reads"""
        m = getattr(self, "input_modality", None)                 # a model unpickled from before the field existed has none
        return x if m is None else m.apply(x, self._buffers.get("_modality_parents"), pad_value)

    def _classify(self, linear, feat):
        """the model's last layer.  With `hip_head` set, an nn.Linear whose width the head kernels take
        (functional.head_supported) runs on them: exact fp32 in a fixed order, so a clip's logits do not depend on the
        batch it came in.  Everything else -- the switch off (the default), nn.Identity for num_classes == 0, the
        Transformer's nn.Sequential 'concat' head -- is the module call it has always been."""
        if self.hip_head and isinstance(linear, nn.Linear) and HF.head_supported(linear.in_features):
            return HF.head_linear(feat, linear.weight, linear.bias)
        return linear(feat)
