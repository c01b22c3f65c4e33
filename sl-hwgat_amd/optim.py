"""AdamW / Adam on the HIP kernels of csrc/optim.hip (reference: the torch.optim.AdamW that hwgat/utils.py:71-82 builds
and utils.py:93-116 steps).  One launch updates every parameter tensor of the model from a table in device memory, and
every hyper-parameter is a device word the kernels read when they run, so `train.GraphedTrainStep` captures this
optimizer's step inside its graph: a replay is the whole train step, under any torch LR scheduler.

The state is torch's: `param_groups` carry the keys of torch.optim.AdamW, `state[p]` is {"step": 0-d fp32 device
tensor, "exp_avg", "exp_avg_sq"}, and those ARE the tensors the kernels read and write (a caller may seat them itself
before the first step, e.g. as views of one flat arena), so `state_dict()` interchanges
with torch.optim.AdamW (and the reference's) in both directions and `checkpoint.save_checkpoint` / `load_checkpoint`
work unchanged.  There is no CPU fallback: the object can be built, inspected and (de)serialised on CPU tensors, `step()`
on them raises.
"""
import struct

import torch

from ._lib import call, ptr, stream

CHUNK = 4096            # HWGAT_OPTIM_CHUNK: elements per workgroup of hwgat_optim_step
NHYPER = 8              # HWGAT_OPTIM_NHYPER: fp64 words per group
NDERIVED = 8            # HWGAT_OPTIM_NDERIVED: fp32 words per table entry
# hwgat_optim_entry: p, g, m, v, step (pointers), n (int64), group, first_block (int32)
ENTRY = struct.Struct("<5QqIi")
ENTRY_BYTES = ENTRY.size
_STATE_KEYS = ("step", "exp_avg", "exp_avg_sq")


def build_table(records, chunk=CHUNK):
    """records: (p, g, m, v, step addresses, n, group) per tensor that has a gradient, n > 0.  Returns (the packed
    hwgat_optim_entry array as bytes, [first_block per entry], total_blocks): entry i owns ceil(n_i / chunk) workgroups
    from first_block_i on."""
    blob, first, total = bytearray(), [], 0
    for p, g, m, v, step, n, group in records:
        if n <= 0:
            raise ValueError("an empty tensor has no table entry")
        first.append(total)
        blob += ENTRY.pack(p, g, m, v, step, n, group, total)
        total += (n + chunk - 1) // chunk
    if total >= 2 ** 31:
        raise ValueError("more workgroups than one launch holds")
    return bytes(blob), first, total


class _Table:
    """one device table + its derived block; `records` is what the device holds (or, while `pending`, will hold)"""

    def __init__(self, capacity, device):
        self.capacity = capacity
        self.buf = torch.zeros(max(1, capacity) * ENTRY_BYTES, dtype=torch.uint8, device=device)
        self.derived = torch.zeros(max(1, capacity) * NDERIVED, dtype=torch.float32, device=device)
        self.records, self.n, self.total, self.pending = None, 0, 0, None

    def upload(self, blob):
        self.buf[:len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
        self.pending = None


class DeviceAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled_weight_decay=True) or Adam (False) with amsgrad = maximize = False on fp32
    parameters.  `step()`: pushes the param-group values that differ from what the device holds (hwgat_optim_set, one
    tiny launch per changed group), revalidates the table against the current (parameter, gradient) addresses -- a tuple
    compare; rebuilt and uploaded only on change -- then issues hwgat_optim_advance and hwgat_optim_step.  A parameter
    whose grad is None is skipped and gets no state, as in torch.

    Capturing `step()` in a HIP graph: the gradients of a capture come from the graph's pool, so the table the graph's
    launches read is a new one.  `begin_capture()` (before the capture; allocates it) ... the capture, with `step()`
    inside ... `end_capture()` (after it; uploads the table -- capture executes nothing, so that is early enough -- and
    returns it: keep the returned object alive as long as the graph).  Hyper-parameters must be on the device before the
    capture (`push_hyper()`), and before each replay call `push_hyper()` again: it launches only when something changed.
    `train.GraphedTrainStep` does all of this."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled_weight_decay=True,
                 amsgrad=False, maximize=False):
        if amsgrad:
            raise ValueError("DeviceAdamW: amsgrad=True is not supported")
        if maximize:
            raise ValueError("DeviceAdamW: maximize=True is not supported")
        if not 0.0 <= float(lr):
            raise ValueError(f"invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"invalid epsilon: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"invalid weight_decay: {weight_decay}")
        # exactly the keys torch's own class writes into a state_dict, whatever the torch version
        like = torch.optim.AdamW if decoupled_weight_decay else torch.optim.Adam
        defaults = dict(like([torch.nn.Parameter(torch.zeros(1))]).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        capturable=True, decoupled_weight_decay=bool(decoupled_weight_decay))
        self._dev = None
        self._live = {}              # parameter -> (step, exp_avg, exp_avg_sq): the tensors the device tables point at
        self._key = None             # ((p address, g address) ...) of the eager table
        self._table = None
        self._capture = None
        self._hyper = None           # device block, NHYPER fp64 per group
        self._held = []              # host mirror of it, one tuple per group
        super().__init__(params, defaults)

    # ---- construction-time checks
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            if p.dtype != torch.float32:
                raise ValueError(f"DeviceAdamW needs float32 parameters, got {p.dtype}")
        self._key = self._dev = None

    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    # ---- hyper-parameters
    @staticmethod
    def _group_values(group):
        if group.get("amsgrad", False):
            raise ValueError("DeviceAdamW: amsgrad=True is not supported")
        if group.get("maximize", False):
            raise ValueError("DeviceAdamW: maximize=True is not supported")
        b1, b2 = group["betas"]
        return (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                bool(group.get("decoupled_weight_decay", True)))

    def _device(self):
        if self._dev is not None:
            return self._dev
        ps = self._params()
        if not ps or not all(p.is_cuda for p in ps):
            raise RuntimeError("DeviceAdamW.step needs its parameters on an MI355X device; there is no CPU fallback")
        if any(p.device != ps[0].device for p in ps):
            raise ValueError("DeviceAdamW needs all parameters on one device")
        self._dev = ps[0].device                 # checked once per set of parameters
        return self._dev

    def push_hyper(self):
        """make the device block hold what `param_groups` say: one hwgat_optim_set launch per group that changed"""
        n = len(self.param_groups)
        if self._hyper is None or self._hyper.numel() < n * NHYPER:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceAdamW: take one eager step (or push_hyper()) before capturing")
            self._hyper = torch.zeros(n * NHYPER, dtype=torch.float64, device=self._device())
            self._held = [None] * n
        for i, group in enumerate(self.param_groups):
            vals = self._group_values(group)
            if vals != self._held[i]:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("DeviceAdamW: a hyper-parameter changed inside a capture; push_hyper() before it")
                call("hwgat_optim_set", ptr(self._hyper), i, *vals[:5], int(vals[5]), stream())
                self._held[i] = vals

    def device_hyper(self):
        """what the device block holds, read back: per group {lr, betas, eps, weight_decay, decoupled_weight_decay}"""
        h = self._hyper.cpu().view(-1, NHYPER).tolist()
        return [dict(lr=r[0], betas=(r[1], r[2]), eps=r[3], weight_decay=r[4], decoupled_weight_decay=r[5] == 0.0)
                for r in h[:len(self.param_groups)]]

    # ---- state and table
    def _state_of(self, p, create):
        st = self.state[p]
        if len(st) == 0:
            if not create:
                raise RuntimeError("DeviceAdamW: a parameter would get its state inside a capture; warm up with one eager step")
            if p in self._live:                  # had state before (a load_state_dict without it): same tensors, fresh
                live = self._live[p]
                for t in live:
                    t.zero_()
            else:
                live = (torch.zeros((), dtype=torch.float32, device=p.device),
                        torch.zeros_like(p, memory_format=torch.contiguous_format),
                        torch.zeros_like(p, memory_format=torch.contiguous_format))
                self._live[p] = live
            st.update(zip(_STATE_KEYS, live))
        elif p not in self._live:                # state seated by the caller (e.g. views of a flat arena): adopt it
            live = tuple(st[k] for k in _STATE_KEYS)
            step, m, v = live
            if not (step.dtype == m.dtype == v.dtype == torch.float32 and step.numel() == 1 and m.shape == v.shape == p.shape
                    and m.is_contiguous() and v.is_contiguous() and step.device == m.device == v.device == p.device):
                raise ValueError("DeviceAdamW: state tensors must be float32 on the parameter's device, the moments "
                                 "contiguous and of its shape, the step count one element")
            self._live[p] = live
        return st

    def table_records(self, create=True):
        """(p, g, m, v, step addresses, n, group) of every non-empty parameter that has a gradient, in group order;
        creates the state of a parameter the first time it has one"""
        recs = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                if g.is_sparse:
                    raise ValueError("DeviceAdamW does not support sparse gradients")
                if g.dtype != torch.float32 or not g.is_contiguous() or not p.is_contiguous() or g.shape != p.shape:
                    raise ValueError("DeviceAdamW needs contiguous float32 parameters and gradients of one shape")
                st = self._state_of(p, create)
                recs.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             st["step"].data_ptr(), p.numel(), gi))
        return recs

    def _address_key(self):
        return tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for p in self._params())

    def _fill(self, table, defer):
        recs = self.table_records(create=not defer)
        table.records = recs
        table.n = len(recs)
        if recs:
            blob, _, table.total = build_table(recs)
            if defer:
                table.pending = blob
            else:
                table.upload(blob)

    def begin_capture(self):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("begin_capture() goes before the capture")
        self._capture = _Table(len(self._params()), self._device())

    def end_capture(self):
        """upload the table the captured launches read; returns it (the graph's owner keeps it alive)"""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("end_capture() goes after the capture")
        table, self._capture = self._capture, None
        if table is not None and table.pending is not None:
            table.upload(table.pending)
        return table

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev = self._device()
        self.push_hyper()
        if torch.cuda.is_current_stream_capturing():
            table = self._capture
            if table is None:
                raise RuntimeError("DeviceAdamW: begin_capture() before a capture that holds step()")
            if table.records is None:
                self._fill(table, defer=True)
            elif self.table_records(create=False) != table.records:   # a later step of the same capture: same tensors
                raise RuntimeError("DeviceAdamW: the steps of one capture must see the same parameters and gradients")
        else:
            key = self._address_key()
            if self._table is None or self._table.capacity < len(key):
                self._table, self._key = _Table(len(key), dev), None
            table = self._table
            if key != self._key:
                self._fill(table, defer=False)
                self._key = key
        if table.n:
            call("hwgat_optim_advance", ptr(table.buf), table.n, ptr(self._hyper), ptr(table.derived), stream())
            call("hwgat_optim_step", ptr(table.buf), table.n, ptr(table.derived), table.total, stream())
        return loss

    # ---- (de)serialisation: the loaded values go INTO the live tensors, whose addresses device tables (a captured
    # graph's among them) hold
    @torch.no_grad()
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._group_values(group)
            group["capturable"] = True
            for p in group["params"]:
                st, live = self.state.get(p), self._live.get(p)
                if not st:
                    if live is not None:         # the file has no state for it: fresh state in the same tensors
                        for t in live:
                            t.zero_()
                        self.state[p].update(zip(_STATE_KEYS, live))
                    continue
                new = (torch.as_tensor(st.get("step", 0.0), dtype=torch.float32).reshape(()),
                       st["exp_avg"], st["exp_avg_sq"])
                if live is None:
                    live = tuple(t.detach().to(device=p.device, dtype=torch.float32).contiguous().clone() for t in new)
                    self._live[p] = live
                else:
                    for dst, src in zip(live, new):
                        dst.copy_(src.to(device=dst.device, dtype=torch.float32).reshape(dst.shape))
                st.update(zip(_STATE_KEYS, live))
        self._key = None
