"""Checkpoint files, optimizer and LR schedule in the reference's formats (reference hwgat/utils.py:71-88, 164-237).

The reference's `utils.py` cannot be imported without its dataset stack (decord, matplotlib); what `main.py` needs from
it for THIS backend's model is small and restated here with the same names, argument meaning and file layout, so a
checkpoint written by either side loads on the other:

  save_checkpoint               utils.py:164-176   torch.save of one dict: 'model_state_dict', 'optimizer_state_dict',
                                                   'train_loss_list', 'val_loss_list', 'train_acc_list', 'val_acc_list',
                                                   'epoch', 'learning_rate', 'scheduler'
  load_weights_from_pretrained  utils.py:185-214   strips a "model." prefix from every key, keeps a tensor only when the
                                                   key exists in the model AND the shapes agree, reports the rest
  load_checkpoint               utils.py:216-237   weights as above + optimizer / scheduler state, start epoch, 4 lists
  get_optimizer / get_scheduler utils.py:71-88     AdamW(lr) by default; CosineAnnealingLR(T_max=20, last_epoch=-1)
  get_device_optimizer          utils.py:71-82     the same four optimizer types on this backend's HIP kernels
  read_extra                    --                 what save_checkpoint(extra=...) put next to the nine keys (train.EpochLoop)
"""
from typing import Optional

import torch

_LISTS = ("train_loss_list", "val_loss_list", "train_acc_list", "val_acc_list")
EXTRA_KEY = "extra"     # this backend's own key next to the reference's nine (save_checkpoint(extra=...), read_extra)


def get_optimizer(model, lr: float = 5e-4, optimizer_type: str = "adamw", fused: Optional[bool] = None,
                  device_step: bool = False):
    """utils.py:71-82 (configs.py:84: lr 5e-4, 'adamw').  `fused=True` selects torch's single-launch AdamW on a GPU.
    `device_step=True` returns optim.DeviceAdamW for 'adamw' / 'adam' (torch's defaults: weight decay 0.01 / 0), the HIP
    optimizer that train.GraphedTrainStep captures inside its graph; for 'nadam' / 'sgd' this keyword raises: use
    `get_device_optimizer`, which covers all four types."""
    # ALL parameters, as the reference passes them (utils.py:76: model.parameters()): the frozen Fourier matrix `B`
    # is an nn.Parameter and therefore entry 0 of the param group, so optimizer_state_dict files interchange with the
    # reference's AdamW (param-group sizes must match).  AdamW skips parameters whose grad is None: B gets no update.
    params = list(model.parameters())
    kinds = {"adamw": torch.optim.AdamW, "adam": torch.optim.Adam, "nadam": torch.optim.NAdam, "sgd": torch.optim.SGD}
    if optimizer_type not in kinds:
        raise ValueError(f"optimizer_type {optimizer_type!r}: one of {sorted(kinds)}")
    if device_step:
        if optimizer_type not in ("adamw", "adam"):
            raise ValueError(f"device_step=True: only 'adamw' or 'adam', not {optimizer_type!r}; "
                             "get_device_optimizer() returns the HIP optimizer of every type")
        from .optim import DeviceAdamW
        adamw = optimizer_type == "adamw"
        return DeviceAdamW(params, lr=lr, weight_decay=1e-2 if adamw else 0.0, decoupled_weight_decay=adamw)
    kw = {"fused": fused} if fused is not None and optimizer_type in ("adamw", "adam") else {}
    return kinds[optimizer_type](params, lr=lr, **kw)


def get_device_optimizer(model, lr: float = 5e-4, optimizer_type: str = "adamw", max_grad_norm: Optional[float] = None,
                         on_nonfinite: str = "propagate", weight_average: Optional[dict] = None):
    """utils.py:71-82 on the HIP optimizers (optim.DeviceAdamW / DeviceNAdam / DeviceSGD), which train.GraphedTrainStep
    captures inside its graph: ALL parameters in one group, as `get_optimizer` passes them, and the values the reference's
    `Class(model.parameters(), lr=cfg.lr)` leaves at torch's defaults -- AdamW weight decay 0.01, Adam and NAdam 0, SGD
    without momentum.  `max_grad_norm` (clip the gradients to that global 2-norm before every step) and `on_nonfinite`
    ("skip": a step with a NaN or Inf gradient changes nothing) attach an `optim.GradGuard` as the optimizer's `guard`
    when either differs from its default; the reference has neither.  `weight_average`: a dict of `optim.WeightAverage`
    keywords (`{}` for the defaults) attaches an EMA / SWA of the model's weights as the optimizer's `averager`."""
    from . import optim
    params = list(model.parameters())
    if optimizer_type == "adamw":
        opt = optim.DeviceAdamW(params, lr=lr, weight_decay=1e-2, decoupled_weight_decay=True)
    elif optimizer_type == "adam":
        opt = optim.DeviceAdamW(params, lr=lr, weight_decay=0.0, decoupled_weight_decay=False)
    elif optimizer_type == "nadam":
        opt = optim.DeviceNAdam(params, lr=lr)
    elif optimizer_type == "sgd":
        opt = optim.DeviceSGD(params, lr=lr)
    else:
        raise ValueError(f"optimizer_type {optimizer_type!r}: one of ['adam', 'adamw', 'nadam', 'sgd']")
    if max_grad_norm is not None or on_nonfinite != "propagate":
        opt.guard = optim.GradGuard(max_norm=float("inf") if max_grad_norm is None else max_grad_norm,
                                    on_nonfinite=on_nonfinite)
    if weight_average is not None:
        opt.averager = optim.WeightAverage(model, **weight_average)
    return opt


def get_scheduler(optimizer, scheduler: Optional[str] = "CosineAnnealingLR"):
    """utils.py:84-89: cosine annealing over 20 scheduler steps (one per epoch in run_epochs, utils.py:263), else None"""
    if scheduler == "CosineAnnealingLR":
        return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=20, last_epoch=-1)
    return None


def _plain(v):
    """a 1-element tensor hyper-parameter (torch optimizers accept a tensor lr) as the Python float the reference writes;
    lists, tuples and dicts element-wise, everything else as it is"""
    if torch.is_tensor(v) and v.numel() == 1:
        return float(v.item())
    if isinstance(v, (list, tuple)):
        return type(v)(_plain(e) for e in v)
    if isinstance(v, dict):
        return {k: _plain(e) for k, e in v.items()}
    return v


def save_checkpoint(path, model, optimizer, scheduler, train_acc_list, train_loss_list, val_acc_list, val_loss_list,
                    epoch, lr, extra=None):
    """same argument order and the same dict layout as utils.py:164-176.  Learning rates are written as floats even when
    the optimizer holds them as tensors: the reference's AdamW(foreach=True) refuses a tensor lr.  `extra` (a dict of
    plain Python values and tensors: numbers, strings, lists, dicts -- what `weights_only=True` loads) goes under one more key,
    'extra', which the reference's loader never looks at; None (the default) writes exactly the reference's nine keys.
    `read_extra` returns it."""
    opt_state = optimizer.state_dict()
    opt_state["param_groups"] = [{k: (v if k == "params" else _plain(v)) for k, v in g.items()}
                                 for g in opt_state["param_groups"]]
    ckpt = {
        "model_state_dict": model.state_dict(),
        "optimizer_state_dict": opt_state,
        "train_loss_list": train_loss_list,
        "val_loss_list": val_loss_list,
        "train_acc_list": train_acc_list,
        "val_acc_list": val_acc_list,
        "epoch": epoch,
        "learning_rate": lr,
        "scheduler": _plain(scheduler.state_dict()),
    }
    if extra is not None:
        if not isinstance(extra, dict):
            raise TypeError(f"extra must be a dict of plain values or None, got {type(extra).__name__}")
        ckpt[EXTRA_KEY] = extra
    torch.save(ckpt, path)


def _read(path, device):
    # a checkpoint is tensors + python scalars / lists: the safe loader suffices (and is required for files that
    # were not written by this process)
    return torch.load(path, map_location=device, weights_only=True)


def read_extra(path, device="cpu"):
    """the dict `save_checkpoint(extra=...)` wrote, {} for a file without one (the reference's own files)"""
    return _read(path, device).get(EXTRA_KEY, {})


def load_weights_from_pretrained(model, pretrained_model_path, device="cpu", report=None):
    """utils.py:185-214.  Returns the model; `report` (a dict, optional) receives the three lists the reference
    prints: keys skipped because absent from the model, keys skipped because of a shape mismatch, model keys the
    file did not provide."""
    ckpt = _read(pretrained_model_path, device)["model_state_dict"]
    pretrained = {k.replace("model.", ""): v for k, v in ckpt.items()}
    own = model.state_dict()
    unknown = [k for k in pretrained if k not in own]
    mismatched = [k for k in pretrained if k in own and pretrained[k].shape != own[k].shape]
    missing = [k for k in own if k not in pretrained]
    for k, v in pretrained.items():
        if k in own and v.shape == own[k].shape:
            own[k] = v
    model.load_state_dict(own)
    model.to(dtype=torch.float)
    if report is not None:
        report.update(unknown=unknown, mismatched=mismatched, missing=missing)
    return model


def load_checkpoint(path, model, optimizer, scheduler, device="cpu", model_weights=None):
    """utils.py:216-237 with the model / optimizer / scheduler passed in (the reference builds them from its cfg).
    Returns (model, optimizer, scheduler, [train_loss, val_loss, train_acc, val_acc], start_epoch)."""
    if model_weights is not None:                         # fine-tuning: weights only, fresh optimizer state
        return load_weights_from_pretrained(model, model_weights, device), optimizer, scheduler, [[], [], [], []], 0
    ckpt = _read(path, device)
    load_weights_from_pretrained(model, path, device)
    optimizer.load_state_dict(ckpt["optimizer_state_dict"])
    scheduler.load_state_dict(ckpt["scheduler"])
    return model, optimizer, scheduler, [ckpt[k] for k in _LISTS], ckpt["epoch"] + 1
