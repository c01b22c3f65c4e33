"""sl-hwgat_amd: MI355X (gfx950) backend for the HWGAT hot path.

The directory name carries a hyphen (it mirrors the upstream project name), so
import it with importlib:

    import importlib
    hw = importlib.import_module("sl-hwgat_amd")
    model = hw.Model(*hw.HWGATEParams({'src_len': 128, 'num_class': 2002}, 2, dev).get_model_params())
"""
from . import _lib
from . import functional
from . import checkpoint
from . import augment
from . import evaluate
from . import optim
from . import data
from .parts import part_table
from .models.HWGATE import Model
from .models.HGATE import Model as HGATEModel
from .models.WGATE import Model as WGATEModel
from .models.GATE import Model as GATEModel
from .models.Transformer import Model as TransformerModel
from .models.STGCN import Model as STGCNModel
from .models.DecoupledGCN import Model as DecoupledGCNModel
from .models.model_params import (HWGATEParams, HGATEParams, WGATEParams, GATEParams, TransformerParams, STGCNParams,
                                  DecoupledGCNParams)
from . import explain
from . import modality
from . import ensemble

__all__ = ["Model", "HWGATEParams", "HGATEModel", "HGATEParams", "WGATEModel", "WGATEParams", "GATEModel", "GATEParams",
           "TransformerModel",
           "TransformerParams", "STGCNModel", "STGCNParams", "DecoupledGCNModel", "DecoupledGCNParams", "functional",
           "part_table", "_lib", "checkpoint", "augment", "evaluate", "optim", "data", "explain",
           "modality", "ensemble"]
