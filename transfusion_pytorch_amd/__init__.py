"""transfusion_pytorch_amd - MI355X-native Transfusion training / sampling hot path.

Mirrors the reference's public surface (transfusion_pytorch/__init__.py:1-6)."""
from .transfusion import (
    Transfusion,
    Transformer,
    LossBreakdown,
    TokenLosses,
    print_modality_sample,
    create_dataloader,
    exists,
    apply_fn_modality_type,
    stack_same_shape_tensors_with_inverse,
    filter_with_inverse,
    random_modality_length_to_time_fn,
    default_modality_length_to_time_fn,
)

from .ema import EMA
from .self_flow import SelfMaskedRepTraining, default_rep_loss_fn
from .optim import FusedAdamAtan2, FusedMuonAdamAtan2, AdamAtan2
from .lora import add_lora_, lora_parameters, merge_lora_, remove_lora_

__all__ = ['Transfusion', 'Transformer', 'LossBreakdown', 'TokenLosses', 'print_modality_sample', 'create_dataloader', 'EMA', 'SelfMaskedRepTraining', 'default_rep_loss_fn',
           'FusedAdamAtan2', 'FusedMuonAdamAtan2', 'AdamAtan2', 'add_lora_', 'lora_parameters', 'merge_lora_', 'remove_lora_']
