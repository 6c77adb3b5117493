"""Run a 4:8-pruned model ON its packed weights (include/vlmc.h: vlmc_linear_fwd_48).

The reference publishes three sparsity regimes; 4:8 (`prune_n = 4`, `prune_m = 8` in every pruner) is the second n:m one, and a
4:8-pruned, SparseLoRA-recovered checkpoint comes out of the same workflow as a 2:4 one (train.py:626-637, :677-714).  This is
`packed24` for that regime: `Linear48` computes with `weight_packed48` [out, in / 2] + `weight_meta48` [out, in / 8] (one byte
per group of eight input columns, bit j = column j kept) -- 9 / 16 of the weight's bytes, the forward bit for bit the dense
layer's on the batch-invariant kernel (`ops.linear_fwd(x, W . mask, bias)`).  `pack_model_48_(model)` swaps it in for every linear
a 4:8 prune left behind, `unpack_model_48_` swaps the dense linears back, `formats.load_packed_48` loads a packed state dict into
a freshly built dense model.

Every 2:4 mask is also a 4:8 mask, and everything here accepts such masks: a caller who wants the 2:4 selector form (`packed24`)
for the 2:4 linears of a model runs `pack_model_24_` first; what it leaves is then packed here.

Inference only: no gradient flows through a `Linear48`, and the dense weight no longer exists (`dense=True` raises).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .formats import PACKED_META_48, PACKED_VALUES_48
from .packed24 import _mask_nm_from_zeros, _pack_model_, _PackedLinearNM, _unpack_model_


def meta_48_is_valid(meta: torch.Tensor) -> bool:
    """Whether every byte of `meta` has exactly four bits set -- what `ops.pack_48` writes and the kernels trust."""
    m = meta.to(torch.int16)
    return bool((sum((m >> j) & 1 for j in range(8)) == 4).all())


def mask_48_from_zeros(weight: torch.Tensor) -> torch.Tensor:
    """A 4:8 mask for a weight whose masks were dropped and whose zeros were kept (the reference's reload, evaluate_new.py:226-276):
    per group of eight input columns the non-zero ones, filled up with the lowest-index zero columns to exactly four.  Raises
    ValueError with the number of groups that hold more than four non-zeros.  (A 2:4 weight passes: it is a 4:8 weight too.)"""
    return _mask_nm_from_zeros(weight, 4, 8, "mask_48_from_zeros", ("four", "eight"))


def is_mask_48(mask, shape) -> bool:
    return (torch.is_tensor(mask) and mask.dtype == torch.bool and tuple(mask.shape) == tuple(shape) and len(shape) == 2
            and shape[1] % 8 == 0 and bool((mask.reshape(shape[0], -1, 8).sum(-1) == 4).all()))


class Linear48(_PackedLinearNM):
    """A linear whose weight exists only as `weight_packed48` [out, in / 2] + `weight_meta48` [out, in / 8] (buffers, the names of
    `formats.pack_state_dict_48`) and a `bias` buffer.  `forward(x, dense=False)` takes the reference model files' call
    `lin(x, dense)` (eva_vit.py:54-60) and refuses what `Linear24` refuses."""
    _NAMES, _TAG = (PACKED_VALUES_48, PACKED_META_48), "48"


def pack_model_48_(model: nn.Module, from_zeros: bool = False) -> list:
    """Replace, in place, every `nn.Linear` (exact type) that carries a 4:8 `mask` attribute, and every SparseLoRA `Linear` with
    `sparse=True` and an empty adapter, by a `Linear48`.  `from_zeros`: also a plain linear without a mask whose zeros allow a 4:8
    one (`mask_48_from_zeros`).  fp32 linears and masks that are not 4:8 stay as they are; a 2:4 mask IS a 4:8 mask and is packed
    (run `pack_model_24_` first to give such linears the 2:4 form).  Returns the names replaced."""
    return _pack_model_(model, Linear48, from_zeros, is_mask_48, mask_48_from_zeros)


def unpack_model_48_(model: nn.Module) -> list:
    """Replace every `Linear48` by its dense `nn.Linear` (`to_linear`).  Returns the names replaced."""
    return _unpack_model_(model, Linear48)
