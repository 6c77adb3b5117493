"""Run an UNSTRUCTURED-pruned model ON its packed weights (include/vlmc.h: vlmc_linear_fwd_bm).

Unstructured masks are what every pruner here produces by default (the 50 % Wanda prune of the benchmark, DSnoT, SparseGPT, the
global pruners, every ECoFLaP allocation: wanda_pruner.py:330-339); `packed24` / `packed48` only take the two n:m regimes.  This is
their sibling for ANY bool mask: `LinearBM` computes with the bitmap format -- `weight_packedbm` [nnz + 16] (the kept weights, row after
row), `weight_metabm` [out, in / 8] (bit j of byte c = column 8c + j kept), `weight_offsbm` [out, ceil(in / 32)] uint16 and
`weight_rowptrbm` [out + 1] int64 -- (16 d + 1.5) / 16 of the weight's bytes at kept density d, 9.5 / 16 at 50 %, the forward bit for
bit the dense layer's on the batch-invariant kernel (`ops.linear_fwd(x, W . mask, bias)`).  `pack_model_bm_(model)` swaps it in for
every masked 16-bit linear that gets smaller by it, `unpack_model_bm_` swaps the dense linears back, `formats.load_packed_bm` loads a
packed state dict into a freshly built dense model.

ORDER: every 2:4 and 4:8 mask is a mask, and would be packed here at 9.5 / 16; the n:m forms take 9 / 16.  A caller who wants them runs
`pack_model_24_`, then `pack_model_48_`, then `pack_model_bm_`: each walk leaves the `Linear24` / `Linear48` modules before it alone.

Inference only: no gradient flows through a `LinearBM`, and the dense weight no longer exists (`dense=True` raises).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .formats import PACKED_META_BM, PACKED_OFFS_BM, PACKED_ROWPTR_BM, PACKED_VALUES_BM
from .packed24 import _16BIT, _pack_model_, _PackedLinear, _unpack_model_

MAX_IN_FEATURES = 65536                                  # offs counts a row's kept columns in 16 bits


def packed_bm_bytes(out_features: int, in_features: int, nnz: int) -> int:
    """Bytes of the four packed tensors of a 16-bit weight [out, in] with `nnz` kept positions."""
    return (nnz + 16) * 2 + out_features * in_features // 8 + 2 * out_features * ((in_features + 31) // 32) + 8 * (out_features + 1)


def _u16(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16).to(torch.int64) & 0xffff


def meta_bm_is_valid(meta: torch.Tensor, offs: torch.Tensor, rowptr: torch.Tensor, nnz: int) -> bool:
    """Whether `offs` and `rowptr` are the running popcounts of the bitmap `meta` and `rowptr[out] == nnz` -- what `ops.pack_bm` writes
    and the kernels trust."""
    out_f, chunks = meta.shape
    steps = (chunks + 3) // 4
    if tuple(offs.shape) != (out_f, steps) or tuple(rowptr.shape) != (out_f + 1,) or offs.dtype != torch.uint16 or rowptr.dtype != torch.int64:
        return False
    m = meta.to(torch.int64)
    count = sum((m >> j) & 1 for j in range(8))                                        # kept columns per chunk
    count = torch.nn.functional.pad(count, (0, 4 * steps - chunks)).reshape(out_f, steps, 4).sum(-1)
    before = count.cumsum(1) - count                                                   # kept columns of the row before step s
    rows = torch.nn.functional.pad(count.sum(1).cumsum(0), (1, 0))
    return bool((_u16(offs) == before).all()) and bool((rowptr.to(rows.device) == rows).all()) and int(rows[-1]) == int(nnz)


def mask_bm_from_zeros(weight: torch.Tensor) -> torch.Tensor:
    """The mask of a weight whose masks were dropped and whose zeros were kept (the reference's reload, evaluate_new.py:226-276):
    `weight != 0` (a -0.0 is a zero)."""
    if weight.dim() != 2:
        raise ValueError("mask_bm_from_zeros: a weight [out, in] expected")
    return weight != 0


def is_mask_bm(mask, shape) -> bool:
    """A bool mask of `shape` that the format takes (in % 8 == 0, in <= 65536) AND under which the packed bytes are fewer than the
    dense ones (below a kept density of about 0.9)."""
    if not (torch.is_tensor(mask) and mask.dtype == torch.bool and tuple(mask.shape) == tuple(shape) and len(shape) == 2
            and shape[0] > 0 and shape[1] % 8 == 0 and 0 < shape[1] <= MAX_IN_FEATURES):
        return False
    return packed_bm_bytes(shape[0], shape[1], int(mask.sum())) < 2 * shape[0] * shape[1]


class LinearBM(_PackedLinear):
    """A linear whose weight exists only as `weight_packedbm`, `weight_metabm`, `weight_offsbm` and `weight_rowptrbm` (buffers, the
    names of `formats.pack_state_dict_bm`) and a `bias` buffer.  `forward(x, dense=False)` takes the reference model files' call
    `lin(x, dense)` (eva_vit.py:54-60) and refuses what `Linear24` refuses."""
    _NAMES, _TAG = (PACKED_VALUES_BM, PACKED_META_BM, PACKED_OFFS_BM, PACKED_ROWPTR_BM), "bm"
    _LAYOUT = "values [nnz + 16] (fp16 / bf16), meta [out, in / 8] (uint8), offs [out, ceil(in / 32)] (uint16) and rowptr [out + 1] (int64)"

    def __init__(self, values: torch.Tensor, meta: torch.Tensor, offs: torch.Tensor, rowptr: torch.Tensor, bias: torch.Tensor | None = None):
        super().__init__((values, meta, offs, rowptr), bias)

    @staticmethod
    def _features(values, meta, offs, rowptr):
        if values.dim() != 1 or values.dtype not in _16BIT or values.numel() < 16 or meta.dim() != 2 or meta.dtype != torch.uint8 or \
                not 0 < 8 * meta.shape[1] <= MAX_IN_FEATURES or offs.dtype != torch.uint16 or \
                tuple(offs.shape) != (meta.shape[0], (meta.shape[1] + 3) // 4) or rowptr.dtype != torch.int64 or \
                tuple(rowptr.shape) != (meta.shape[0] + 1,):
            return None
        return meta.shape[0], 8 * meta.shape[1]


def pack_model_bm_(model: nn.Module, from_zeros: bool = False) -> list:
    """Replace, in place, every 16-bit `nn.Linear` (exact type) that carries a bool `mask` attribute of its shape, and every SparseLoRA
    `Linear` with `sparse=True` and an empty adapter, by a `LinearBM` -- where the packed bytes are fewer than the dense ones.
    `from_zeros`: also a plain linear without a mask, under `mask_bm_from_zeros`.  fp32 linears, masks denser than break-even and
    `Linear24` / `Linear48` modules stay as they are (run `pack_model_24_` / `pack_model_48_` FIRST for the tighter n:m forms).
    Returns the names replaced."""
    return _pack_model_(model, LinearBM, from_zeros, is_mask_bm, mask_bm_from_zeros)


def unpack_model_bm_(model: nn.Module) -> list:
    """Replace every `LinearBM` by its dense `nn.Linear` (`to_linear`).  Returns the names replaced."""
    return _unpack_model_(model, LinearBM)
