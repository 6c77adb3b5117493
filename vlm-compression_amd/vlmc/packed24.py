"""Run a 2:4-pruned model ON its packed weights (include/vlmc.h: vlmc_linear_fwd_24).

The reference's workflow ends in a 2:4-pruned, SparseLoRA-recovered checkpoint (train.py:626-637, :677-714) that
`formats.pack_state_dict_24` shrinks to 9 / 16 of its bytes.  `Linear24` is the module that computes with those bytes:
`pack_model_24_(model)` swaps it in for every linear a 2:4 prune left behind, `unpack_model_24_` swaps the dense linears back,
`formats.load_packed_24` loads a packed state dict into a freshly built dense model.  The forward is bit for bit the dense
layer's on the batch-invariant kernel (`ops.linear_fwd(x, W . mask, bias)`): only bytes and time change.

Inference only: no gradient flows through a `Linear24`, and the dense weight no longer exists (`dense=True` raises).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .formats import PACKED_META, PACKED_VALUES

_16BIT = (torch.float16, torch.bfloat16)


def meta_24_is_valid(meta: torch.Tensor) -> bool:
    """Whether every byte of `meta` holds two codes i0 | i1 << 2 with i0 < i1 -- what `ops.pack_24` writes and the kernels trust."""
    m = meta.to(torch.int16)
    return bool((((m & 3) < ((m >> 2) & 3)) & (((m >> 4) & 3) < ((m >> 6) & 3))).all())


def _mask_nm_from_zeros(weight: torch.Tensor, n: int, m: int, fn: str, words: tuple) -> torch.Tensor:
    """the non-zeros of every group of `m` input columns, filled up with the lowest-index zero columns to exactly `n`"""
    if weight.dim() != 2 or weight.shape[1] % m:
        raise ValueError(f"{fn}: a weight [out, in] with in % {m} == 0 expected")
    nz = (weight != 0).reshape(weight.shape[0], -1, m)
    count = nz.sum(-1, keepdim=True)
    bad = int((count > n).sum())
    if bad:
        raise ValueError(f"{fn}: {bad} groups of {words[1]} columns hold more than {words[0]} non-zero weights: not a {n}:{m} weight")
    zero_rank = (~nz).cumsum(-1)                          # 1 for a group's first zero column, 2 for its second, ..
    return (nz | (~nz & (zero_rank <= n - count))).reshape(weight.shape)


def mask_24_from_zeros(weight: torch.Tensor) -> torch.Tensor:
    """A 2:4 mask for a weight whose masks were dropped and whose zeros were kept (the reference's reload, evaluate_new.py:226-276):
    per group of four input columns the non-zero ones, filled up with the lowest-index zero columns to exactly two.  Raises
    ValueError with the number of groups that hold more than two non-zeros."""
    return _mask_nm_from_zeros(weight, 2, 4, "mask_24_from_zeros", ("two", "four"))


def is_mask_24(mask, shape) -> bool:
    return (torch.is_tensor(mask) and mask.dtype == torch.bool and tuple(mask.shape) == tuple(shape) and len(shape) == 2
            and shape[1] % 8 == 0 and bool((mask.reshape(shape[0], -1, 4).sum(-1) == 2).all()))


class _PackedLinear(nn.Module):
    """What `Linear24`, `packed48.Linear48` and `packedbm.LinearBM` share: everything but the constructor's signature, the buffer names,
    their shapes and the three ops of the format.  A subclass spells its own `__init__(self, <its buffers>, bias=None)` and hands the
    buffers on as one tuple; `cls(*packed, bias=bias)` therefore builds any of them."""
    _NAMES = ()                                          # the state-dict names of the packed buffers, in the order ops.pack_<tag> returns them
    _TAG = None                                          # "24" / "48" / "bm": ops.pack_<tag>, ops.unpack_<tag>, ops.linear_fwd_<tag>
    _LAYOUT = "values [out, in / 2] (fp16 / bf16) and meta [out, in / 8] (uint8)"

    @staticmethod
    def _features(values, meta):
        """(out_features, in_features) of well-formed packed buffers, None otherwise (the two n:m formats' rule)"""
        if values.dim() != 2 or values.dtype not in _16BIT or meta.dtype != torch.uint8 or values.shape[1] % 4 or \
                tuple(meta.shape) != (values.shape[0], values.shape[1] // 4):
            return None
        return values.shape[0], 2 * values.shape[1]

    def __init__(self, packed: tuple, bias: torch.Tensor | None):
        super().__init__()
        cls = type(self).__name__
        feats = self._features(*packed)
        if feats is None:
            raise TypeError(f"{cls}: {self._LAYOUT} expected")
        if bias is not None and (bias.dtype != packed[0].dtype or tuple(bias.shape) != (feats[0],)):
            raise TypeError(f"{cls}: a bias [out] of the values' dtype expected")
        self.out_features, self.in_features = feats
        for name, t in zip(self._NAMES, packed):
            self.register_buffer(name, t.detach().contiguous())
        self.register_buffer("bias", None if bias is None else bias.detach().contiguous())

    @classmethod
    def _op(cls, name: str):
        from . import ops
        return getattr(ops, f"{name}_{cls._TAG}")

    def _packed(self) -> tuple:
        return tuple(getattr(self, name) for name in self._NAMES)

    @property
    def dtype(self):
        return getattr(self, self._NAMES[0]).dtype

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, dtype={self.dtype}"

    def forward(self, x: torch.Tensor, dense: bool = False) -> torch.Tensor:
        cls = type(self).__name__
        if dense:
            raise RuntimeError(f"{cls}: dense=True asks for the unpruned weight, which a packed linear no longer has")
        if x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{cls} is inference only: its input requires a gradient")
        if x.dtype != self.dtype:
            raise TypeError(f"{cls}: input of dtype {x.dtype}, weights packed as {self.dtype}")
        return self._op("linear_fwd")(x, *self._packed(), self.bias)

    @classmethod
    def from_linear(cls, module: nn.Module, mask: torch.Tensor | None = None):
        """Pack `module.weight . mask` (`mask`: the module's own `mask` by default) on the GPU."""
        mask = module.mask if mask is None else mask
        w = module.weight.detach()
        packed = cls._op("pack")(w if w.stride(1) == 1 else w.contiguous(), mask if mask.stride(1) == 1 else mask.contiguous())
        return cls(*packed, bias=None if module.bias is None else module.bias.detach())

    def to_linear(self) -> nn.Linear:
        """The dense `nn.Linear` back: weight W . mask, the `mask` attribute a prune leaves (wanda_pruner.py:339)."""
        w, mask = self._op("unpack")(*self._packed())
        lin = nn.Linear(self.in_features, self.out_features, bias=self.bias is not None, device="meta")
        lin.weight = nn.Parameter(w, requires_grad=False)
        if self.bias is not None:
            lin.bias = nn.Parameter(self.bias.clone(), requires_grad=False)
        lin.mask = mask
        return lin.train(self.training)


class _PackedLinearNM(_PackedLinear):
    """the two n:m formats' constructor: two buffers"""

    def __init__(self, values: torch.Tensor, meta: torch.Tensor, bias: torch.Tensor | None = None):
        super().__init__((values, meta), bias)


class Linear24(_PackedLinearNM):
    """A linear whose weight exists only as `weight_packed24` [out, in / 2] + `weight_meta24` [out, in / 8] (buffers, the names of
    `formats.pack_state_dict_24`) and a `bias` buffer.  `forward(x, dense=False)` takes the reference model files' call
    `lin(x, dense)` (eva_vit.py:54-60)."""
    _NAMES, _TAG = (PACKED_VALUES, PACKED_META), "24"


def _empty_adapter(m) -> bool:
    """A SparseLoRA `Linear` whose adapter adds nothing: r == 0, merged, or lora_B all zero (what `merge()` leaves, lora.py:384-394)."""
    return m.r == 0 or m.merged or not bool(m.lora_B.weight.any())


def _packable(m, from_zeros: bool, is_mask=None, mask_from_zeros=None):
    """The mask under which module `m` can be replaced, or None (`is_mask`, `mask_from_zeros`: the format's; 2:4 by default)."""
    from lavis.peft.src.peft.tuners.lora import Linear as LoraLinear
    is_mask, mask_from_zeros = is_mask or is_mask_24, mask_from_zeros or mask_24_from_zeros
    if type(m) is nn.Linear:
        pass
    elif type(m) is LoraLinear:
        if not (m.sparse and not m.fan_in_fan_out and _empty_adapter(m)):
            return None
    else:
        return None
    w = m.weight
    if w.dtype not in _16BIT or not w.is_cuda or w.shape[1] % 8:
        return None
    mask = getattr(m, "mask", None)
    if torch.is_tensor(mask):
        return mask if is_mask(mask, w.shape) else None
    if from_zeros and type(m) is nn.Linear:
        try:
            mask = mask_from_zeros(w.detach())
        except ValueError:
            return None
        return mask if is_mask(mask, w.shape) else None
    return None


def _replace(model: nn.Module, name: str, new: nn.Module):
    parent_name, _, child = name.rpartition(".")
    setattr(model.get_submodule(parent_name) if parent_name else model, child, new)


def _pack_model_(model: nn.Module, cls, from_zeros: bool, is_mask=None, mask_from_zeros=None) -> list:
    done = []
    for name, m in list(model.named_modules()):
        if not name:
            continue
        mask = _packable(m, from_zeros, is_mask, mask_from_zeros)
        if mask is None:
            continue
        new = cls.from_linear(m, mask)
        new.train(m.training)
        _replace(model, name, new)
        done.append(name)
    return done


def _unpack_model_(model: nn.Module, cls) -> list:
    done = []
    for name, m in list(model.named_modules()):
        if name and isinstance(m, cls):
            _replace(model, name, m.to_linear())
            done.append(name)
    return done


def pack_model_24_(model: nn.Module, from_zeros: bool = False) -> list:
    """Replace, in place, every `nn.Linear` (exact type) that carries a 2:4 `mask` attribute, and every SparseLoRA `Linear` with
    `sparse=True` and an empty adapter, by a `Linear24`.  `from_zeros`: also a plain linear without a mask whose zeros allow a 2:4
    one (`mask_24_from_zeros`).  fp32 linears and masks that are not 2:4 stay as they are.  Returns the names replaced."""
    return _pack_model_(model, Linear24, from_zeros)


def unpack_model_24_(model: nn.Module) -> list:
    """Replace every `Linear24` by its dense `nn.Linear` (`to_linear`).  Returns the names replaced."""
    return _unpack_model_(model, Linear24)
