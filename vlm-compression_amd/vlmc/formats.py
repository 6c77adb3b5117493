"""On-disk formats either side of the pruning path, as the reference's drivers write and read them.

Writing (train.py:677-714, after `pruner.prune()` / the RESSA loop):
    pruned_checkpoint/V+L/<pruning_method>/<job_id>.pth   full `model.state_dict()` (incl. the `mask` buffers and LoRA tensors)
    sparsity_dict/<job_id>.yaml                           the dict `prune()` returned, when it is a dict
    training_statistics/<job_id>.yaml                     {"memory": peak GB, "time": seconds}
    importance_scores/<job_id>.pth                        {param name: weight.importance_score}
Reading (evaluate_new.py:226-276, evaluate_old.py:246-290): one tower at a time, dropping LoRA and mask entries and
the PEFT wrapper prefixes, then `load_state_dict` into the tower.

Host-side file formats only: the tensors are whatever the pruners left on the GPU; nothing above touches the kernels.

Packed 2:4 (SURVEY.md §8(f)3 "an optional packed 2:4 format for inference"; the reference has none): `pack_state_dict_24` /
`unpack_state_dict_24` turn the `weight` + `mask` pair of every linear that a 2:4 prune left behind into
`weight_packed24` [out, in / 2] + `weight_meta24` [out, in / 8] (include/vlmc.h: vlmc_pack_24) and back, bit for bit --
9 / 16 of the bytes of the 16-bit weight, 3 / 8 of weight + mask.  Packed 4:8 (the reference's other n:m regime, prune_n = 4,
prune_m = 8): `pack_state_dict_48` / `unpack_state_dict_48` / `load_packed_48`, the same functions over `weight_packed48` +
`weight_meta48` (vlmc_pack_48: one byte per group of eight, bit j = column j kept), the same 9 / 16.  Packed bitmap (ANY mask, what the
unstructured prunes leave): `pack_state_dict_bm` / `unpack_state_dict_bm` / `load_packed_bm` over `weight_packedbm` + `weight_metabm` +
`weight_offsbm` + `weight_rowptrbm` (vlmc_pack_bm), (16 d + 1.5) / 16 of the weight's bytes at kept density d.
"""
from __future__ import annotations

import os
import time

import torch
import yaml

LANGUAGE_TOWERS = ("t5_model", "opt_model", "llm_model")          # the order evaluate_new.py probes them in
VIT_PREFIXES = ("visual.", "visual_encoder.")


def save_pruned_model(model, job_id: str, pruning_method: str, sparsity_dict=None, start_time: float | None = None,
                      root: str = ".") -> dict:
    """train.py:677-714.  Returns the paths written."""
    out = {}
    folder = os.path.join(root, "pruned_checkpoint/V+L", pruning_method)
    os.makedirs(folder, exist_ok=True)
    out["checkpoint"] = os.path.join(folder, job_id + ".pth")
    torch.save(model.state_dict(), out["checkpoint"])
    if sparsity_dict is not None and isinstance(sparsity_dict, dict):
        folder = os.path.join(root, "sparsity_dict")
        os.makedirs(folder, exist_ok=True)
        out["sparsity_dict"] = os.path.join(folder, job_id + ".yaml")
        with open(out["sparsity_dict"], "w") as f:
            yaml.dump(sparsity_dict, f)
    peak_memory = (torch.cuda.max_memory_allocated() / 1024 ** 2) / 1000 if torch.cuda.is_available() else 0.0
    training_dict = {"memory": peak_memory, "time": time.time() - (start_time if start_time is not None else time.time())}
    folder = os.path.join(root, "training_statistics")
    os.makedirs(folder, exist_ok=True)
    out["training_statistics"] = os.path.join(folder, job_id + ".yaml")
    with open(out["training_statistics"], "w") as f:
        yaml.dump(training_dict, f)
    folder = os.path.join(root, "importance_scores")
    os.makedirs(folder, exist_ok=True)
    out["importance_scores"] = os.path.join(folder, job_id + ".pth")
    torch.save({k: v.importance_score for k, v in model.named_parameters() if getattr(v, "importance_score", None) is not None},
               out["importance_scores"])
    return out


def _strip(state, prefix, wrappers):
    """Entries of one tower without LoRA tensors and masks, tower prefix and PEFT wrapper prefixes removed
    (evaluate_new.py:229-231; `str.replace`, i.e. every occurrence, as there)."""
    state = {k: v for k, v in state.items() if k.startswith(prefix) and "lora" not in k and "mask" not in k}
    state = {k.replace(prefix + ".", ""): v for k, v in state.items()}
    for w in wrappers:
        state = {k.replace(w, ""): v for k, v in state.items()}
    return state


def load_pruned_language_model(model, checkpoint: str):
    """evaluate_new.py:226-249: the first of t5_model / opt_model / llm_model the model has receives the pruned weights
    (strict load).  Returns the tower's attribute name, or None when the model has none of them."""
    for tower in LANGUAGE_TOWERS:
        if getattr(model, tower, None) is None:
            continue
        state = torch.load(checkpoint, map_location="cpu")
        wrappers = ("base_model.model.", "base_model.Model.") if tower == "t5_model" else ("base_model.model.",)
        getattr(model, tower).load_state_dict(_strip(state, tower, wrappers))
        return tower
    return None


def load_pruned_vit(model, checkpoint: str, interpolate_pos_embed=None):
    """evaluate_new.py:251-276: the checkpoint's vision entries (prefix `visual.` or `visual_encoder.`) overwrite the
    matching entries of the current vision tower's state dict; unknown keys are ignored, missing ones keep their
    current values.  `interpolate_pos_embed(visual_encoder, state)` is the reference's eva_vit helper, if needed."""
    state = torch.load(checkpoint, map_location="cpu")
    prefix = None
    for cand in VIT_PREFIXES:
        if any(k.startswith(cand) for k in state.keys()):
            prefix = cand
            break
    assert prefix is not None
    state = {k: v for k, v in state.items() if k.startswith(prefix) and "lora" not in k and "mask" not in k}
    state = {k.replace(prefix, ""): v for k, v in state.items()}
    state = {k.replace("base_model.model.", ""): v for k, v in state.items()}
    current = model.visual_encoder.state_dict()
    for k, v in state.items():
        if k in current:
            current[k] = v
    if interpolate_pos_embed is not None:
        interpolate_pos_embed(model.visual_encoder, current)
    model.visual_encoder.load_state_dict(current)
    return prefix


def remaining_proportion(model, orig_total_size) -> float:
    """evaluate_new.py:279-283: non-zero parameters over the original parameter count, in percent."""
    kept = sum((p != 0).float().sum() for p in model.parameters())
    return float(kept / orig_total_size * 100)


PACKED_VALUES, PACKED_META = "weight_packed24", "weight_meta24"
PACKED_VALUES_48, PACKED_META_48 = "weight_packed48", "weight_meta48"
PACKED_VALUES_BM, PACKED_META_BM, PACKED_OFFS_BM, PACKED_ROWPTR_BM = "weight_packedbm", "weight_metabm", "weight_offsbm", "weight_rowptrbm"
_KEYS_24, _KEYS_48 = (PACKED_VALUES, PACKED_META), (PACKED_VALUES_48, PACKED_META_48)
_KEYS_BM = (PACKED_VALUES_BM, PACKED_META_BM, PACKED_OFFS_BM, PACKED_ROWPTR_BM)


def _keeps_half(group: int):
    """the n:m formats' rule: the mask keeps exactly group / 2 of every `group` input columns"""
    return lambda m, shape: bool((m.reshape(shape[0], -1, group).sum(-1) == group // 2).all())


def _pack_state_dict(state: dict, keep_masks: bool, accepts, keys: tuple, pack) -> dict:
    """every (`<name>.weight`, `<name>.mask`) pair whose bool mask the format `accepts(mask, shape)` -> `pack`'s tensors under `keys`"""
    out = {}
    for k, v in state.items():
        if k.endswith(".weight") and k[:-6] + "mask" in state and isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 2 and \
                v.dtype in (torch.float16, torch.bfloat16) and v.shape[1] % 8 == 0:
            m = state[k[:-6] + "mask"]
            if m.shape == v.shape and m.dtype == torch.bool and accepts(m, v.shape):
                w = v if v.stride(1) == 1 else v.contiguous()
                # (what is stored is W . mask: under SparseLoRA the pruned positions of `weight` are zero already, lora.py:362)
                for key, t in zip(keys, pack(w, m if m.stride(1) == 1 else m.contiguous())):
                    out[k[:-6] + key] = t
                continue
        out[k] = v
    if not keep_masks:
        for k in [k for k in out if k.endswith(".mask") and k[:-4] + keys[0] in out]:
            del out[k]
    return out


def _unpack_state_dict(state: dict, device, keys: tuple, unpack) -> dict:
    out = {}
    for k, v in state.items():
        if k.endswith("." + keys[0]):
            base = k[:-len(keys[0])]
            packed = [state[base + key] for key in keys]
            if device is not None:
                packed = [t.to(device) for t in packed]
            w, m = unpack(*(t.contiguous() for t in packed))
            out[base + "weight"], out[base + "mask"] = w, m
        elif not any(k.endswith("." + key) for key in keys[1:]):
            out.setdefault(k, v)
    return out


def _load_packed(model, packed_state: dict, strict: bool, tag: str, keys: tuple, is_valid, cls, checked: tuple = None):
    """swap a `cls` in for every module whose `<name>.<keys[0]>` is in `packed_state` (metadata validated once: `is_valid` takes the
    tensors of keys[1:], then the values; `checked`: the keys a failure is blamed on, keys[1] by default), then load"""
    state, fn = dict(packed_state), "load_packed_" + tag
    for k in [k for k in state if k.endswith("." + keys[0])]:
        name = k[:-len(keys[0]) - 1]
        packed = [state.get(name + "." + key) for key in keys]
        for key, t in zip(keys, packed):
            if t is None:
                raise KeyError(f"{fn}: {name}.{key} is missing")
        if not is_valid(*packed[1:], packed[0]):
            blamed = " / ".join(f"{name}.{key}" for key in (checked or keys[1:2]))
            raise ValueError(f"{fn}: {blamed} {'hold entries' if checked else 'holds codes'} that pack_{tag} never writes")
        old = model.get_submodule(name)
        dev = next((t.device for t in list(old.parameters(recurse=False)) + list(old.buffers(recurse=False))), packed[0].device)
        bias = state.get(name + ".bias")
        new = cls(*(torch.empty_like(t, device=dev) for t in packed), bias=None if bias is None else torch.empty_like(bias, device=dev))
        new.train(old.training)
        parent, _, child = name.rpartition(".")
        setattr(model.get_submodule(parent) if parent else model, child, new)
        state.pop(name + ".mask", None)
    return model.load_state_dict(state, strict=strict)


def pack_state_dict_24(state: dict, keep_masks: bool = False) -> dict:
    """`model.state_dict()` of a 2:4-pruned model with every (`<name>.weight`, `<name>.mask`) pair whose mask keeps exactly two of
    every four input columns replaced by `<name>.weight_packed24` / `<name>.weight_meta24` (CUDA tensors; the kernels pack).
    Pairs that are not 2:4 (unstructured masks, 4:8 masks, fp32 weights, widths that are not multiples of 8) stay as they are.
    `keep_masks`: keep the `mask` entries of packed linears too (they are recoverable from the metadata)."""
    from . import ops
    return _pack_state_dict(state, keep_masks, _keeps_half(4), _KEYS_24, ops.pack_24)


def unpack_state_dict_24(state: dict, device=None) -> dict:
    """The dense state dict back: `<name>.weight` (zeros where nothing was kept) and `<name>.mask` for every packed pair."""
    from . import ops
    return _unpack_state_dict(state, device, _KEYS_24, ops.unpack_24)


def load_packed_24(model, packed_state: dict, strict: bool = True):
    """Load what `pack_state_dict_24` made into a dense model: exactly the modules whose `<name>.weight_packed24` key is in
    `packed_state` become `packed24.Linear24` (on the device of the module they replace), then `model.load_state_dict`.  Each
    `weight_meta24` is validated once here (the kernels trust it); `mask` entries of packed linears (`keep_masks=True`) are
    recoverable from the metadata and dropped.  Afterwards `model.state_dict()` is the packed state: it goes through
    `unpack_state_dict_24` / `pack_state_dict_24` bit for bit.  Returns `load_state_dict`'s result."""
    from . import packed24
    return _load_packed(model, packed_state, strict, "24", _KEYS_24, lambda meta, _values: packed24.meta_24_is_valid(meta), packed24.Linear24)


def pack_state_dict_48(state: dict, keep_masks: bool = False) -> dict:
    """`pack_state_dict_24` for the 4:8 regime: every (`<name>.weight`, `<name>.mask`) pair whose mask keeps exactly four of every
    eight input columns becomes `<name>.weight_packed48` / `<name>.weight_meta48` (include/vlmc.h: vlmc_pack_48), 9 / 16 of the
    weight's bytes; every other pair stays as it is.  A 2:4 mask is also a 4:8 mask and is packed here: run `pack_state_dict_24`
    first on a state dict whose 2:4 linears should get the 2:4 selector form."""
    from . import ops
    return _pack_state_dict(state, keep_masks, _keeps_half(8), _KEYS_48, ops.pack_48)


def unpack_state_dict_48(state: dict, device=None) -> dict:
    """The dense state dict back: `<name>.weight` (zeros where nothing was kept) and `<name>.mask` for every packed 4:8 pair."""
    from . import ops
    return _unpack_state_dict(state, device, _KEYS_48, ops.unpack_48)


def load_packed_48(model, packed_state: dict, strict: bool = True):
    """`load_packed_24` for what `pack_state_dict_48` made: the modules whose `<name>.weight_packed48` key is in `packed_state`
    become `packed48.Linear48`, each `weight_meta48` validated once here (every byte has popcount 4; the kernels trust it)."""
    from . import packed48
    return _load_packed(model, packed_state, strict, "48", _KEYS_48, lambda meta, _values: packed48.meta_48_is_valid(meta), packed48.Linear48)


def pack_state_dict_bm(state: dict, keep_masks: bool = False) -> dict:
    """`pack_state_dict_24` for ANY mask: every (`<name>.weight`, `<name>.mask`) pair of a 16-bit weight (in % 8 == 0, in <= 65536)
    whose packed bytes are fewer than its dense ones becomes `<name>.weight_packedbm` / `weight_metabm` / `weight_offsbm` /
    `weight_rowptrbm` (include/vlmc.h: vlmc_pack_bm), (16 d + 1.5) / 16 of the weight's bytes at kept density d; every other pair stays
    as it is.  n:m masks are masks and are packed here too: run `pack_state_dict_24` / `pack_state_dict_48` FIRST on a state dict whose
    n:m linears should get the tighter 9 / 16 forms."""
    from . import ops, packedbm
    return _pack_state_dict(state, keep_masks, packedbm.is_mask_bm, _KEYS_BM, ops.pack_bm)


def unpack_state_dict_bm(state: dict, device=None) -> dict:
    """The dense state dict back: `<name>.weight` (zeros where nothing was kept) and `<name>.mask` for every bitmap-packed linear."""
    from . import ops
    return _unpack_state_dict(state, device, _KEYS_BM, ops.unpack_bm)


def load_packed_bm(model, packed_state: dict, strict: bool = True):
    """`load_packed_24` for what `pack_state_dict_bm` made: the modules whose `<name>.weight_packedbm` key is in `packed_state` become
    `packedbm.LinearBM`; `weight_offsbm` and `weight_rowptrbm` are validated once here against the bitmap's running popcount
    (`packedbm.meta_bm_is_valid`; the kernels trust them)."""
    from . import packedbm
    return _load_packed(model, packed_state, strict, "bm", _KEYS_BM,
                        lambda meta, offs, rowptr, values: values.dim() == 1 and values.numel() >= 16 and
                        packedbm.meta_bm_is_valid(meta, offs, rowptr, values.numel() - 16), packedbm.LinearBM,
                        checked=(PACKED_OFFS_BM, PACKED_ROWPTR_BM))
