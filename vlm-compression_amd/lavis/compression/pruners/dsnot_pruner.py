"""DSnoT pruners behind the reference's `lavis.compression` API, running on the gfx950 kernels
(`vlmc.dsnot`): `t5_dsnot_pruner`, `vit_dsnot_pruner`, `blipt5_dsnot_pruner`.

Reference: lavis/compression/pruners/dsnot_pruner.py (T5LayerDSnoTPruner :107-858,
VITLayerDSnoTPruner :861-1596, BLIPT5LayerDSnoTPruner :1599-1878).  Same registry names,
constructor kwargs, `prune(...) -> (model, sparsity_dict | None)` contract and side effects
(`module.mask` bool [out,in] True = keep; weights zeroed in place unless `lora_model`; no
`importance_score` -- the reference's assignment is commented out, :365).

  reference op sequence (per linear)                        here
  -------------------------------------------------------  -----------------------------------
  hook: var / norm**2 / sum over tokens, running means       vlmc_act_moments (one launch per
  (WrappedGPT.add_batch :79-101)                             DISTINCT input tensor) +
                                                             vlmc_dsnot_stats_update
  three full sorts, reorder_indices (python loop over        vlmc_wanda_select (initial mask) +
  rows), <= max_cycle_time cycles of ~20 small kernels       vlmc_dsnot_refine (one launch, one
  (:553-751 / n:m :407-552; the ViT copy is identical and    workgroup per row) + vlmc_dsnot_apply
  per-row as well, :1285-1482)

Differences that are visible to a caller:
* the standalone tower pruners accept `initial_method` (the reference reads
  `self.initial_method` in `_prune` but only the BLIP pruner sets it, :1675, so its tower
  classes cannot run on their own);
* `initial_method="sparsegpt"` runs (the reference's branch cannot: its `WrappedGPT` is built
  without `initial_method`, :340 / ViT :1073, so `H` is never allocated).  Its contract here: the
  Hessian of SparseGPT's `add_batch` (sparsegpt_pruner.py:68-79) over the statistics pass's calls,
  shared by the linears fed the same tensor; `H[dead, dead] = 1`, ONE unconditional damp of
  0.01 * mean(diag H), `U = cholesky(cholesky_inverse(cholesky(H)), upper)` (a non positive
  definite H raises VlmcError(VLMC_ENOTPD)), initial metric fp32(w*w) / diag(U) with dead columns 0
  (:380-402), then DSnoT's cycles as for the other initial methods; the weights are not
  reconstructed (no OBS update), only masked;
* `max_cycle_time >= in_features` raises instead of indexing out of range.

This module holds the DSnoT statistics, options, per-block step and the BLIP pruner's gating; the tower step, the tower
sequence, the constructor keywords and the shared SparseGPT Hessians (`initial_method="sparsegpt"`) are in `tower_walk.py`.

There is no CPU fallback: without the HIP library or a GPU model the pruner raises.
"""
from __future__ import annotations


import torch

from lavis.common.registry import registry
from lavis.compression.pruners import calibration as cal
from lavis.compression.pruners.tower_walk import (SharedHessians, TowerKind, TowerPruner, autocast_bf16,
                                                  input_signature)
from lavis.compression.pruners.utils import print_time
from lavis.compression.pruners.wanda_pruner import uniform_or_layer_sparsity
from vlmc import config

_VERBOSE = config.flag("VLMC_VERBOSE")


class DsnotStatCollector:
    """Forward hooks on the linears of one block (dsnot_pruner.py:338-356).  Linears fed by the
    very same tensor (q/k/v, wi_0/wi_1) share one moments launch and one statistic."""

    def __init__(self, subset, hessians=False):
        from vlmc import dsnot
        self._dsnot = dsnot
        self.subset = subset
        self.calls = {n: [] for n in subset}              # per linear: one record (of one or more samples) per hook call
        self._cache = {}
        self._cur = -1
        # initial_method="sparsegpt": per linear the SparseGPT Hessian accumulator of its input (shared like the statistics);
        # None on the other routes (no launches, no memory)
        self._shared = SharedHessians(subset) if hessians else None
        self.hessians = self._shared.wrapped if hessians else None
        self.handles = [m.register_forward_hook(self._make_hook(n)) for n, m in subset.items()]

    def _make_hook(self, name):
        def hook(_module, inp, _out):
            x = inp[0].data
            if x.dim() == 2:
                x = x.unsqueeze(0)
            key = input_signature(x)
            hit = self._cache.get(key)
            if hit is None:
                stacked = cal.stacked_samples()              # batched replay: one record per stacked calibration sample
                calls, _b0, idx = stacked if stacked and stacked[0] * stacked[1] == x.shape[0] else (1, x.shape[0], (self._cur,))
                st = self._dsnot.DsnotInputStat(x.shape[-1], x.device)
                # a padded group of ragged samples: the token rows of sample c that are its own (the rest is padding, never read);
                # the cross-attention's k / v see the ENCODER's padded length: the lookup is by this input's own token dimension
                lens = cal.stacked_lengths(x.shape[1]) if calls > 1 else None
                if lens is None and cal.in_padded_group():
                    raise RuntimeError(f"{name}: a linear input of shape {tuple(x.shape)} inside a padded group of ragged samples "
                                       "carries no per-sample token counts (VLMC_DSNOT_PAD=0 forwards groups of equal shape)")
                if lens is None:
                    st.add_calls(x, calls, idx)              # ONE launch: sum of squares, sum, variance over tokens, per sample
                else:
                    st.add_calls(x, calls, idx, call_tokens=lens, host_tokens=cal.stacked_host_lengths(x.shape[1]))
                hit = (x, st)                                # `x` stays referenced until the next sample (see wanda collector)
                self._cache[key] = hit
            self.calls[name].append(hit[1])
            if self._shared is not None:
                self._shared.add(name, key, x)
        return hook

    def next_sample(self, j=None):
        self._cache.clear()
        if self._shared is not None:
            self._shared.begin_forward()
        self._cur = self._cur + 1 if j is None else j

    def close(self):
        for h in self.handles:
            h.remove()
        self.handles = []
        self._cache.clear()
        if self._shared is not None:
            self._shared.begin_forward()

    def finalize(self):
        """{name: DsnotInputStat}; linears whose hooks saw identical tensors share the object."""
        shared, out, order = {}, {}, []
        for name, calls in self.calls.items():
            sig = tuple(id(c) for c in calls)                # (DsnotInputStat.ordered() restores the reference's sample order)
            st = shared.get(sig)
            if st is None:
                mod = self.subset[name]
                st = self._dsnot.DsnotInputStat(mod.weight.shape[1], mod.weight.device)
                for c in calls:
                    st.extend(c)
                shared[sig] = st
                order.append(st)
            out[name] = st
        self._dsnot.gather_stats(order)
        if self.hessians is not None:
            self._divisors(out)
        return out

    def _divisors(self, stats):
        """Sample-sharded runs exchange the Hessians (the sample-weighted mean, as the SparseGPT pruner); then every distinct
        input's divisor goes onto its statistic and the H buffers are freed."""
        from vlmc.shard import require_real_exchange
        unique = self._shared.unique()
        require_real_exchange("blipt5_dsnot_pruner (initial_method='sparsegpt')")
        self._shared.allreduce()
        acc_of_stat = {}
        for name, acc in self.hessians.items():
            if acc_of_stat.setdefault(id(stats[name]), acc) is not acc:
                raise RuntimeError(f"{name}: linears that share DSnoT statistics must share one Hessian")
        divs = self._dsnot.sparsegpt_divisors([acc.H for acc in unique])
        by_acc = {id(acc): d for acc, d in zip(unique, divs)}
        for name, acc in self.hessians.items():
            stats[name].divisor = by_acc[id(acc)]
        for acc in unique:
            acc.free()
        self.hessians = {}


_DSNOT_KW = dict(initial_method="wanda", skip_layer=None, skip_sub_layer=None, pow_of_var_regrowing=1., max_cycle_time=1e2,
                 update_threshold=0.1, without_same_sign=True, without_DSnoT=False)


class _DsnotPruner(TowerPruner):
    """The DSnoT options, tower kinds and per-block step; the reference's T5/LLM and ViT `_prune` bodies are the same code,
    and its ViT blocks run under bf16 autocast like the T5 ones (:1086, :1493)."""
    llm_kind = TowerKind(vit=False, tuple_output=True, autocast=autocast_bf16,
                         pad_ragged=lambda: config.flag("VLMC_DSNOT_PAD"))
    vit_kind = TowerKind(vit=True, tuple_output=False, autocast=autocast_bf16, pad_ragged=None)

    def __init__(self, model, data_loader, model_prefix, **kwargs):
        super().__init__(model, data_loader, model_prefix, **kwargs)
        for name, default in _DSNOT_KW.items():
            setattr(self, name, kwargs.get(name, default))

    def get_sparsity(self, original_sparsity, sparsity_ratio_granularity=None):
        return uniform_or_layer_sparsity(self, original_sparsity, sparsity_ratio_granularity)

    def _block_step(self, i, subset, run_pass, n_inps, batch0, *, kind, module_to_process, model_prefix, sparsity_ratio,
                    lora_model):
        from vlmc import dsnot
        col = DsnotStatCollector(subset, hessians=self.initial_method == "sparsegpt")
        try:
            run_pass(col.next_sample, outputs=False)
        finally:
            col.close()
        stats = col.finalize()
        for name, mod in subset.items():
            st = stats[name]
            assert st.nsamples == n_inps * batch0                               # dsnot_pruner.py:359
            W = mod.weight.data
            if not W.is_contiguous():
                raise RuntimeError(f"{name}: weight must be contiguous")
            if self.prune_n != 0:
                ratio = None
                if _VERBOSE:
                    print(f"pruning {model_prefix} layer {i} {name} at structured {self.prune_n}:{self.prune_m} sparsity")
            else:
                ratio = sparsity_ratio[f"{module_to_process}.{i}.{name}.weight"]
                if _VERBOSE:
                    print(f"pruning {model_prefix} layer {i} {name} at unstructured {ratio} sparsity")
            keep = dsnot.prune_linear(W, st, ratio, prune_n=self.prune_n, prune_m=self.prune_m,
                                      initial_method=self.initial_method, without_DSnoT=self.without_DSnoT,
                                      max_cycle_time=self.max_cycle_time, update_threshold=self.update_threshold,
                                      pow_of_var_regrowing=self.pow_of_var_regrowing,
                                      without_same_sign=self.without_same_sign, apply_zero=not lora_model)
            if keep is None:                                                     # ratio == 0: `continue` (:560-561)
                continue
            setattr(mod, "mask", keep)                                           # True = keep (:753)


@registry.register_pruner("t5_dsnot_pruner")
class T5LayerDSnoTPruner(_DsnotPruner):
    """T5 / OPT / LLaMA tower (dsnot_pruner.py:107-858)."""
    pruner_name = "t5_dsnot_pruner"
    tower_kind = _DsnotPruner.llm_kind

    def __init__(self, model, data_loader, model_prefix="t5_model", **kwargs):
        super().__init__(model, data_loader, model_prefix, **kwargs)

    def forward_to_cache(self, model, batch, lora_model=False):
        return model(batch)

    @cal.quiet_gc
    @print_time
    def prune(self, importance_scores=None, keep_indices_or_masks=None, lora_model=False):
        return self._prune_alone(("encoder.block", "decoder.block"), lora_model)             # :842-857


@registry.register_pruner("vit_dsnot_pruner")
class VITLayerDSnoTPruner(_DsnotPruner):
    """EVA ViT tower (dsnot_pruner.py:861-1596): the same per-row procedure; blocks return a tensor."""
    pruner_name = "vit_dsnot_pruner"
    tower_kind = _DsnotPruner.vit_kind

    def __init__(self, model, data_loader, model_prefix="visual", **kwargs):
        super().__init__(model, data_loader, model_prefix, **kwargs)

    def forward_to_cache(self, model, batch, lora_model=False):
        return model.encode_image(batch["image"])

    @cal.quiet_gc
    @print_time
    def prune(self, importance_scores=None, keep_indices_or_masks=None, lora_model=False):
        return self._prune_alone(("blocks",), lora_model)


@registry.register_pruner("blipt5_dsnot_pruner")
class BLIPT5LayerDSnoTPruner(_DsnotPruner):
    """ViT tower, then T5 encoder, then T5 decoder (or the LLaMA/OPT stack) -- dsnot_pruner.py:1599-1878."""
    pruner_name = "blipt5_dsnot_pruner"

    def __init__(self, model, data_loader, t5_prune_spec=None, vit_prune_spec=None, t5_pruning_method=None,
                 vit_pruning_method=None, t5_model_prefix="t5_model", vit_model_prefix="visual_encoder", peft_postfix="",
                 **kwargs):
        super().__init__(model, data_loader, f"{vit_model_prefix}+{t5_model_prefix}", **dict(kwargs, prune_spec=None))
        self._set_blip_towers(t5_prune_spec, vit_prune_spec, t5_pruning_method, vit_pruning_method, t5_model_prefix,
                              vit_model_prefix, peft_postfix)

    def get_sparsity(self, t5_sparsity, vit_sparsity, sparsity_ratio_granularity=None):
        """(:1683-1757): a yaml override, else LayerSparsity at the MEAN of both sparsities (per-tower budgets
        under `prune_per_model`), with the grouping rule of the Wanda pruner's get_sparsity (:1693-1740)."""
        return uniform_or_layer_sparsity(self, 0.5 * (t5_sparsity + vit_sparsity), sparsity_ratio_granularity,
                                         prune_per_model=self.prune_per_model,
                                         per_model_group=[self.t5_model_prefix, self.vit_model_prefix],
                                         per_model_sparsity=[t5_sparsity, vit_sparsity])

    def forward_to_cache(self, model, batch, lora_model=False):
        if lora_model:
            return model(batch, vit_dense=True, llm_dense=True)                 # always dense here (:1759-1763)
        return model(batch)

    @cal.quiet_gc
    @print_time
    def prune(self, importance_scores=None, keep_indices_or_masks=None, lora_model=False):
        dtype_record, requires_grad_record, device = self.model_setup_and_record_attributes(self.model)
        global_sparsity_dict = None
        _, vit_keep_ratio, _, _ = self.convert_spec_to_list(self.vit_prune_spec)
        _, t5_keep_ratio, _, _ = self.convert_spec_to_list(self.t5_prune_spec)
        if self.sparsity_ratio_granularity not in [None, "none"]:
            global_sparsity_dict = self.get_sparsity(1 - t5_keep_ratio, 1 - vit_keep_ratio,
                                                     sparsity_ratio_granularity=self.sparsity_ratio_granularity)

        def own(keep_ratio):
            s = 1 - keep_ratio
            return lambda: global_sparsity_dict if global_sparsity_dict is not None else \
                self.get_sparsity(s, s, sparsity_ratio_granularity=None)
        self._prune_towers(lora_model,
                           vit=own(vit_keep_ratio) if self.vit_prune_spec is not None and float(vit_keep_ratio) < 1. else None,
                           llm=own(t5_keep_ratio) if self.t5_prune_spec is not None and float(t5_keep_ratio) < 1. else None)
        self.model_reset(self.model, dtype_record, requires_grad_record, device)
        return self.model, global_sparsity_dict

    def check(self, name, v, model_prefix):
        return len(v.shape) == 2 and ".block" in name and "relative_attention_bias.weight" not in name \
            and name.startswith(model_prefix)

    def trans_sparsity(self, vit_params, t5_params, vit_keep_ratio, t5_keep_ratio):
        """(:1873-1878) equalise the kept parameter budgets of the two towers."""
        vit_keep = (vit_params + t5_params) * vit_keep_ratio / 2
        t5_keep = (vit_params + t5_params) * t5_keep_ratio / 2
        return min(vit_keep / vit_params, 1.0), min(t5_keep / t5_params, 1.0)


def return_reorder_indice(input_tensor):
    """The reference's module-level helper (dsnot_pruner.py:1881-1925), same name and contract: for
    [[1., -2., 3.], [-2, 2., -4], [5., 6., -7], [-6, -7, -4]] the int64 indices [[1, 2, 0], [0, 2, 1], [2, 1, 0], [0, 1, 2]] --
    negative entries keep their relative order at the head, positive entries are flipped at the tail, an entry that is
    neither contributes a 0 between them.  One launch of `vlmc_reorder_indices` instead of two fp64 [rows, cols] index
    matrices, two sorts, a flip and a sum; GPU tensors only (no CPU fallback, like every op of this build)."""
    from vlmc import dsnot
    return dsnot.reorder_indices(input_tensor)
