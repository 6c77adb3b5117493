"""What the layer-wise pruners (`wanda_pruner`, `dsnot_pruner`, `sparsegpt_pruner`) have in common, once:

* `input_signature` / `SharedHessians` -- how forward hooks recognise "the very same input tensor" and the SparseGPT Hessians
  that linears with the same input share (SparseGPT itself, DSnoT's `initial_method="sparsegpt"`);
* `TowerKind` and `TowerPruner._prune` -- the tower step: capture the calibration inputs of a tower's block 0, walk its
  blocks with the method's block step, the method's end-of-tower step, `config.use_cache` off meanwhile;
* `TowerPruner._prune_towers` -- the BLIP pruners' tower sequence: ViT, then T5 encoder and decoder or the one LLM stack;
* `BASE_KW` / `TowerPruner.__init__` -- the constructor keywords every registered class forwards to LayerWiseBasePruner.

The pruner modules keep what belongs to their method: the statistics, the per-block step and the reference's quirks (which
tower is pruned when, which sparsity dict it gets).
"""
from __future__ import annotations

import contextlib
from typing import Callable, NamedTuple, Optional

import torch

from lavis.compression.pruners import calibration as cal
from lavis.compression.pruners.layer_single_base_pruner import LayerWiseBasePruner
from lavis.compression.pruners.utils import print_time

BASE_KW = dict(prune_spec=None, importance_scores_cache=None, keep_indices_or_masks_cache=None, is_strct_pruning=False,
               num_samples=64, is_global=False, sparsity_ratio_granularity=None, max_sparsity_per_layer=0.8,
               score_method="obd_avg", num_data_first_stage=128, num_noise=1, sparsity_dict=None, noise_eps=1e-3,
               prune_per_model=False, prune_n=0, prune_m=0)


def input_signature(x):
    """The key under which a block's forward hooks recognise the very same tensor (q/k/v, wi_0/wi_1, the cross-attention's
    k/v).  It holds only while `x` lives: whoever stores it keeps `x` referenced."""
    return (x.data_ptr(), tuple(x.shape), tuple(x.stride()), x.dtype, x._version)


class SharedHessians:
    """SparseGPT Hessian accumulators of one block's linears; linears that receive the very same tensor have bit-identical
    Hessians and share ONE accumulator (one GEMM per hook input instead of one per linear, one Cholesky chain).  The first
    forward discovers who shares what; afterwards each distinct input is folded in once per forward, and a linear whose
    partners change between calibration samples raises."""

    def __init__(self, subset):
        self.subset = subset
        self.wrapped = {}                                  # linear name -> accumulator
        self._fed = {}                                     # input signature -> accumulator fed in this forward

    def begin_forward(self):
        self._fed.clear()

    def add(self, name, key, x):
        """The hook of linear `name` saw `x` (`key`: its signature).  A stacked replay's call counts its samples: the
        accumulator's rule.  (The hook's `out` is None where the statistics pass cut the dead tail; add_batch never reads it,
        sparsegpt_pruner.py:68-79.)"""
        from vlmc import sparsegpt
        acc = self.wrapped.get(name)
        if acc is None:                                    # first sample: discover who shares what
            acc = self._fed.get(key)
            if acc is None:
                acc = sparsegpt.SparseGPT(self.subset[name])
                cal.add_batch_rows(acc, name, x)
                self._fed[key] = acc
            self.wrapped[name] = acc
        elif self._fed.get(key) is not acc:
            if key in self._fed:
                raise RuntimeError(f"{name}: the linears sharing an input changed between calibration samples")
            cal.add_batch_rows(acc, name, x)
            self._fed[key] = acc
        acc._keep_alive = x                                # the signature holds only while `x` lives

    def unique(self):
        return list({id(a): a for a in self.wrapped.values()}.values())

    def allreduce(self):
        """Multi-GPU: every rank accumulated H over its share of the samples; the global running mean
        is the sample-weighted average.  (Not in the reference, which runs replicas.)"""
        import torch.distributed as dist
        if cal.calibration_shard()[1] == 1:
            return
        for w in self.unique():
            total = torch.tensor([float(w.nsamples)], device=w.H.device)
            w.H.mul_(w.nsamples)
            dist.all_reduce(w.H)
            dist.all_reduce(total)
            w.nsamples = int(total.item())
            w.H.div_(w.nsamples)
            if hasattr(w, "_folded"):
                w._folded = w.nsamples


class TowerKind(NamedTuple):
    """How one kind of tower (a method's ViT, a method's T5/LLM stack) is captured and walked."""
    vit: bool                                       # the ViT Catcher (inp, rel_pos_bias); else the language model's kwargs, use_cache off
    tuple_output: bool                              # the blocks return a tuple (T5/LLM), not a tensor (ViT)
    autocast: Callable                              # model -> the context its blocks are forwarded under
    pad_ragged: Optional[Callable[[], bool]]        # ragged text as one padded group?  None: the ViT, walked with the memo cache
    count_batches: bool = False                     # SparseGPT's stop rule of the capture (batch index, not sample count)


def autocast_bf16(model):
    return model.maybe_autocast(dtype=torch.bfloat16)


def autocast_default(model):
    return model.maybe_autocast()


@contextlib.contextmanager
def _use_cache_off(model, model_prefix, kind):
    """A language tower is captured and walked with `config.use_cache = False` (wanda_pruner.py:214-215, :277-278); the value
    comes back also when the tower raises."""
    if kind.vit:
        yield
        return
    cfg = getattr(model, model_prefix).config
    use_cache, cfg.use_cache = cfg.use_cache, False
    try:
        yield
    finally:
        cfg.use_cache = use_cache


class TowerPruner(LayerWiseBasePruner):
    """Base of the three methods' pruners.  A method supplies `vit_kind` / `llm_kind`, `_block_step` and, if it has one,
    `_end_of_tower`; a stand-alone tower class names its `tower_kind`."""
    opt_walk = False                    # a non-T5, non-"llm_model" prefix is walked as the reference's OPT (SparseGPT only)

    def __init__(self, model, data_loader, model_prefix, **kwargs):
        """`kwargs`: what the registered class was given; the LayerWiseBasePruner ones are forwarded, the rest ignored."""
        kw = dict(BASE_KW)
        kw.update({k: v for k, v in kwargs.items() if k in BASE_KW})
        super().__init__(model=model, data_loader=data_loader, model_prefix=model_prefix, **kw)

    def _set_blip_towers(self, t5_prune_spec, vit_prune_spec, t5_pruning_method, vit_pruning_method, t5_model_prefix,
                         vit_model_prefix, peft_postfix):
        self.t5_prune_spec = t5_prune_spec
        self.vit_prune_spec = vit_prune_spec
        self.peft_postfix = peft_postfix
        assert t5_pruning_method is not None
        assert vit_pruning_method is not None
        self.t5_model_prefix = t5_model_prefix
        self.vit_model_prefix = vit_model_prefix

    def check_sparsity(self, model, module_to_process="encoder.block"):
        layers = cal.get_module_recursive(model, module_to_process)
        zeros = total = 0
        for layer in layers:
            for mod in cal.find_layers(layer).values():
                zeros += (mod.weight.data == 0).sum().item()
                total += mod.weight.numel()
        return float(zeros) / total

    # ---- one tower ------------------------------------------------------------------------------------------------
    def _block_step(self, i, subset, run_pass, n_inps, batch0, *, kind, module_to_process, model_prefix, sparsity_ratio,
                    lora_model):
        raise NotImplementedError

    def _end_of_tower(self, walked):
        """After a tower's walk, also when it raised (`walked` False)."""

    def _capture(self, kind, model, dataloader, n_samples, module_to_process, lora_model):
        return cal.capture_block_inputs(model, dataloader, n_samples, module_to_process, self.forward_to_cache, lora_model,
                                        vit=kind.vit, model_prefix=self.model_prefix, count_batches=kind.count_batches,
                                        done_towers=getattr(self, "_done_towers", None),
                                        proxy_cache=self.__dict__.setdefault("_proxy_cache", {}))

    def prepare_calibration_input_encoder(self, model, dataloader, model_prefix, n_samples,
                                          module_to_process="encoder.block", lora_model=False):
        """The reference's public capture step of a stand-alone tower pruner: (inps, outs, caches)."""
        with _use_cache_off(model, model_prefix, self.tower_kind):
            return self._capture(self.tower_kind, model, dataloader, n_samples, module_to_process, lora_model)

    @print_time
    def _prune(self, kind, model, dataloader, model_prefix, module_to_process="encoder.block", n_samples=64,
               sparsity_ratio=0.5, lora_model=False):
        with _use_cache_off(model, model_prefix, kind):
            with torch.no_grad():
                inps, outs, caches = self._capture(kind, model, dataloader, n_samples, module_to_process, lora_model)
            # under calibration sharding every rank holds 1/world of the samples; statistics are global
            n_inps, batch0 = len(inps) * cal.calibration_shard()[1], inps[0].shape[0] if inps else 0

            def prune_block(i, layer, subset, run_pass, state):
                self._block_step(i, subset, run_pass, n_inps, batch0, kind=kind, module_to_process=module_to_process,
                                 model_prefix=model_prefix, sparsity_ratio=sparsity_ratio, lora_model=lora_model)

            # (the statistics of a padded group take per-sample token counts, the Hessians a row map: the collectors)
            how = dict(memo_cache=self.__dict__.get("_proxy_cache")) if kind.pad_ragged is None else \
                dict(pad_ragged=kind.pad_ragged())
            walked = False
            try:
                cal.walk_blocks(model, inps, outs, caches, module_to_process, n_samples, lambda: kind.autocast(model),
                                prune_block, tuple_output=kind.tuple_output, **how)
                walked = True
            finally:
                self._end_of_tower(walked)
        cal.release_tower_memory()
        return model

    def _prune_alone(self, blocks, lora_model):
        """`prune()` of a stand-alone tower pruner: the towers `{model_prefix}.{blocks[k]}` at the sparsity of `prune_spec`."""
        dtype_record, requires_grad_record, device = self.model_setup_and_record_attributes(self.model)
        if self.prune_spec is None:
            return self.model, None
        _, keep_ratio, _, _ = self.convert_spec_to_list(self.prune_spec)
        sparsity_dict = self.get_sparsity(1 - keep_ratio, sparsity_ratio_granularity=self.sparsity_ratio_granularity)
        for name in blocks:
            self.model = self._prune(self.tower_kind, self.model, self.data_loader, model_prefix=self.model_prefix,
                                     module_to_process=f"{self.model_prefix}.{name}", n_samples=self.num_samples,
                                     sparsity_ratio=sparsity_dict, lora_model=lora_model)
        self.model_reset(self.model, dtype_record, requires_grad_record, device)
        return self.model, sparsity_dict

    # ---- the towers of a BLIP model -------------------------------------------------------------------------------
    def _blip_towers(self):
        """[(part, kind, model prefix, module_to_process)] in pruning order, part "vit" or "llm": the ViT; then T5's encoder
        and decoder, or the one stack of an LLM at `{prefix}{peft_postfix}.model.layers` (InstructBLIP-Vicuna's LLaMA,
        wanda_pruner.py:1031-1038), or -- `opt_walk` -- the reference SparseGPT pruner's OPT walk (sparsegpt_pruner.py:1084)."""
        vit, t5 = self.vit_model_prefix, self.t5_model_prefix
        if "t5_model" in t5:
            language = [f"{t5}.encoder.block", f"{t5}.decoder.block"]
        elif self.opt_walk and "llm_model" not in t5:
            language = [f"{t5}.model.decoder.layers"]
        else:
            language = [f"{t5}{self.peft_postfix}.model.layers"]
        return [("vit", self.vit_kind, vit, f"{vit}.blocks")] + [("llm", self.llm_kind, t5, m) for m in language]

    def _prune_towers(self, lora_model, **sparsity):
        """Prune the towers of a BLIP model in order.  `sparsity`: for `vit` and `llm` None to leave that part of the model
        alone, else a function that gives its sparsity dict (asked when the part's first tower is up).  The finished towers
        are listed in `_done_towers` (their blocks may replay from HIP graphs while the next tower's inputs are captured),
        and the capture of the last one is told that nothing is captured after it (what a capture phase records for the
        NEXT tower is not recorded)."""
        towers = [t for t in self._blip_towers() if sparsity[t[0]] is not None]
        dicts = {}
        for k, (part, kind, model_prefix, module_to_process) in enumerate(towers):
            if part not in dicts:
                dicts[part] = sparsity[part]()
            if k == len(towers) - 1:
                self.__dict__.setdefault("_proxy_cache", {})[("last_tower",)] = module_to_process
            self.model = self._prune(kind, self.model, self.data_loader, model_prefix=model_prefix,
                                     module_to_process=module_to_process, n_samples=self.num_samples,
                                     sparsity_ratio=dicts[part], lora_model=lora_model)
            self._done_towers = getattr(self, "_done_towers", []) + [module_to_process]
