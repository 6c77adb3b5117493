"""SparseGPT pruners behind the reference's `lavis.compression` API: `t5_sparsegpt_pruner`,
`vit_sparsegpt_pruner`, `blipt5_sparsegpt_pruner`
(reference: lavis/compression/pruners/sparsegpt_pruner.py:222-497, :500-867, :870-1090).

Same registry names, constructor kwargs and `prune(importance_scores=None,
keep_indices_or_masks=None) -> (model, sparsity_dict | None)` contract.  Quirks kept: calibration stops by BATCH index
(`i >= n_samples`, :391-393), both towers are pruned whenever their spec is not None (no keep-ratio < 1 test,
:1021,:1044), no `module.mask` is attached (SparseGPT only rewrites the weights).  The arithmetic lives in `vlmc.sparsegpt`.
The tower step, the tower sequence, the constructor keywords and the Hessian-sharing hook rule are in `tower_walk.py`.

Beyond the reference:
* `blipt5_sparsegpt_pruner` with a `t5_model_prefix` containing "llm_model" walks
  `{prefix}{peft_postfix}.model.layers` (InstructBLIP-Vicuna), as the Wanda and DSnoT BLIP pruners do; any other non-T5
  prefix keeps the reference's OPT walk `...model.decoder.layers` (:1084).  `peft_postfix=""` is accepted.
* `prune(..., lora_model=False)`.  With True (what the RESSA driver calls, train.py:569) every linear gets the same
  Hessian, factorization and blocked OBS sweep as without, on the fp32 working copy, but the sweep's keep pattern
  (the complement of its `mask_out`) goes onto `module.mask` (bool [out, in], True = keep, the SparseLoRA buffer) and
  `module.weight` is left bit for bit as it was: the reconstruction is discarded.  RESSA's `dense=True` teacher forward
  reads that same weight tensor (lora.py `Linear.forward`), Wanda and DSnoT never write weights under `lora_model`, and
  keeping the reconstruction would need a second weight buffer (another checkpoint format).  The calibration forward is
  `model(batch, vit_dense=..., llm_dense=...)` and a tower whose keep ratio is 1 is skipped, as in the Wanda BLIP pruner
  (wanda_pruner.py:436-470); the blocks replay with the cached `dense=True`, so every block is calibrated on the dense
  model's activations.  Layer-sharded runs broadcast the mask from the linear's owner instead of the weight.
"""
from __future__ import annotations


import torch

from lavis.common.registry import registry
from lavis.compression.pruners import calibration as cal
from lavis.compression.pruners.tower_walk import (SharedHessians, TowerKind, TowerPruner, autocast_bf16, autocast_default,
                                                  input_signature)
from lavis.compression.pruners.utils import print_time
from lavis.compression.pruners.wanda_pruner import uniform_or_layer_sparsity
from vlmc import config


class _SparseGPTPruner(TowerPruner):
    """The SparseGPT tower kinds and per-block step shared by the T5/LLM, ViT and BLIP pruners."""
    # (padded groups of ragged text are opt-in; the Hessian hooks take the padded group's row map)
    llm_kind = TowerKind(vit=False, tuple_output=True, autocast=autocast_bf16,
                         pad_ragged=lambda: config.flag("VLMC_SGPT_PAD"), count_batches=True)
    vit_kind = TowerKind(vit=True, tuple_output=False, autocast=autocast_default, pad_ragged=None, count_batches=True)
    opt_walk = True

    def get_sparsity(self, original_sparsity, sparsity_ratio_granularity=None):
        return uniform_or_layer_sparsity(self, original_sparsity, sparsity_ratio_granularity)

    def _capture(self, kind, *args):
        if not kind.vit:
            print("loading calibdation data")
        return super()._capture(kind, *args)

    def _end_of_tower(self, walked):
        _flush_score_backlog(self)                       # per tower, also when it raised

    def _block_step(self, i, subset, run_pass, n_inps, batch0, *, kind, module_to_process, model_prefix, sparsity_ratio,
                    lora_model):
        """Hooks -> one dense pass -> prune every linear (sparsegpt_pruner.py:405-459).  Linears that receive the
        very same tensor (q/k/v, wi_0/wi_1, cross-attention k/v) share ONE Hessian accumulator and ONE Cholesky chain
        (`SharedHessians`).  `lora_model`: the sweeps' keep masks go onto `module.mask`, the weights stay (module docstring)."""
        from vlmc import sparsegpt
        shared = SharedHessians(subset)

        def make_hook(name):
            def hook(_m, inp, out):
                x = inp[0].data
                shared.add(name, input_signature(x), x)
            return hook

        handles = [mod.register_forward_hook(make_hook(name)) for name, mod in subset.items()]
        try:
            run_pass(lambda _j: shared.begin_forward(), outputs=False)
        finally:
            for h in handles:
                h.remove()
        wrapped, unique = shared.wrapped, shared.unique()
        from vlmc.shard import require_real_exchange
        require_real_exchange("blipt5_sparsegpt_pruner")
        shared.allreduce()
        owner = _shard_linears(subset, wrapped)
        rank = cal.calibration_shard()[0]
        mine = [name for name in subset if owner is None or owner[name] == rank]
        # the Hessians this rank prunes with: factorized together, each chain on a stream of its own, one host check for all
        sparsegpt.factorize_many(list({id(wrapped[n]): (wrapped[n].H, wrapped[n].factor_cache) for n in mine}.values()), percdamp=0.01,
                                 history=self.__dict__.setdefault("_damping_history", {}).setdefault(module_to_process, {}))
        # importance scores (:165: a Python float per linear) are queued on the pruner and read back once per tower: a host
        # copy per block made the host wait for the block's sweeps before it could issue the next block's replay
        scores = self.__dict__.setdefault("_score_backlog", [])
        by_acc = {}
        for name in mine:
            assert wrapped[name].nsamples == n_inps                                # :442
            by_acc.setdefault(id(wrapped[name]), []).append(name)
        masks = {}
        only = dict(mask_only=True) if lora_model else {}          # (the prune-only calls keep their exact arguments)

        def sweep(names):
            acc = wrapped[names[0]]
            keys = [f"{module_to_process}.{i}.{n}.weight" for n in names]
            same = len({(subset[n].weight.dtype, subset[n].weight.shape[1]) for n in names}) == 1
            if len(names) > 1 and same and "U" in acc.factor_cache and sparsegpt.stacked_sweeps_enabled():
                # linears fed the same tensor share the factor: ONE column sweep over their stacked rows
                keep = sparsegpt.fasterprune_group([subset[n] for n in names], [sparsity_ratio[k] for k in keys], acc.factor_cache,
                                                   prune_n=self.prune_n, prune_m=self.prune_m, blocksize=128, score_sink=scores, **only)
                if lora_model:
                    masks.update(zip(names, keep))
                return
            for name, key in zip(names, keys):
                keep = sparsegpt.fasterprune(subset[name], acc.H, sparsity_ratio[key], prune_n=self.prune_n, prune_m=self.prune_m,
                                             percdamp=0.01, blocksize=128, factor_cache=acc.factor_cache, score_sink=scores, **only)
                if lora_model:
                    masks[name] = keep

        # The sweeps of linears with DIFFERENT inputs are independent chains of (cols / 128) x [latency-bound sweep kernel +
        # trailing GEMM] (the reference prunes them one after the other, :430-446): each chain on a stream of its own, the
        # longest first (`VLMC_SGPT_SWEEP_STREAMS=1`: one after the other).  Same kernels on the same data: bit-identical.
        # configs[2] (2:4): 2.10 -> 1.90 s per prune.
        groups = sorted(by_acc.values(), key=lambda g: -(subset[g[0]].weight.shape[1] * sum(subset[n].weight.shape[0] for n in g)))
        dev = subset[groups[0][0]].weight.device if groups else None
        # (n:m mode only: the unstructured block threshold is agreed on through grid barriers between co-resident workgroups --
        # vlmc_sparsegpt_select_sweep -- and two such launches side by side strand each other: measured 8.6 s against 2.5 s)
        streams = sparsegpt.sweep_streams(dev) if groups and dev.type == "cuda" and len(groups) > 1 and self.prune_n != 0 else []
        if not streams:
            for names in groups:
                sweep(names)
        else:
            main = torch.cuda.current_stream(dev)
            n0 = len(scores)
            for g, names in enumerate(groups):
                st = streams[g % len(streams)]
                st.wait_stream(main)
                for t in (wrapped[names[0]].factor_cache.get("U"), wrapped[names[0]].factor_cache.get("dead")):
                    if isinstance(t, torch.Tensor):
                        t.record_stream(st)
                with torch.cuda.stream(st):
                    sweep(names)
            for st in streams:
                main.wait_stream(st)
            for name in mine:                                   # made on a side stream, used on the caller's from here on
                subset[name].weight.data.record_stream(main)
                if name in masks:
                    masks[name].record_stream(main)
            for _w, sc in scores[n0:]:
                sc.record_stream(main)
        for name, keep in masks.items():
            setattr(subset[name], "mask", keep)                 # True = keep: the SparseLoRA buffer
        if owner is not None:
            _flush_score_backlog(self)                                             # (the exchange sends the scores along)
            _exchange_pruned(subset, owner, rank, masks=lora_model)
        for acc in unique:
            acc.free()


def _flush_score_backlog(pruner):
    """`weight.importance_score` for every linear pruned since the last flush: one host copy (end of a tower, also on error)."""
    from vlmc import sparsegpt
    sparsegpt.flush_scores(pruner.__dict__.get("_score_backlog", []))


def _shard_linears(subset, wrapped):
    """Multi-GPU (BASELINE.json config 3, "layers sharded"): after the Hessian all-reduce every rank holds the same H, and
    pruning a linear is deterministic, so each linear needs to be pruned by ONE rank only.  Linears sharing an accumulator
    (one factorization) stay together; groups go to the least loaded rank, heaviest first (n^3 for the factorization +
    rows * n per sweep).  Returns {linear name: rank}, or None when running single / as replicas
    (`VLMC_SGPT_SHARD_LAYERS=0`: every rank prunes everything)."""
    rank, world = cal.calibration_shard()
    if world == 1 or not config.flag("VLMC_SGPT_SHARD_LAYERS"):
        return None
    groups = {}
    for name in subset:
        groups.setdefault(id(wrapped[name]), []).append(name)

    def cost(names):
        n = subset[names[0]].weight.shape[1]
        return n ** 3 / 3 + sum(subset[m].weight.shape[0] * n * 128.0 for m in names)
    load = [0.0] * world
    owner = {}
    for names in sorted(groups.values(), key=lambda g: (-cost(g), g[0])):
        r = min(range(world), key=lambda k: (load[k], k))
        load[r] += cost(names)
        for m in names:
            owner[m] = r
    return owner


def _exchange_pruned(subset, owner, rank, masks=False):
    """Every linear's pruned weights (and its importance score) travel from the rank that pruned it to all others;
    `masks` (lora_model): its keep mask instead of the weights, which no rank has changed."""
    import torch.distributed as dist
    names = list(subset)
    dev = subset[names[0]].weight.device
    scores = torch.zeros(len(names), dtype=torch.float64, device=dev)
    for k, name in enumerate(names):
        w = subset[name].weight
        if owner[name] == rank:
            scores[k] = float(getattr(w, "importance_score", 0.0))
        if masks:
            if owner[name] != rank:
                subset[name].mask = torch.empty(w.shape, dtype=torch.bool, device=dev)
            dist.broadcast(subset[name].mask.view(torch.uint8), src=owner[name])      # (as bytes: every backend takes them)
            continue
        data = w.data if w.data.is_contiguous() else w.data.contiguous()
        dist.broadcast(data, src=owner[name])
        if data is not w.data:
            w.data.copy_(data)
    dist.all_reduce(scores)
    for k, name in enumerate(names):
        setattr(subset[name].weight, "importance_score", float(scores[k].item()))


@registry.register_pruner("t5_sparsegpt_pruner")
class T5LayerSparseGPTPruner(_SparseGPTPruner):
    pruner_name = "t5_sparsegpt_pruner"
    tower_kind = _SparseGPTPruner.llm_kind

    def __init__(self, model, data_loader, model_prefix="t5_model", **kwargs):
        super().__init__(model, data_loader, model_prefix, **kwargs)

    def forward_to_cache(self, model, batch, lora_model=False):
        return model(batch)

    @cal.quiet_gc
    @print_time
    def prune(self, importance_scores=None, keep_indices_or_masks=None, lora_model=False):
        """Encoder, then decoder (sparsegpt_pruner.py:511-543)."""
        print("In: ", self.pruner_name)
        out = self._prune_alone(("encoder.block", "decoder.block"), lora_model)
        if self.prune_spec is not None:
            _release_factor_caches()
        return out


@registry.register_pruner("vit_sparsegpt_pruner")
class VITLayerSparseGPTPruner(_SparseGPTPruner):
    pruner_name = "vit_sparsegpt_pruner"
    tower_kind = _SparseGPTPruner.vit_kind

    def __init__(self, model, data_loader, model_prefix="visual", **kwargs):
        super().__init__(model, data_loader, model_prefix, **kwargs)

    def forward_to_cache(self, model, batch, lora_model=False):
        return model.encode_image(batch["image"])

    @cal.quiet_gc
    @print_time
    def prune(self, importance_scores=None, keep_indices_or_masks=None, lora_model=False):
        """The ViT blocks (sparsegpt_pruner.py:838-864)."""
        print("In: ", self.pruner_name)
        out = self._prune_alone(("blocks",), lora_model)
        if self.prune_spec is not None:
            _release_factor_caches()
        return out


def _release_factor_caches():
    from vlmc import sparsegpt as _sg
    _sg.release_caches()          # factorization graphs + n x n work buffers are not kept past the prune


@registry.register_pruner("blipt5_sparsegpt_pruner")
class BLIPT5LayerSparseGPTPruner(_SparseGPTPruner):
    pruner_name = "blipt5_sparsegpt_pruner"

    def __init__(self, model, data_loader, t5_prune_spec=None, vit_prune_spec=None, t5_pruning_method=None,
                 vit_pruning_method=None, t5_model_prefix="t5_model", vit_model_prefix="visual_encoder", peft_postfix="",
                 **kwargs):
        super().__init__(model, data_loader, f"{vit_model_prefix}+{t5_model_prefix}", **dict(kwargs, prune_spec=None))
        self._set_blip_towers(t5_prune_spec, vit_prune_spec, t5_pruning_method, vit_pruning_method, t5_model_prefix,
                              vit_model_prefix, peft_postfix)
        self.vit_dense = True
        self.llm_dense = True

    def forward_to_cache(self, model, batch, lora_model=False):
        if lora_model:
            return model(batch, vit_dense=self.vit_dense, llm_dense=self.llm_dense)      # (wanda_pruner.py:941-945)
        return model(batch)

    @cal.quiet_gc
    @print_time
    def prune(self, importance_scores=None, keep_indices_or_masks=None, lora_model=False):
        """Without `lora_model` the reference's rule: a tower is pruned whenever its spec is not None (:1021, :1044).  With it
        the towers and dense flags of the Wanda BLIP pruner (wanda_pruner.py:436-470) -- a tower is pruned only when its keep
        ratio is below 1, and its calibration forward is dense exactly then -- with SparseGPT's sweeps deciding every
        `module.mask`; no weight is written."""
        print("In: ", self.pruner_name)
        dtype_record, requires_grad_record, device = self.model_setup_and_record_attributes(self.model)
        grouped = self.sparsity_ratio_granularity not in [None, "none"] if lora_model else \
            self.sparsity_ratio_granularity is not None
        # (the reference reads both specs once a granularity is set: a missing one raises there)
        keep = {part: self.convert_spec_to_list(spec)[1] if spec is not None or (grouped and not lora_model) else None
                for part, spec in (("vit", self.vit_prune_spec), ("llm", self.t5_prune_spec))}
        global_sparsity_dict = None
        if grouped:
            assert keep["vit"] == keep["llm"]
            global_sparsity_dict = self.get_sparsity(1 - keep["llm"], sparsity_ratio_granularity=self.sparsity_ratio_granularity)
        pruned = {part: ratio is not None and (not lora_model or float(ratio) < 1.) for part, ratio in keep.items()}
        if lora_model:
            self.vit_dense, self.llm_dense = pruned["vit"], pruned["llm"]

        def own(part):
            return lambda: global_sparsity_dict if global_sparsity_dict is not None else self.get_sparsity(1 - keep[part], None)
        self._prune_towers(lora_model, **{part: own(part) if pruned[part] else None for part in keep})
        self.model_reset(self.model, dtype_record, requires_grad_record, device)
        _release_factor_caches()
        return self.model, global_sparsity_dict
