#!/usr/bin/env python
"""Generate tests/golden/sparsegpt_vicuna.npz: SparseGPT on the toy InstructBLIP-Vicuna of tests/toy_models.py (ToyBlipVicuna:
the ViT blocks, then the LLaMA layers at `llm_model.model.layers`), by the prune-only route and by the `lora_model` route.

The reference's `blipt5_sparsegpt_pruner` cannot run this model: its LLM branch walks `llm_model.model.decoder.layers` (the OPT
layout, lavis/compression/pruners/sparsegpt_pruner.py:1080-1086) and its `prune` has no `lora_model`.  So this generator restates
the pruner's block loop (:405-459: the inputs of the first block are captured, then per block hooks -> one pass over the samples
feeding `add_batch` -> `fasterprune` per linear -> the block re-run for the next block's inputs) and drives the reference's own
`SparseGPT` helper (:53-219) for every Hessian and every prune.  The restated loop is checked against the reference's own
`VITLayerSparseGPTPruner._prune` on the ViT tower (the one tower the reference can prune here) before anything is stored.

Routes:
* prune: `fasterprune`'s weights stay in the model; each block is calibrated on the pruned blocks before it (:455-459).
* lora: every block linear is the reference's SparseLoRA `Linear` (lora.py); the capture forward is
  `model(batch, vit_dense=True, llm_dense=True)` and caches `dense=True` for the block calls (wanda_pruner.py:238-253, :941-945),
  so each block is calibrated on the dense model's activations; after `fasterprune` the weight is put back as it was and
  `mask` = the complement of the pruned set.

The pruned set is recorded from the sweep's own decision, not read back from zeros: `q[mask1[:, i]] = 0` (:197) is the only
assignment of the sweep indexed by a 1-D bool tensor, so a TorchFunctionMode sees every column's `mask1[:, i]` in column order.

Stored per variant `<route>_<pattern>` and pruned linear `<variant>/lin/<module name>/`: `pruned` (bool [out, in]), `imp` (the
importance score, :165) and, on the prune route, `Wn_kept` (the final weights where not pruned, row-major; every pruned entry is
0).  The weights before pruning are those of the seeded toy model (nothing to store).

    python tests/golden/make_golden_sparsegpt_vicuna.py
"""
import os
import sys

import torch
import torch.nn as nn
from torch.overrides import TorchFunctionMode

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import golden_io  # noqa: E402
import toy_models  # noqa: E402

N_SAMPLES = 6
VARIANTS = {
    "prune_u50": dict(lora=False, ratio=0.5, n=0, m=0),
    "prune_2_4": dict(lora=False, ratio=0.5, n=2, m=4),
    "lora_u50": dict(lora=True, ratio=0.5, n=0, m=0),
    "lora_2_4": dict(lora=True, ratio=0.5, n=2, m=4),
}
TOWERS = (("visual_encoder.blocks", True), ("llm_model.model.layers", False))
LLM_KEYS = ["attention_mask", "position_ids"]                  # the llm_model catcher's keys (wanda_pruner.py:233-236)


def build_model():
    torch.manual_seed(0)
    model = toy_models.init_toy(toy_models.ToyBlipVicuna(), seed=5)
    return model.eval(), toy_models.make_batches(N_SAMPLES, seed=13)


def wrap_block_linears(model, linear_cls, r=4, alpha=16):
    """Every linear inside a ViT block or a LLaMA layer becomes a SparseLoRA Linear sharing the weight (what get_peft_model does
    for the targets q/k/v/o/gate/up/down and qkv/proj/fc1/fc2); `llm_proj` stays a plain linear."""
    g = torch.Generator().manual_seed(4242)
    for tower, _vit in TOWERS:
        for parent in [m for blk in get_module(model, tower) for m in blk.modules()]:
            for cname, child in list(parent.named_children()):
                if type(child) is nn.Linear:
                    new = linear_cls(child.in_features, child.out_features, r=r, lora_alpha=alpha, bias=child.bias is not None)
                    new.weight = child.weight
                    if child.bias is not None:
                        new.bias = child.bias
                    new.mask = torch.ones_like(child.weight.data).bool()
                    with torch.no_grad():
                        new.lora_A.weight.copy_(torch.randn(new.lora_A.weight.shape, generator=g) * 0.05)
                        new.lora_B.weight.copy_(torch.randn(new.lora_B.weight.shape, generator=g) * 0.05)
                    setattr(parent, cname, new)
    return model


def get_module(model, path):
    for part in path.split("."):
        model = getattr(model, part)
    return model


def find_linears(module, name=""):
    """{name: module} of the linears of a block: nn.Linear and the SparseLoRA Linear (not its lora_A / lora_B)."""
    if isinstance(module, nn.Linear):
        return {name: module}
    out = {}
    for cname, child in module.named_children():
        out.update(find_linears(child, f"{name}.{cname}" if name else cname))
    return out


class _Stop(Exception):
    pass


def capture(model, batches, tower, vit, lora):
    """(inps, caches) of block 0 of `tower` for the first N_SAMPLES batches (:380-395 / ViT :595-608)."""
    layers = get_module(model, tower)
    inps, caches = [], []

    class Catcher(nn.Module):
        def __init__(self, module):
            super().__init__()
            self.module = module

        def forward(self, inp, *args, dense=True, **kwargs):
            inps.append(inp)
            cache = {"rel_pos_bias": args[0] if args else kwargs.get("rel_pos_bias")} if vit else {k: kwargs[k] for k in LLM_KEYS}
            if lora:
                cache["dense"] = dense
            caches.append(cache)
            raise _Stop

    layers[0] = Catcher(layers[0])
    try:
        for i, batch in enumerate(batches):
            if i >= N_SAMPLES:
                break
            try:
                model(batch, vit_dense=True, llm_dense=True) if lora else model(batch)
            except _Stop:
                pass
    finally:
        layers[0] = layers[0].module
    return inps, caches


class PrunedColumns(TorchFunctionMode):
    """Records the index of every `q[mask1[:, i]] = 0` (:197): one bool row-vector per swept column, in column order."""

    def __init__(self):
        super().__init__()
        self.cols = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if func is torch.Tensor.__setitem__ and isinstance(args[1], torch.Tensor) and args[1].dtype == torch.bool \
                and args[1].dim() == 1:
            self.cols.append(args[1].clone())
        return func(*args, **(kwargs or {}))


def block_output(layer, inp, cache, vit):
    out = layer(inp, **cache)
    return out if vit else out[0]


def restated_tower(R, model, batches, tower, vit, v, record):
    """The block loop of sparsegpt_pruner.py:405-459 over `tower`, with the reference's SparseGPT helper."""
    inps, caches = capture(model, batches, tower, vit, v["lora"])
    layers = get_module(model, tower)
    for i, layer in enumerate(layers):
        subset = find_linears(layer)
        wrapped = {name: R.SparseGPT(subset[name]) for name in subset}
        handles = [subset[name].register_forward_hook(
            (lambda nm: lambda _m, inp, out: wrapped[nm].add_batch(inp[0].data, out.data))(name)) for name in subset]
        with torch.no_grad():
            for j in range(len(inps)):
                block_output(layer, inps[j], caches[j], vit)
        for h in handles:
            h.remove()
        for name in subset:
            lin = subset[name]
            assert wrapped[name].nsamples == len(inps)
            W0 = lin.weight.data.clone()
            with PrunedColumns() as rec:
                wrapped[name].fasterprune(v["ratio"], prune_n=v["n"], prune_m=v["m"], percdamp=0.01, blocksize=128)
            pruned = torch.stack(rec.cols, dim=1)
            assert pruned.shape == W0.shape
            Wn = lin.weight.data.clone()
            assert bool((Wn[pruned] == 0).all())
            if v["lora"]:
                lin.weight.data = W0                                  # the weight stays; the mask carries the decision
                lin.mask = ~pruned
            wrapped[name].free()
            record[f"{tower}.{i}.{name}"] = (pruned, Wn, float(lin.weight.importance_score))
        with torch.no_grad():
            outs = [block_output(layer, inps[j], caches[j], vit) for j in range(len(inps))]
        inps = outs


def check_restated_loop_against_the_reference(R, v):
    """The reference's own ViT tower prune (the BLIP pruner without an LLM spec) equals the restated loop bit for bit."""
    model, batches = build_model()
    spec = "2-%r-1.0-1.0" % (1 - v["ratio"])
    pr = R.BLIPT5LayerSparseGPTPruner(model=model, data_loader=batches, t5_prune_spec=None, vit_prune_spec=spec,
                                      t5_pruning_method="sparsegpt", vit_pruning_method="sparsegpt", num_samples=N_SAMPLES,
                                      prune_n=v["n"], prune_m=v["m"], max_sparsity_per_layer=1.01, t5_model_prefix="llm_model")
    ref, _ = pr.prune()
    mine, batches = build_model()
    restated_tower(R, mine, batches, "visual_encoder.blocks", True, v, {})
    for (ka, va), (kb, vb) in zip(ref.state_dict().items(), mine.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


def gen():
    from lavis.compression.pruners import sparsegpt_pruner as R
    from lavis.peft.src.peft.tuners.lora import Linear as RefLoraLinear
    out = {}
    for name, v in VARIANTS.items():
        if not v["lora"]:
            check_restated_loop_against_the_reference(R, v)
        model, batches = build_model()
        if v["lora"]:
            wrap_block_linears(model, RefLoraLinear)
        W0 = {mn: mod.weight.data.clone() for mn, mod in model.named_modules() if isinstance(mod, nn.Linear)}
        record = {}
        for tower, vit in TOWERS:
            restated_tower(R, model, batches, tower, vit, v, record)
        for mn, (pruned, Wn, imp) in record.items():
            p = f"{name}/lin/{mn}"
            out[f"{p}/pruned"] = pruned
            out[f"{p}/imp"] = imp
            if v["lora"]:
                assert torch.equal(dict(model.named_modules())[mn].weight.data, W0[mn])
            else:
                out[f"{p}/Wn_kept"] = Wn[~pruned]
        for k_, val in v.items():
            out[f"{name}/{k_}"] = int(val) if isinstance(val, bool) else val
    golden_io.save("sparsegpt_vicuna", out)
    print("sparsegpt_vicuna.npz:", len(out), "arrays")


if __name__ == "__main__":
    import_reference()
    torch.set_num_threads(1)
    gen()
