#!/usr/bin/env python
"""Generate tests/golden/dsnot_sgpt.npz: the reference's `blipt5_dsnot_pruner` with `initial_method="sparsegpt"` on the toy
models of tests/toy_models.py (ToyBlipT5 with an fp32 and a bf16 T5, ToyBlipVicuna through `t5_model_prefix="llm_model"`).

The reference cannot run this option as it stands: `_prune` builds `WrappedGPT(subset[name])` without `initial_method`
(lavis/compression/pruners/dsnot_pruner.py:340, ViT :1073), so `H` is never allocated, and `add_batch` (:79-101) would not
accumulate it anyway.  This generator changes the reference in exactly ONE place: `dsnot_pruner.WrappedGPT` is replaced by
`SparseGPTInitWrappedGPT` below, which is given `initial_method="sparsegpt"` (so it allocates `H`, :65-66) and, in front of
the reference's own `add_batch`, accumulates `H` by SparseGPT's recurrence (sparsegpt_pruner.py:68-79):
`H *= n/(n+b); n += b; x = sqrt(2/n) * x.float(); H += x^T x`.  Everything else -- the damp, the three factorizations, the
metric `W**2 / diag(Hinv)`, the initial masks and the cycles (:380-751) -- is the reference's code as it is.

Stored per variant and pruned linear `<variant>/lin/<module name>/`: `H_triu` (the upper triangle, row by row, of H as
the pruner found it, before :384 touched it; it is exactly symmetric), `divU` (diag of the upper factor, from the reference's statements on that H; dead columns are where diag(H) == 0),
`stats` = [scaler_row, sum_metric_row, var] (the DSnoT statistics), `mask`, `Wn_kept` (the final weights at the kept positions, in row-major
order; every other entry is 0; not under lora_model=True, where the weights stay as they were).
Linears fed the same tensor store these once, the others `shares` = that linear's name; the inputs `xs` are stored where a
column is dead.  The weights before pruning are those of the seeded toy models (`toy_weight`; the LoRA variant's merge its
adapters into them, as tests/pruner_helpers.py:wrap_lora rebuilds them).

    python tests/golden/make_golden_dsnot_sgpt.py
"""
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _wrap_lora_reference, import_reference  # noqa: E402
import golden_io  # noqa: E402
import toy_models  # noqa: E402


def _stand_in(R, record):
    class SparseGPTInitWrappedGPT(R.WrappedGPT):
        """The reference's WrappedGPT given initial_method="sparsegpt", accumulating H as sparsegpt_pruner.py:68-79."""

        def __init__(self, layer, initial_method="sparsegpt", layer_id=0, layer_name="none"):
            super().__init__(layer, initial_method=initial_method, layer_id=layer_id, layer_name=layer_name)
            self.h_samples = 0
            self.inputs = []
            record.append(self)

        def add_batch(self, inp, out):
            x = inp.unsqueeze(0) if len(inp.shape) == 2 else inp
            self.inputs.append(x.detach().clone())
            tmp = x.shape[0]
            xt = x.reshape((-1, x.shape[-1])).t()
            self.H *= self.h_samples / (self.h_samples + tmp)
            self.h_samples += tmp
            xt = (2 / self.h_samples) ** 0.5 * xt.float()
            self.H += xt.matmul(xt.t())
            self.H_seen = self.H.clone()                       # the pruner modifies H in place (:384, :392)
            super().add_batch(inp, out)

    return SparseGPTInitWrappedGPT


def ref_divisor(H):
    """diag(Hinv) by the reference's statements :382-398 (torch CPU, as the pruner ran them)."""
    H = H.clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    damp = 0.01 * torch.mean(torch.diag(H))
    diag = torch.arange(H.shape[0])
    H[diag, diag] += damp
    H = torch.linalg.cholesky(H)
    H = torch.cholesky_inverse(H)
    H = torch.linalg.cholesky(H, upper=True)
    return torch.diag(H).clone(), dead


VARIANTS = {
    "t5bf16_2_4": dict(model="t5", dtype=torch.bfloat16, ratio=0.5, n=2, m=4, lora=False, kw=dict(max_cycle_time=4)),
    "t5fp32_u40_lora": dict(model="t5", dtype=torch.float32, ratio=0.4, n=0, m=0, lora=True,
                            kw=dict(max_cycle_time=16, update_threshold=0.02)),
    "t5fp32_u50_dead": dict(model="t5", dtype=torch.float32, ratio=0.5, n=0, m=0, lora=False, dead=True, kw=dict(max_cycle_time=20)),
    "vicuna_u50": dict(model="vicuna", dtype=torch.float32, ratio=0.5, n=0, m=0, lora=False, kw=dict(max_cycle_time=12)),
}


def build_model(v):
    if v["model"] == "t5":
        model = toy_models.init_toy(toy_models.ToyBlipT5(vit_dtype=torch.float32, t5_dtype=v["dtype"]), seed=7)
        batches = toy_models.make_batches(6, seed=11)
    else:
        torch.manual_seed(0)
        model = toy_models.init_toy(toy_models.ToyBlipVicuna(llm_dtype=v["dtype"]), seed=5)
        batches = toy_models.make_batches(6, seed=13)
    if v.get("dead"):
        # channel 3 of the first ViT block's attention input is 0 for every token: a dead column of qkv's Hessian
        norm = model.visual_encoder.blocks[0].norm1
        norm.weight.data[3] = 0
        norm.bias.data[3] = 0
    if v["lora"]:
        _wrap_lora_reference(model)
    return model.eval(), batches


def toy_weight(variant, module_name):
    """The weight a linear had before pruning (the toy models are seeded: nothing to store)."""
    model, _ = build_model(dict(VARIANTS[variant], lora=False))
    return dict(model.named_modules())[module_name.replace(".base_layer", "")].weight.data


def gen():
    from lavis.compression.pruners import dsnot_pruner as RD
    out = {}
    for name, v in VARIANTS.items():
        record = []
        RD.WrappedGPT = _stand_in(RD, record)
        model, batches = build_model(v)
        names = {id(mod): mn for mn, mod in model.named_modules()}
        W0 = {mn: mod.weight.data.clone() for mn, mod in model.named_modules() if hasattr(mod, "weight") and mod.weight is not None}
        spec = "2-%r-1.0-1.0" % (1 - v["ratio"])
        kw = dict(t5_model_prefix="llm_model") if v["model"] == "vicuna" else {}
        pr = RD.BLIPT5LayerDSnoTPruner(model=model, data_loader=batches, t5_prune_spec=spec, vit_prune_spec=spec,
                                       t5_pruning_method="dsnot", vit_pruning_method="dsnot", num_samples=6,
                                       prune_n=v["n"], prune_m=v["m"], max_sparsity_per_layer=1.01, initial_method="sparsegpt",
                                       **kw, **v["kw"])
        pruned, _ = pr.prune(lora_model=True) if v["lora"] else pr.prune()
        first = []                                                # (hook inputs, module name) of each distinct input
        for w in record:
            mn = names[id(w.layer)]
            p = f"{name}/lin/{mn}"
            xs = torch.cat(w.inputs)
            twin = next((n_ for x_, n_ in first if x_.shape == xs.shape and torch.equal(x_, xs)), None)
            if twin is None:                                      # linears fed the same tensor share H, divU and statistics
                first.append((xs, mn))
                div, dead = ref_divisor(w.H_seen)
                iu = torch.triu_indices(*w.H_seen.shape)
                assert torch.equal(w.H_seen, w.H_seen.t())                # stored as its upper triangle (golden_hessian)
                out.update({f"{p}/H_triu": w.H_seen[iu[0], iu[1]], f"{p}/divU": div,
                            f"{p}/stats": torch.stack([w.scaler_row, w.sum_metric_row, w.var.flatten()])})
                if bool(dead.any()):
                    out[f"{p}/xs"] = xs
            else:
                out[f"{p}/shares"] = twin
            out[f"{p}/mask"] = w.layer.mask.clone()
            if not v["lora"]:
                assert torch.equal(W0[mn], toy_weight(name, mn))
                Wn = w.layer.weight.data
                assert torch.equal(Wn, torch.where(w.layer.mask, W0[mn], torch.zeros_like(W0[mn])))
                out[f"{p}/Wn_kept"] = Wn[w.layer.mask]                # the final weights' kept entries (the rest are 0)
            else:
                assert torch.equal(w.layer.weight.data, W0[mn])       # lora_model=True: the weights are not touched
        out[f"{name}/ratio"] = v["ratio"]
        out[f"{name}/n"] = v["n"]
        out[f"{name}/m"] = v["m"]
        out[f"{name}/lora"] = int(v["lora"])
        for k_, val in v["kw"].items():
            out[f"{name}/kw/{k_}"] = val
    golden_io.save("dsnot_sgpt", out)
    print("dsnot_sgpt.npz:", len(out), "arrays")


if __name__ == "__main__":
    import_reference()
    torch.set_num_threads(1)
    gen()
