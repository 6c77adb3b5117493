#!/usr/bin/env python
"""Generate tests/golden/llama_ops.npz: the reference's OWN LLaMA layer and its pruners on it, recorded for
tests/test_llama_ops.py.

Part 1 -- `lavis/models/blip2_models/modeling_llama.py` itself (loaded from its file: the package around it needs `timm`, the file
only `transformers`): `_make_causal_mask`, `_expand_mask`, their sum as `_prepare_decoder_attention_mask` forms it (:470-491),
`apply_rotary_pos_emb` and two stacked `LlamaDecoderLayer`s on a toy configuration (hidden 64, 4 heads of 16, feed-forward 96) in
fp32, bf16 and fp16; batch 1 and a right-padded batch of 3 (lengths 9, 5, 7); positions that are not `arange`.  In the 16-bit dtypes
the combined mask of the padded batch holds -inf (min + min) before the clamp of :236.  Weights are not stored: they are
`toy_models.init_toy(seed)` on both sides (same parameter names, same order).

Part 2 -- the reference's `BLIPT5LayerWandaPruner` / `BLIPT5LayerDSnoTPruner` with `t5_model_prefix="llm_model"` on
tests/toy_llama_ops.py's toy InstructBLIP built around the reference's `LlamaDecoderLayer` and mask functions, ragged text: final
weights and masks per variant.

Part 3, printed and written here, not stored: how far the reference ALONE moves when its language model's activations are typed
bf16 instead of fp32 (same fp32-initialised weights, rounded) -- the bound tests/test_vicuna_branch.py::test_llm_branch_on_gpu uses
for an fp32 CPU golden against GPU statistics (mask agreement above 0.985) has to leave room for the reference's own spread on this
toy.  Observed when this fixture was generated (hidden 32, 4 heads, 2 layers, 6 ragged samples): 25066 of 25088 language-model mask
bits agree = 0.9991, inside the bound.

    python tests/golden/make_golden_llama_ops.py

No text of the reference is stored: inputs and outputs only."""
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.append(os.path.join(os.path.dirname(os.path.dirname(HERE)), "vlm-compression_amd"))    # vlmc only: `lavis` is the reference's (import_reference)
from make_golden import REF, import_reference  # noqa: E402
import golden_io  # noqa: E402
import toy_llama_ops as TL  # noqa: E402
import toy_models  # noqa: E402

# agreement of the reference with itself, fp32 against bf16-typed language-model activations, written down when the fixture was made
OBSERVED = "wanda 50 % per row, language-model masks, fp32 run against bf16 run of the reference: {agree}"

LAYER = dict(hidden=64, heads=4, d_ff=96, layers=2, max_pos=64)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def load_modeling_llama():
    spec = importlib.util.spec_from_file_location("reference_modeling_llama", REF + "/lavis/models/blip2_models/modeling_llama.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def llama_config(M, hidden, heads, d_ff, layers, max_pos):
    from transformers.models.llama.configuration_llama import LlamaConfig
    return LlamaConfig(hidden_size=hidden, intermediate_size=d_ff, num_attention_heads=heads, num_hidden_layers=layers, vocab_size=TL.VOCAB,
                       max_position_embeddings=max_pos, hidden_act="silu", rms_norm_eps=1e-6)


def layer_inputs():
    """dtype-independent inputs of part 1 (fp32; each dtype rounds them)"""
    g = torch.Generator().manual_seed(20241016)
    h = LAYER["hidden"]
    d = h // LAYER["heads"]
    return {
        "x1": torch.randn(1, 7, h, generator=g), "pos1": torch.randperm(7, generator=g)[None],        # (the layer cuts its tables to the sequence)
        "x3": torch.randn(3, 9, h, generator=g), "pos3": torch.randint(0, 9, (3, 9), generator=g),
        "rope_pos": torch.randint(0, LAYER["max_pos"], (3, 9), generator=g),
        "atts3": torch.tensor([[1] * 9, [1] * 5 + [0] * 4, [1] * 7 + [0] * 2]),
        "rope_q": torch.randn(3, LAYER["heads"], 9, d, generator=g), "rope_k": torch.randn(3, LAYER["heads"], 9, d, generator=g),
    }


def gen_layer(M, out):
    cfg = llama_config(M, **LAYER)
    inp = layer_inputs()
    for k_, t in inp.items():
        out[f"layer/in/{k_}"] = t
    model = M.LlamaModel(cfg)                                    # (for _prepare_decoder_attention_mask: a method)
    for tag, dt in DTYPES.items():
        torch.manual_seed(0)
        layers = torch.nn.ModuleList([M.LlamaDecoderLayer(cfg) for _ in range(LAYER["layers"])])
        toy_models.init_toy(layers, seed=11)
        with torch.no_grad():
            for n_, p_ in layers.named_parameters():
                if p_.dim() == 1:                                    # norm weights: not all ones (where the product is rounded must show)
                    p_.copy_(1.0 + 0.1 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(len(n_))))
        layers = layers.to(dt).eval()
        with torch.no_grad():
            out[f"layer/{tag}/causal1"] = M._make_causal_mask((1, 7), dt, torch.device("cpu")).contiguous()
            out[f"layer/{tag}/expand3"] = M._expand_mask(inp["atts3"], dt, tgt_len=9).contiguous()
            m1 = model._prepare_decoder_attention_mask(torch.ones(1, 7, dtype=torch.bool), (1, 7), torch.zeros(1, dtype=dt), 0)
            m3 = model._prepare_decoder_attention_mask(inp["atts3"], (3, 9), torch.zeros(1, dtype=dt), 0)
            out[f"layer/{tag}/mask1"], out[f"layer/{tag}/mask3"] = m1.contiguous(), m3.contiguous()
            if dt != torch.float32:
                assert torch.isinf(m3).any(), "the 16-bit mask of the padded batch must hold -inf before the clamp"
            rot = layers[0].self_attn.rotary_emb
            cos, sin = rot(inp["rope_q"].to(dt), seq_len=LAYER["max_pos"])
            qe, ke = M.apply_rotary_pos_emb(inp["rope_q"].to(dt), inp["rope_k"].to(dt), cos, sin, inp["rope_pos"])
            out[f"layer/{tag}/rope_q"], out[f"layer/{tag}/rope_k"] = qe.contiguous(), ke.contiguous()
            for name, x, mask, pos in (("1", inp["x1"], m1, inp["pos1"]), ("3", inp["x3"], m3, inp["pos3"])):
                hcur = x.to(dt)
                for li, layer in enumerate(layers):
                    hcur = layer(hcur, attention_mask=mask, position_ids=pos)[0]
                    out[f"layer/{tag}/out{name}/{li}"] = hcur.contiguous()
                assert torch.isfinite(hcur.float()).all()


def ref_toy(M, name):
    cfg = llama_config(M, TL.DIM, TL.HEADS, TL.D_FF, TL.DEPTH, TL.MAX_POS)
    holder = M.LlamaModel(llama_config(M, TL.DIM, TL.HEADS, TL.D_FF, 0, TL.MAX_POS))

    def mask_fn(atts, shape, dtype, device):
        return holder._prepare_decoder_attention_mask(atts, shape, torch.zeros(1, dtype=dtype, device=device), 0)
    return TL.build(name, layer_factory=lambda: M.LlamaDecoderLayer(cfg), mask_fn=mask_fn)


def run_reference(M, name, llm_dtype=None):
    from lavis.compression.pruners import dsnot_pruner as RD
    from lavis.compression.pruners import wanda_pruner as R
    _pruner, method, _dt, _ragged, kw = TL.VARIANTS[name]
    model, batches = ref_toy(M, name)
    if llm_dtype is not None:
        model.llm_proj.to(llm_dtype)
        model.llm_model.to(llm_dtype)
        model.llm_dtype = llm_dtype
    cls = RD.BLIPT5LayerDSnoTPruner if method == "dsnot" else R.BLIPT5LayerWandaPruner
    pruned, _ = cls(model=model, data_loader=batches, **TL.config(method, kw)).prune()
    return pruned


def masks_of(pruned):
    return {mn: mod.mask for mn, mod in pruned.named_modules() if hasattr(mod, "mask") and torch.is_tensor(mod.mask)}


def gen_e2e(M, out):
    for name in TL.VARIANTS:
        pruned = run_reference(M, name)
        for k_, t in pruned.state_dict().items():
            if "rotary_emb" not in k_:
                out[f"e2e/{name}/sd/{k_}"] = t
        for mn, mask in masks_of(pruned).items():
            out[f"e2e/{name}/mask/{mn}"] = mask
    # part 3: the reference against itself, fp32 against bf16-typed language-model activations
    a, b = masks_of(run_reference(M, "wanda_r50")), masks_of(run_reference(M, "wanda_r50", torch.bfloat16))
    same = sum(int((a[k_] == b[k_]).sum()) for k_ in a if k_.startswith("llm_model"))
    total = sum(a[k_].numel() for k_ in a if k_.startswith("llm_model"))
    print(OBSERVED.format(agree=f"{same} of {total} mask bits = {same / total:.4f}"))
    return same / total


if __name__ == "__main__":
    torch.set_num_threads(1)
    import_reference()
    M = load_modeling_llama()
    out = {}
    gen_layer(M, out)
    agree = gen_e2e(M, out)
    golden_io.save("llama_ops", out)
    size = os.path.getsize(os.path.join(HERE, "llama_ops.npz"))
    print("llama_ops.npz:", len(out), "arrays,", size, "bytes; reference fp32 against bf16 mask agreement", round(agree, 4))
