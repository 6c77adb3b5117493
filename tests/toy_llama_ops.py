"""A toy InstructBLIP-Vicuna whose language layers follow the reference's LLaMA layer op for op (vlmc/synthetic_llama.py:
rotary embedding, additive [B, 1, T, T] mask, the clamp, fp32 softmax) -- the `llm_model...model.layers` branch of the pruners on
the real op sequence.  tests/toy_models.py's ToyBlipVicuna (a stand-in rotary factor, -inf causal mask inside the attention) stays
what tests/test_vicuna_branch.py is written against.

`layer_factory` / `mask_fn`: tests/golden/make_golden_llama_ops.py builds the SAME toy around the reference's own
`LlamaDecoderLayer` and `_prepare_decoder_attention_mask` pieces (same parameter names and order: `init_toy` gives both the same
weights) and records what the reference's pruners make of it."""
import contextlib
import types

import torch
import torch.nn as nn

import toy_models
from vlmc import synthetic_llama as SL

DIM, D_FF, HEADS, DEPTH, VOCAB, MAX_POS = 32, 88, 4, 2, 50, 64


def ops_layer():
    return SL.LlamaLayerOps(DIM, D_FF, HEADS, rms_norm_eps=1e-6, max_position_embeddings=MAX_POS)


class ToyBlipVicunaOps(nn.Module):
    def __init__(self, vit_dim=32, vit_hidden=64, vit_depth=2, vit_dtype=torch.float32, llm_dtype=torch.float32, layer_factory=ops_layer,
                 mask_fn=SL.prepare_decoder_attention_mask):
        super().__init__()
        self.visual_encoder = nn.Module()
        self.visual_encoder.blocks = nn.ModuleList([toy_models.ToyViTBlock(vit_dim, vit_hidden) for _ in range(vit_depth)])
        self.visual_encoder.to(vit_dtype)
        self.llm_proj = nn.Linear(vit_dim, DIM)
        llm = nn.Module()
        llm.config = types.SimpleNamespace(use_cache=True, hidden_size=DIM)
        llm.model = nn.Module()
        llm.model.embed_tokens = nn.Embedding(VOCAB, DIM)
        llm.model.layers = nn.ModuleList([layer_factory() for _ in range(DEPTH)])
        llm.model.norm = toy_models.ToyRMSNorm(DIM)
        self.llm_model = llm
        self.llm_proj.to(llm_dtype)
        self.llm_model.to(llm_dtype)
        self.vit_dtype, self.llm_dtype, self.mask_fn = vit_dtype, llm_dtype, mask_fn

    def maybe_autocast(self, dtype=None):
        return contextlib.nullcontext()

    def forward(self, samples, vit_dense=False, llm_dense=False):
        x = samples["image"].to(self.vit_dtype)
        for blk in self.visual_encoder.blocks:
            x = blk(x, None, dense=vit_dense)
        m = self.llm_model.model
        h = torch.cat([self.llm_proj(x.to(self.llm_dtype)), m.embed_tokens(samples["text_input"]), m.embed_tokens(samples["text_output"])], dim=1)
        bsz, seq = h.shape[:2]
        pos = torch.arange(0, seq, dtype=torch.long, device=h.device).unsqueeze(0).view(-1, seq)           # modeling_llama.py:532-537
        atts = torch.ones((bsz, seq), dtype=torch.bool, device=h.device)                                   # :544-547
        mask = self.mask_fn(atts, (bsz, seq), h.dtype, h.device)
        for layer in m.layers:
            h = layer(h, attention_mask=mask, position_ids=pos, dense=llm_dense)[0]
        h = m.norm(h)
        return {"loss": h.float().pow(2).mean(), "logits": h.float() @ m.embed_tokens.weight.float().t()}


RAGGED_TXT = [5, 7, 5, 3, 7, 9, 5, 7]


def make_batches(n, ragged, seed0=300):
    """one sample per batch; ragged: four prompt lengths and three answer lengths, interleaved (9 image tokens + 3..9 + 2..4)"""
    out = []
    for j in range(n):
        ln = RAGGED_TXT[j % len(RAGGED_TXT)]
        out.append(toy_models.make_batches(1, txt_len=ln if ragged else 5, out_len=(2 + ln % 3) if ragged else 4, seed=seed0 + j)[0])
    return out


VARIANTS = {
    # name: pruner, method, language-model dtype, ragged text, extra config
    "wanda_r50": ("blipt5_wanda_pruner", "wanda", torch.float32, True, {}),
    "wanda_2_4_bf16": ("blipt5_wanda_pruner", "wanda", torch.bfloat16, True, dict(prune_n=2, prune_m=4)),
    "dsnot_r50": ("blipt5_dsnot_pruner", "dsnot", torch.float32, True, dict(max_cycle_time=12)),
}
N_SAMPLES = 6


def config(method, kw):
    spec = "2-0.5-1.0-1.0"
    return dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method=method, vit_pruning_method=method, num_samples=N_SAMPLES,
                t5_model_prefix="llm_model", max_sparsity_per_layer=1.01, **kw)


def build(name, device="cpu", **model_kw):
    _pruner, _method, llm_dtype, ragged, _kw = VARIANTS[name]
    torch.manual_seed(0)
    model = toy_models.init_toy(ToyBlipVicunaOps(llm_dtype=llm_dtype, **model_kw), seed=5).eval().to(device)
    batches = [{k: t.to(device) for k, t in b.items()} for b in make_batches(N_SAMPLES, ragged)]
    return model, batches
