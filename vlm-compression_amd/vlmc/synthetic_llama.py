"""The language model of InstructBLIP-Vicuna with the reference's OWN op sequence (lavis/models/blip2_models/modeling_llama.py),
restated: rotary position embedding gathered by `position_ids`, `matmul(q, k^T) / sqrt(d)`, the additive `[B, 1, T, T]` mask, the
clamp at the dtype's minimum, softmax in fp32, `matmul(probs, v)`, `LlamaRMSNorm`, the gated SiLU feed-forward.

`vlmc.synthetic.InstructBlipVicuna` (the default stand-in of bench.py and the tools) writes the attention as
`F.scaled_dot_product_attention(q, k, v, is_causal=True)`: no rotary embedding, no mask tensor, no clamp.  A user who binds the
pruners under the real `modeling_llama.py` runs the ops below instead; `InstructBlipVicunaOps` is the stand-in for THAT model
(same module names, same block call contract: `layer(hidden, attention_mask=, position_ids=, dense=) -> (hidden,)`), so that what
the replay engine does under it can be tested and timed without a checkpoint.

Every class cites the lines it restates; the op ORDER and every rounding point are the reference's (tests/test_llama_ops.py holds
the layer, the masks and `apply_rotary_pos_emb` against outputs recorded from the reference itself, bit for bit on the CPU).

This module imports torch and `vlmc.synthetic` only: it can be dropped next to an older tree of this package to time that tree on
the same model (tools/bench_vicuna_ops.py)."""
from __future__ import annotations

import contextlib
import math
import types

import torch
import torch.nn as nn

from vlmc.synthetic import RMSNorm, ViTBlock, _lin


# ---- masks: modeling_llama.py:41-71 (copied there from BART), combined as :470-491 -----------------------------------------------
def make_causal_mask(input_shape, dtype, device):
    """`_make_causal_mask` (modeling_llama.py:41-56) without a past: [bsz, 1, T, T], 0 on and below the diagonal, the dtype's minimum
    above it.  The reference fills with an fp32 0-dim tensor of `finfo(dtype).min` and casts afterwards: the same value."""
    bsz, tgt_len = input_shape
    mask = torch.full((tgt_len, tgt_len), torch.tensor(torch.finfo(dtype).min, device=device), device=device)
    cond = torch.arange(mask.size(-1), device=device)
    mask.masked_fill_(cond < (cond + 1).view(mask.size(-1), 1), 0)
    mask = mask.to(dtype)
    return mask[None, None, :, :].expand(bsz, 1, tgt_len, tgt_len)


def expand_mask(mask, dtype, tgt_len=None):
    """`_expand_mask` (modeling_llama.py:59-71): [bsz, src] of ones / zeros -> [bsz, 1, tgt, src], 0 where attended, the dtype's
    minimum where not."""
    bsz, src_len = mask.size()
    tgt_len = tgt_len if tgt_len is not None else src_len
    expanded = mask[:, None, None, :].expand(bsz, 1, tgt_len, src_len).to(dtype)
    inverted = 1.0 - expanded
    return inverted.masked_fill(inverted.to(torch.bool), torch.finfo(dtype).min)


def prepare_decoder_attention_mask(attention_mask, input_shape, dtype, device):
    """`LlamaModel._prepare_decoder_attention_mask` (modeling_llama.py:470-491): the causal mask PLUS the expanded padding mask.  Both
    hold the dtype's minimum and are added: a padded key that is also causally hidden carries min + min = -inf in fp16 and bf16 --
    what the clamp in the attention (:236) is for."""
    combined = None
    if input_shape[-1] > 1:
        combined = make_causal_mask(input_shape, dtype, device)
    if attention_mask is not None:
        expanded = expand_mask(attention_mask, dtype, tgt_len=input_shape[-1]).to(device)
        combined = expanded if combined is None else expanded + combined
    return combined


# ---- rotary position embedding: modeling_llama.py:94-140 ----------------------------------------------------------------------
class LlamaRotaryEmbeddingOps(nn.Module):
    """`LlamaRotaryEmbedding` (modeling_llama.py:94-123): cos / sin tables [1, 1, positions, d] built in fp32 from `inv_freq`
    (`cat(freqs, freqs)`), handed out cut to `seq_len` and cast to the activation dtype."""

    def __init__(self, dim, max_position_embeddings=2048, base=10000):
        super().__init__()
        self.dim, self.base = dim, base
        self._build(max_position_embeddings, None)

    def _build(self, positions, device):
        inv_freq = 1.0 / (self.base ** (torch.arange(0, self.dim, 2).float().to(device) / self.dim))
        self.register_buffer("inv_freq", inv_freq)
        self.max_seq_len_cached = positions
        t = torch.arange(positions, device=inv_freq.device, dtype=inv_freq.dtype)
        freqs = torch.einsum("i,j->ij", t, inv_freq)
        emb = torch.cat((freqs, freqs), dim=-1)
        self.register_buffer("cos_cached", emb.cos()[None, None, :, :], persistent=False)
        self.register_buffer("sin_cached", emb.sin()[None, None, :, :], persistent=False)

    def forward(self, x, seq_len=None):
        if seq_len > self.max_seq_len_cached:
            self._build(seq_len, x.device)
        return (self.cos_cached[:, :, :seq_len, ...].to(dtype=x.dtype), self.sin_cached[:, :, :seq_len, ...].to(dtype=x.dtype))


def rotate_half(x):
    """modeling_llama.py:126-130"""
    x1 = x[..., : x.shape[-1] // 2]
    x2 = x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def apply_rotary_pos_emb(q, k, cos, sin, position_ids):
    """modeling_llama.py:133-140.  A module-level function called by the attention class, as in the reference: the replay engine
    looks it up by this name in the module that defines the attention class, and runs `vlmc_rope` in its place where that
    reproduces it bit for bit (vlmc/forward.py)."""
    gather_indices = position_ids[:, None, :, None]                           # [bs, 1, seq_len, 1]
    gather_indices = gather_indices.repeat(1, cos.shape[1], 1, cos.shape[3])
    cos = torch.gather(cos.repeat(gather_indices.shape[0], 1, 1, 1), 2, gather_indices)
    sin = torch.gather(sin.repeat(gather_indices.shape[0], 1, 1, 1), 2, gather_indices)
    q_embed = (q * cos) + (rotate_half(q) * sin)
    k_embed = (k * cos) + (rotate_half(k) * sin)
    return q_embed, k_embed


# ---- the decoder layer: modeling_llama.py:143-327 -----------------------------------------------------------------------------
class LlamaMLPOps(nn.Module):
    """`LlamaMLP` (modeling_llama.py:143-160): `down(act(gate(x)) * up(x))`, `dense` threaded to the three linears."""

    def __init__(self, hidden_size, intermediate_size, dtype=None):
        super().__init__()
        self.gate_proj = nn.Linear(hidden_size, intermediate_size, bias=False, dtype=dtype)
        self.down_proj = nn.Linear(intermediate_size, hidden_size, bias=False, dtype=dtype)
        self.up_proj = nn.Linear(hidden_size, intermediate_size, bias=False, dtype=dtype)
        self.act_fn = nn.SiLU()                                                # ACT2FN["silu"]

    def forward(self, x, dense=False):
        return _lin(self.down_proj, self.act_fn(_lin(self.gate_proj, x, dense)) * _lin(self.up_proj, x, dense), dense)


class LlamaAttentionOps(nn.Module):
    """`LlamaAttention.forward` (modeling_llama.py:187-257) without a key / value cache."""

    def __init__(self, hidden_size, num_heads, max_position_embeddings=2048, dtype=None):
        super().__init__()
        self.hidden_size, self.num_heads = hidden_size, num_heads
        self.head_dim = hidden_size // num_heads
        if self.head_dim * num_heads != hidden_size:
            raise ValueError(f"hidden_size must be divisible by num_heads (got {hidden_size} and {num_heads})")
        self.q_proj = nn.Linear(hidden_size, hidden_size, bias=False, dtype=dtype)
        self.k_proj = nn.Linear(hidden_size, hidden_size, bias=False, dtype=dtype)
        self.v_proj = nn.Linear(hidden_size, hidden_size, bias=False, dtype=dtype)
        self.o_proj = nn.Linear(hidden_size, hidden_size, bias=False, dtype=dtype)
        self.rotary_emb = LlamaRotaryEmbeddingOps(self.head_dim, max_position_embeddings=max_position_embeddings)

    def forward(self, hidden_states, attention_mask=None, position_ids=None, dense=False):
        bsz, q_len, _ = hidden_states.size()
        query_states = _lin(self.q_proj, hidden_states, dense).view(bsz, q_len, self.num_heads, self.head_dim).transpose(1, 2)
        key_states = _lin(self.k_proj, hidden_states, dense).view(bsz, q_len, self.num_heads, self.head_dim).transpose(1, 2)
        value_states = _lin(self.v_proj, hidden_states, dense).view(bsz, q_len, self.num_heads, self.head_dim).transpose(1, 2)
        kv_seq_len = key_states.shape[-2]
        cos, sin = self.rotary_emb(value_states, seq_len=kv_seq_len)
        query_states, key_states = apply_rotary_pos_emb(query_states, key_states, cos, sin, position_ids)      # (the module's global)
        attn_weights = torch.matmul(query_states, key_states.transpose(2, 3)) / math.sqrt(self.head_dim)
        if attention_mask is not None:
            if attention_mask.size() != (bsz, 1, q_len, kv_seq_len):
                raise ValueError(f"attention_mask {tuple(attention_mask.size())}: expected {(bsz, 1, q_len, kv_seq_len)}")
            attn_weights = attn_weights + attention_mask
            attn_weights = torch.max(attn_weights, torch.tensor(torch.finfo(attn_weights.dtype).min))      # :236, a 0-dim CPU tensor
        attn_weights = nn.functional.softmax(attn_weights, dim=-1, dtype=torch.float32).to(query_states.dtype)
        attn_output = torch.matmul(attn_weights, value_states)
        attn_output = attn_output.transpose(1, 2)
        attn_output = attn_output.reshape(bsz, q_len, self.hidden_size)
        return _lin(self.o_proj, attn_output, dense)


class LlamaLayerOps(nn.Module):
    """`LlamaDecoderLayer` (modeling_llama.py:260-327): pre-norm attention and feed-forward with residuals; returns `(hidden,)`."""

    def __init__(self, hidden_size, intermediate_size, num_heads, rms_norm_eps=1e-6, max_position_embeddings=2048, dtype=None):
        super().__init__()
        self.hidden_size = hidden_size
        self.self_attn = LlamaAttentionOps(hidden_size, num_heads, max_position_embeddings, dtype=dtype)
        self.mlp = LlamaMLPOps(hidden_size, intermediate_size, dtype=dtype)
        self.input_layernorm = RMSNorm(hidden_size, eps=rms_norm_eps)          # (LlamaRMSNorm, :74-91: T5LayerNorm's op sequence)
        self.post_attention_layernorm = RMSNorm(hidden_size, eps=rms_norm_eps)
        if dtype is not None:
            self.input_layernorm.to(dtype)
            self.post_attention_layernorm.to(dtype)

    def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None, output_attentions=False,
                use_cache=False, dense=False):
        residual = hidden_states
        hidden_states = self.input_layernorm(hidden_states)
        hidden_states = self.self_attn(hidden_states, attention_mask=attention_mask, position_ids=position_ids, dense=dense)
        hidden_states = residual + hidden_states
        residual = hidden_states
        hidden_states = self.post_attention_layernorm(hidden_states)
        hidden_states = self.mlp(hidden_states, dense=dense)
        hidden_states = residual + hidden_states
        return (hidden_states,)


class InstructBlipVicunaOps(nn.Module):
    """ViT-g (fp16) + 32 reference-op LLaMA layers 4096 / 11008 (fp16): `llm_model.model.layers[i].{self_attn.*_proj, mlp.*_proj}`.
    The language model's forward follows `LlamaModel.forward` (modeling_llama.py:494-608): `position_ids = arange(T)[None]`
    ([1, T]), the mask of `_prepare_decoder_attention_mask` from an attention mask of ones (`samples["llm_attention_mask"]` [B, T]
    replaces it: right-padded batches), every layer called with both."""

    def __init__(self, vit_dim=1408, vit_hidden=6144, vit_heads=16, vit_depth=39, dim=4096, d_ff=11008, heads=32, depth=32,
                 vocab=32000, query_tokens=32, dtype=torch.float16, max_position_embeddings=2048, vit_reference_ops=False):
        super().__init__()
        self.visual_encoder = nn.Module()
        self.visual_encoder.blocks = nn.ModuleList([ViTBlock(vit_dim, vit_hidden, vit_heads, vit_reference_ops) for _ in range(vit_depth)])
        self.visual_encoder.to(dtype)
        self.llm_proj = nn.Linear(vit_dim, dim, dtype=dtype)
        llm = nn.Module()
        llm.config = types.SimpleNamespace(use_cache=True, hidden_size=dim)
        llm.model = nn.Module()
        llm.model.embed_tokens = nn.Embedding(vocab, dim, dtype=dtype)
        llm.model.layers = nn.ModuleList([LlamaLayerOps(dim, d_ff, heads, max_position_embeddings=max_position_embeddings, dtype=dtype)
                                          for _ in range(depth)])
        llm.model.norm = RMSNorm(dim).to(dtype)
        self.llm_model = llm
        self.query_tokens, self.vit_dtype, self.llm_dtype = query_tokens, dtype, dtype

    def maybe_autocast(self, dtype=None):
        return contextlib.nullcontext()

    def forward(self, samples, vit_dense=False, llm_dense=False):
        x = samples["image"].to(self.vit_dtype)
        for blk in self.visual_encoder.blocks:
            x = blk(x, None, dense=vit_dense)
        m = self.llm_model.model
        h = torch.cat([self.llm_proj(x[:, :self.query_tokens]), m.embed_tokens(samples["text_input"]),
                       m.embed_tokens(samples["text_output"])], dim=1)
        bsz, seq = h.shape[:2]
        position_ids = torch.arange(0, seq, dtype=torch.long, device=h.device).unsqueeze(0).view(-1, seq)           # :532-537
        atts = samples.get("llm_attention_mask")
        if atts is None:
            atts = torch.ones((bsz, seq), dtype=torch.bool, device=h.device)                                         # :544-547
        mask = prepare_decoder_attention_mask(atts, (bsz, seq), h.dtype, h.device)
        for layer in m.layers:
            h = layer(h, attention_mask=mask, position_ids=position_ids, dense=llm_dense)[0]
        logits = m.norm(h) @ m.embed_tokens.weight.t()
        return {"loss": logits.float().logsumexp(-1).mean(), "logits": logits}
