"""The reference-op LLaMA stand-in (vlmc/synthetic_llama.py) against the reference itself.

1. `LlamaLayerOps`, the mask functions and `apply_rotary_pos_emb` reproduce, BIT FOR BIT on the CPU, what the reference's
   `LlamaDecoderLayer`, `_make_causal_mask`, `_expand_mask` and `apply_rotary_pos_emb` gave for the same weights and inputs
   (tests/golden/llama_ops.npz, recorded by tests/golden/make_golden_llama_ops.py): fp32, bf16 and fp16, batch 1 and a right-padded batch
   of 3, positions that are not `arange`, 16-bit masks that hold -inf before the clamp.  Same ops in the same order leave no room.
2. The drop-in Wanda / DSnoT pruners (`t5_model_prefix="llm_model"`) on the toy InstructBLIP whose language layers are the
   reference-op ones reproduce the reference's own pruners' masks and weights bit for bit on the CPU through the oracle stand-ins
   (as tests/test_vicuna_branch.py does for the old toy); on the GPU the masks agree up to near-ties."""
import pytest
import torch

import golden_io
import oracle_ops
import toy_llama_ops as TL
import toy_models
from vlmc import synthetic_llama as SL

G = golden_io.load("llama_ops")
LAYER = dict(hidden=64, heads=4, d_ff=96, layers=2, max_pos=64)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)                                               # (as oracle/sparsegpt.py: a threaded product may split its sums)
    yield
    torch.set_num_threads(n)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(_bits(got), _bits(want)), f"{what}: {int((_bits(got) != _bits(want)).sum())} of {got.numel()} entries differ"


def _layers(dt):
    torch.manual_seed(0)
    layers = torch.nn.ModuleList([SL.LlamaLayerOps(LAYER["hidden"], LAYER["d_ff"], LAYER["heads"], rms_norm_eps=1e-6,
                                                   max_position_embeddings=LAYER["max_pos"]) for _ in range(LAYER["layers"])])
    toy_models.init_toy(layers, seed=11)
    with torch.no_grad():
        for n_, p_ in layers.named_parameters():
            if p_.dim() == 1:
                p_.copy_(1.0 + 0.1 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(len(n_))))
    return layers.to(dt).eval()


@pytest.mark.parametrize("tag", list(DTYPES))
def test_masks_and_rotary_embedding_equal_the_reference(tag, one_thread):
    dt = DTYPES[tag]
    inp = {k[len("layer/in/"):]: v for k, v in G.items() if k.startswith("layer/in/")}
    cpu = torch.device("cpu")
    _same(SL.make_causal_mask((1, 7), dt, cpu).contiguous(), G[f"layer/{tag}/causal1"], "causal mask")
    _same(SL.expand_mask(inp["atts3"], dt, tgt_len=9).contiguous(), G[f"layer/{tag}/expand3"], "expanded mask")
    m1 = SL.prepare_decoder_attention_mask(torch.ones(1, 7, dtype=torch.bool), (1, 7), dt, cpu)
    m3 = SL.prepare_decoder_attention_mask(inp["atts3"], (3, 9), dt, cpu)
    _same(m1.contiguous(), G[f"layer/{tag}/mask1"], "combined mask, batch 1")
    _same(m3.contiguous(), G[f"layer/{tag}/mask3"], "combined mask, padded batch")
    if dt != torch.float32:
        assert bool(torch.isinf(m3).any())                                # min + min: what the clamp is for
    rot = SL.LlamaRotaryEmbeddingOps(LAYER["hidden"] // LAYER["heads"], max_position_embeddings=LAYER["max_pos"])
    cos, sin = rot(inp["rope_q"].to(dt), seq_len=LAYER["max_pos"])
    qe, ke = SL.apply_rotary_pos_emb(inp["rope_q"].to(dt), inp["rope_k"].to(dt), cos, sin, inp["rope_pos"])
    _same(qe.contiguous(), G[f"layer/{tag}/rope_q"], "rotated q")
    _same(ke.contiguous(), G[f"layer/{tag}/rope_k"], "rotated k")


@pytest.mark.parametrize("tag", list(DTYPES))
def test_layer_equals_the_reference_bit_for_bit(tag, one_thread):
    dt = DTYPES[tag]
    inp = {k[len("layer/in/"):]: v for k, v in G.items() if k.startswith("layer/in/")}
    layers = _layers(dt)
    with torch.no_grad():
        for name, x, mask, pos in (("1", inp["x1"], G[f"layer/{tag}/mask1"], inp["pos1"]), ("3", inp["x3"], G[f"layer/{tag}/mask3"], inp["pos3"])):
            h = x.to(dt)
            for li, layer in enumerate(layers):
                out = layer(h, attention_mask=mask, position_ids=pos)
                assert isinstance(out, tuple) and len(out) == 1
                h = out[0]
                _same(h.contiguous(), G[f"layer/{tag}/out{name}/{li}"], f"{tag}: batch {name}, layer {li}")


def test_dense_is_threaded_to_every_linear():
    """modeling_llama.py:156-160, :199-206, :250-253: `dense` reaches the seven linears when they are not plain `nn.Linear`s"""
    seen = []

    class Lin(torch.nn.Linear):
        def forward(self, x, dense=False):
            seen.append(dense)
            return super().forward(x)
    layer = SL.LlamaLayerOps(32, 48, 4, max_position_embeddings=16)
    for parent in (layer.self_attn, layer.mlp):
        for n_, c in list(parent.named_children()):
            if type(c) is torch.nn.Linear:
                new = Lin(c.in_features, c.out_features, bias=False)
                new.weight = c.weight
                setattr(parent, n_, new)
    x = torch.randn(1, 5, 32)
    mask = SL.prepare_decoder_attention_mask(torch.ones(1, 5, dtype=torch.bool), (1, 5), torch.float32, x.device)
    layer(x, attention_mask=mask, position_ids=torch.arange(5)[None], dense=True)
    assert seen == [True] * 7


def test_the_full_size_stand_in_has_the_module_names_the_pruners_address():
    m = SL.InstructBlipVicunaOps(vit_dim=32, vit_hidden=64, vit_heads=2, vit_depth=1, dim=32, d_ff=48, heads=4, depth=2, vocab=50, query_tokens=3,
                                 dtype=torch.float32, max_position_embeddings=32)
    names = dict(m.named_modules())
    for n_ in ("q_proj", "k_proj", "v_proj", "o_proj"):
        assert f"llm_model.model.layers.1.self_attn.{n_}" in names
    for n_ in ("gate_proj", "up_proj", "down_proj"):
        assert f"llm_model.model.layers.1.mlp.{n_}" in names
    g = torch.Generator().manual_seed(0)
    s = {"image": torch.randn(2, 5, 32, generator=g), "text_input": torch.randint(0, 50, (2, 4), generator=g),
         "text_output": torch.randint(0, 50, (2, 2), generator=g)}
    out = m(s)
    assert out["logits"].shape == (2, 9, 50) and torch.isfinite(out["loss"])
    s["llm_attention_mask"] = torch.tensor([[1] * 9, [1] * 6 + [0] * 3])
    out2 = m(s)
    assert torch.equal(out2["logits"][0], out["logits"][0]) and torch.equal(out2["logits"][1, :6], out["logits"][1, :6])
    assert torch.isfinite(out2["logits"]).all()


# ---- whole prunes against the reference's own ---------------------------------------------------------------------------------
def run(name, device):
    from lavis.compression import load_pruner
    pruner_name, method, _dt, _ragged, kw = TL.VARIANTS[name]
    model, batches = TL.build(name, device)
    pruned, sd = load_pruner(pruner_name, model, batches, cfg=TL.config(method, kw)).prune()
    assert sd is None
    return pruned


@pytest.mark.parametrize("name", list(TL.VARIANTS))
def test_pruners_match_the_reference_on_the_reference_op_toy_on_cpu(name, monkeypatch, one_thread):
    oracle_ops.install(monkeypatch)
    oracle_ops.install_dsnot(monkeypatch)
    pruned = run(name, "cpu")
    got = pruned.state_dict()
    n_masks = n_sd = 0
    for key, ref in G.items():
        if key.startswith(f"e2e/{name}/sd/"):
            k = key[len(f"e2e/{name}/sd/"):]
            assert got[k].dtype == ref.dtype and torch.equal(got[k].cpu(), ref), k
            n_sd += 1
        elif key.startswith(f"e2e/{name}/mask/"):
            mod = dict(pruned.named_modules())[key[len(f"e2e/{name}/mask/"):]]
            assert torch.equal(mod.mask.cpu(), ref), key
            n_masks += 1
    assert n_masks == 2 * 4 + TL.DEPTH * 7 and n_sd > n_masks               # every ViT and LLaMA-layer linear carries its mask
    assert pruned.llm_model.config.use_cache is True


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TL.VARIANTS))
def test_pruners_on_the_reference_op_toy_on_gpu(name):
    """tests/test_vicuna_branch.py::test_llm_branch_on_gpu's bound, reused: activations come from the GPU's GEMMs, so the masks agree
    with the fp32 CPU golden up to near-ties (above 0.985), and every pruned weight is exactly zero"""
    pruned = run(name, "cuda:0")
    mods = dict(pruned.named_modules())
    agree = total = 0
    for key, ref in G.items():
        if key.startswith(f"e2e/{name}/mask/"):
            m = mods[key[len(f"e2e/{name}/mask/"):]]
            same = m.mask.cpu() == ref
            agree += int(same.sum())
            total += same.numel()
            assert bool((m.weight.data[~m.mask] == 0).all())
    print(f"{name}: {agree} of {total} mask bits agree with the CPU golden = {agree / max(1, total):.4f}")
    assert total > 0 and agree / total > 0.985, agree / total
