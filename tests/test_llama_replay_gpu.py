"""GPU: the replay engine under the reference's LLaMA layer (vlmc/synthetic_llama.py: rotary embedding by `position_ids`, additive
[B, 1, T, T] mask, the clamp, fp32 softmax).

* One layer at Vicuna-7B width, fp16, 6 ragged samples: each alone == ONE padded group == two groups of 3, bit for bit on every
  real token row (modelled on tests/test_replay_invariance_gpu.py::test_block_forward_is_batch_invariant_at_model_width); every
  attention goes through the fused kernel, every rotary embedding through `vlmc_rope`, no library GEMM.  With more keys than a head's
  K and V may take of LDS the chain falls back to the unfused kernels and the equality still holds.
* Whole Wanda / DSnoT prunes of the reference-op toy, ragged text, for `VLMC_BATCH_REPLAY` = 1 / 3 / default: identical masks,
  weights and importance scores (tests/test_replay_invariance_gpu.py::test_whole_prune_is_identical_for_every_grouping, new model).
* SparseGPT on the reference-op toy tracks its CPU restatement within tests/test_sparsegpt_vicuna_gpu.py's tolerance."""
import pytest
import torch

import toy_llama_ops as TL
import toy_models

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _layer_and_samples(lengths, seed=1):
    from vlmc import synthetic, synthetic_llama as SL
    layer = SL.LlamaLayerOps(4096, 11008, 32, dtype=torch.float16).to(DEV).eval()
    synthetic.randomize_(layer, seed=3)
    g = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for norm in (layer.input_layernorm, layer.post_attention_layernorm):
            norm.weight.copy_((1.0 + 0.1 * torch.randn(4096, generator=g, device=DEV)).half())
    xs, caches = [], []
    for t in lengths:
        xs.append((torch.randn(1, t, 4096, generator=g, device=DEV) * 0.5).half())
        mask = SL.prepare_decoder_attention_mask(torch.ones(1, t, dtype=torch.bool, device=DEV), (1, t), torch.float16, torch.device(DEV))
        caches.append({"attention_mask": mask.contiguous(), "position_ids": torch.arange(t, device=DEV)[None]})
    return layer, xs, caches


def _padded(layer, xs, caches, idx):
    """samples `idx` through the layer as ONE padded group, the way calibration.walk_blocks forwards it; their own rows"""
    from vlmc import forward
    from lavis.compression.pruners import replay_padding as rp
    plan = rp.plan_padded([xs[j] for j in idx], [caches[j] for j in idx], len(idx), 128)
    assert plan is not None and len(plan) == 1, "ragged LLaMA samples must form one padded group"
    chunk, spec = plan[0]
    x = rp._pad_inputs([xs[idx[t]] for t in chunk], spec["tp"])
    kw = rp._pad_caches([caches[idx[t]] for t in chunk], spec)
    with forward.padded_rows(spec.get("rows"), spec["lengths"]):
        y = layer(x, **kw)[0]
    return [y[t:t + 1, :xs[idx[t]].shape[1]] for t in range(len(chunk))]


@pytest.mark.parametrize("lengths,fused", [([44, 176, 60, 97, 176, 52], True), ([300, 320, 77, 160, 320, 41], False)],
                         ids=["at most 176 keys", "320 keys"])
def test_llama_layer_is_batch_invariant_at_model_width(lengths, fused):
    from vlmc import forward
    from lavis.compression.pruners import calibration as cal
    layer, xs, caches = _layer_and_samples(lengths)
    n = len(xs)
    subset = cal.find_layers(layer)
    assert len(subset) == 7
    before = dict(forward.stats)
    with torch.no_grad(), forward.invariant_linears(subset.values(), roots=(layer,)):
        one = [layer(x, **c)[0] for x, c in zip(xs, caches)]
        allg = _padded(layer, xs, caches, list(range(n)))
        three = _padded(layer, xs, caches, [0, 1, 2]) + _padded(layer, xs, caches, [3, 4, 5])
    calls = n + 1 + 2                                                      # attention calls
    d = {k: forward.stats[k] - before[k] for k in forward.stats}
    print({k: v for k, v in d.items() if v})
    for j in range(n):
        assert torch.equal(allg[j], one[j]), f"sample {j}: its rows in the padded group differ from its own forward"
        assert torch.equal(three[j], one[j]), f"sample {j}: its rows in a group of three differ from its own forward"
    assert bool(torch.isfinite(torch.cat([o.flatten() for o in one]).float()).all())
    assert d["library"] == 0 and d["attn_library"] == 0 and d["kernel"] == 7 * calls
    assert d["rope_kernel"] == calls, "the rotary embedding did not run on vlmc_rope"
    assert d["kernel_rows"] == 7 * 3                                       # the padded forwards' linears skipped the padding rows
    if fused:
        assert d["attn_fused"] == calls and d["attn_fused_clamp"] == calls
        assert d["attn_chain_unfused"] == d["attn_fused_checks"] <= 2       # the one-off comparison per signature (batch 1 / a group), nothing else
        # the padded groups hand the kernel per-sample lengths -- but for the forward that is a group signature's one-off comparison
        assert d["attn_fused_lens"] == 3 - max(0, d["attn_fused_checks"] - 1) >= 2
    else:
        assert d["attn_fused"] == sum(t <= 288 for t in lengths)           # only a short sample ALONE fits the fused kernel
        assert d["attn_chain_unfused"] >= calls - d["attn_fused"] > 0       # 320 keys: the unfused, batch-invariant kernels
    assert "forward" not in layer.input_layernorm.__dict__
    import vlmc.synthetic_llama as SL
    assert not hasattr(SL.apply_rotary_pos_emb, "_vlmc_rope_orig")          # patches are gone


def test_rope_is_installed_only_where_it_reproduces_the_models_function(monkeypatch):
    """a module whose `apply_rotary_pos_emb` is another computation keeps its own ops; `VLMC_ROPE=0` installs nothing"""
    from vlmc import forward
    import vlmc.synthetic_llama as SL
    from lavis.compression.pruners import calibration as cal
    layer, xs, caches = _layer_and_samples([40, 24])
    subset = cal.find_layers(layer)
    with torch.no_grad(), forward.invariant_linears(subset.values(), roots=(layer,)):
        want = layer(xs[0], **caches[0])[0]
    orig = SL.apply_rotary_pos_emb

    def interleaved(q, k, cos, sin, position_ids):                         # (GPT-NeoX style pairs: not the reference's rotate_half)
        c, s = cos[0, 0][position_ids][:, None], sin[0, 0][position_ids][:, None]
        rot = lambda x: torch.stack((-x[..., 1::2], x[..., ::2]), -1).flatten(-2)
        return q * c + rot(q) * s, k * c + rot(k) * s
    monkeypatch.setattr(SL, "apply_rotary_pos_emb", interleaved)
    before = forward.stats["rope_kernel"]
    with torch.no_grad(), forward.invariant_linears(subset.values(), roots=(layer,)):
        assert SL.apply_rotary_pos_emb is interleaved                      # compared, refused
        other = layer(xs[0], **caches[0])[0]
    assert forward.stats["rope_kernel"] == before and not torch.equal(other, want)
    monkeypatch.setattr(SL, "apply_rotary_pos_emb", orig)
    monkeypatch.setenv("VLMC_ROPE", "0")
    with torch.no_grad(), forward.invariant_linears(subset.values(), roots=(layer,)):
        assert SL.apply_rotary_pos_emb is orig
        assert torch.equal(layer(xs[0], **caches[0])[0], want)              # the op sequence: the same bits
    assert forward.stats["rope_kernel"] == before


# ---- whole prunes ---------------------------------------------------------------------------------------------------------------
def _run_toy(method, group, monkeypatch, n_samples=8):
    from lavis.compression import load_pruner
    if group is None:
        monkeypatch.delenv("VLMC_BATCH_REPLAY", raising=False)
    else:
        monkeypatch.setenv("VLMC_BATCH_REPLAY", str(group))
    monkeypatch.setenv("VLMC_TOWER_BATCH", "0" if group == 1 else "1")     # group 1 = the reference's sample-by-sample route
    model = toy_models.init_toy(TL.ToyBlipVicunaOps(vit_dtype=torch.float16, llm_dtype=torch.float16), seed=7).eval().to(DEV)
    batches = [{k: t.to(DEV) for k, t in b.items()} for b in TL.make_batches(n_samples, True, seed0=100)]
    spec = "2-0.5-1.0-1.0"
    cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method=method, vit_pruning_method=method, num_samples=n_samples,
               max_sparsity_per_layer=1.01, t5_model_prefix="llm_model")
    if method == "dsnot":
        cfg["max_cycle_time"] = 8
    pruned, _ = load_pruner(f"blipt5_{method}_pruner", model, batches, cfg=cfg).prune()
    sd = {k: v.clone() for k, v in pruned.state_dict().items()}
    for n, m in pruned.named_modules():
        if hasattr(m, "mask") and torch.is_tensor(m.mask):
            sd[n + ".mask*"] = m.mask.clone()
        if hasattr(m, "weight") and hasattr(m.weight, "importance_score"):
            sd[n + ".importance*"] = torch.tensor(m.weight.importance_score, dtype=torch.float64)
    return sd


@pytest.mark.parametrize("method", ["wanda", "dsnot"])
def test_whole_prune_of_the_reference_op_toy_is_identical_for_every_grouping(method, monkeypatch):
    from vlmc import forward
    before = dict(forward.stats)
    ref = _run_toy(method, 1, monkeypatch)
    per_sample = {k: forward.stats[k] - before[k] for k in ("attn_fused_clamp", "rope_kernel")}
    assert any(k.endswith(".mask*") and "llm_model" in k for k in ref)
    assert method != "wanda" or any(k.endswith(".importance*") for k in ref)       # (DSnoT records no importance score)
    assert per_sample["attn_fused_clamp"] > 0 and per_sample["rope_kernel"] > 0, per_sample
    for group in (3, None):
        before = dict(forward.stats)
        got = _run_toy(method, group, monkeypatch)
        if method == "wanda":                                             # (only the Wanda statistic takes per-sample token counts: DSnoT's walk
            assert forward.stats["attn_fused_lens"] > before["attn_fused_lens"], "ragged samples were not padded into groups"   # groups equal shapes)
        assert got.keys() == ref.keys()
        bad = [k for k in ref if not torch.equal(got[k], ref[k])]
        assert not bad, f"VLMC_BATCH_REPLAY={group}: {len(bad)} tensors differ from the per-sample loop, e.g. {bad[:4]}"


@pytest.mark.parametrize("nm", [(0, 0), (2, 4)], ids=["u50", "2_4"])
def test_sparsegpt_on_the_reference_op_toy_tracks_its_cpu_restatement(nm, monkeypatch):
    """No bit-equality across groupings is asked of SparseGPT (its Hessian's sum order depends on the grouping by design): the GPU run
    against the same pruner on the CPU restatement (oracle/sparsegpt.py through tests/test_sparsegpt_vicuna.py's stand-ins), within
    tests/test_sparsegpt_vicuna_gpu.py's tolerance: pattern agreement >= 0.97, relative RMS of the weights < 2e-2 on agreeing rows."""
    import test_sparsegpt_vicuna as T
    from lavis.compression import load_pruner

    def run(device):
        model = toy_models.init_toy(TL.ToyBlipVicunaOps(), seed=5).eval().to(device)
        batches = [{k: t.to(device) for k, t in b.items()} for b in TL.make_batches(6, True)]
        cfg = dict(t5_prune_spec="2-0.5-1.0-1.0", vit_prune_spec="2-0.5-1.0-1.0", t5_pruning_method="sparsegpt", vit_pruning_method="sparsegpt",
                   num_samples=6, prune_n=nm[0], prune_m=nm[1], max_sparsity_per_layer=1.01, t5_model_prefix="llm_model")
        pruned, _ = load_pruner("blipt5_sparsegpt_pruner", model, batches, cfg=cfg).prune()
        return {n: m.weight.data.float().cpu() for n, m in pruned.named_modules()
                if isinstance(m, torch.nn.Linear) and (".layers." in n or ".blocks." in n)}
    with monkeypatch.context() as mp:
        T.install_cpu(mp)
        mp.setenv("VLMC_BATCH_REPLAY", "1")
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            want = run("cpu")
        finally:
            torch.set_num_threads(threads)
    got = run(DEV)
    assert got.keys() == want.keys() and len(got) == 2 * 4 + TL.DEPTH * 7
    agree = tot = 0
    num = den = 0.0
    for n in want:
        same = (got[n] == 0) == (want[n] == 0)
        agree += int(same.sum())
        tot += same.numel()
        rows = same.all(dim=1)
        num += float((got[n][rows] - want[n][rows]).pow(2).sum())
        den += float(want[n][rows].pow(2).sum())
        if nm[1]:
            assert bool(((got[n] == 0).view(got[n].shape[0], -1, nm[1]).sum(-1) == nm[0]).all()), n
    rel = (num / den) ** 0.5 if den else 0.0
    print(f"sparsegpt {nm}: pattern agreement {agree / tot:.5f}, relative RMS {rel:.2e}")
    assert agree / tot >= 0.97 and rel < 2e-2
