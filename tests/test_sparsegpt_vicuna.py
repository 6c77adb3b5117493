"""SparseGPT pruners on InstructBLIP-Vicuna (`t5_model_prefix="llm_model"`) and under `prune(lora_model=True)`, on the CPU:
the golden (tests/golden/sparsegpt_vicuna.npz, from tests/golden/make_golden_sparsegpt_vicuna.py: the reference's SparseGPT
helper through the restated block loop) against a CPU restatement and against the drop-in pruners with CPU stand-ins for the
kernels, layer- and sample-sharded worlds of two (gloo), and what is refused without a GPU.  The GPU side is in
tests/test_sparsegpt_vicuna_gpu.py."""
import ctypes
import importlib.util
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import golden_io
import toy_models
from oracle import sparsegpt as OS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANTS = ("prune_u50", "prune_2_4", "lora_u50", "lora_2_4")
LLAMA_TARGETS = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
VIT_TARGETS = [".qkv", ".proj", ".fc1", ".fc2"]
_G = {}


def golden():
    if not _G:
        _G.update(golden_io.load("sparsegpt_vicuna"))
    return _G


def linears(name):
    pre = f"{name}/lin/"
    return sorted({k[len(pre):].rsplit("/", 1)[0] for k in golden() if k.startswith(pre)})


# ---- the model -------------------------------------------------------------------------------------------------------------
class PeftToyBlipVicuna(toy_models.ToyBlipVicuna):
    """ToyBlipVicuna whose language model may sit inside a PEFT wrapper, as InstructBLIP-Vicuna's does under RESSA
    (train.py:413-486): the forward reaches the LLaMA stack through `get_base_model()`.  Same parameters, same forward."""

    def forward(self, samples, vit_dense=False, llm_dense=False):
        x = samples["image"].to(self.vit_dtype)
        for blk in self.visual_encoder.blocks:
            x = blk(x, None, dense=vit_dense)
        llm = self.llm_model.get_base_model() if hasattr(self.llm_model, "get_base_model") else self.llm_model
        m = llm.model
        img = self.llm_proj(x.to(self.llm_dtype))
        h = torch.cat([img, m.embed_tokens(samples["text_input"]), m.embed_tokens(samples["text_output"])], dim=1)
        pos = torch.arange(h.shape[1], device=h.device)[None].expand(h.shape[0], -1)
        for layer in m.layers:
            h = layer(h, attention_mask=None, position_ids=pos, dense=llm_dense)[0]
        h = m.norm(h)
        logits = h.float() @ m.embed_tokens.weight.float().t()
        return {"loss": h.float().pow(2).mean(), "logits": logits}


def build_model(lora, device="cpu", dtype=torch.float32):
    """The golden's model (make_golden_sparsegpt_vicuna.build_model); `lora`: both towers through get_peft_model, the language
    model's layers then at `llm_model.base_model.model.model.layers` (peft_postfix=".base_model.model")."""
    torch.manual_seed(0)
    model = toy_models.init_toy(PeftToyBlipVicuna(llm_dtype=dtype), seed=5)
    batches = toy_models.make_batches(6, seed=13)
    if lora:
        from lavis.peft.src.peft import LoraConfig, get_peft_model
        model.llm_model = get_peft_model(model.llm_model, LoraConfig(r=4, lora_alpha=16, target_modules=LLAMA_TARGETS,
                                                                     lora_dropout=0.0, bias="none", task_type="CAUSAL_LM"))
        model.visual_encoder = get_peft_model(model.visual_encoder, LoraConfig(r=2, lora_alpha=16, target_modules=VIT_TARGETS,
                                                                               lora_dropout=0.0, bias="none", task_type="ViT"))
    model.eval().to(device)
    return model, [{k: t.to(device) for k, t in b.items()} for b in batches]


def golden_name(mn):
    """A pruned linear's name in the golden (the un-wrapped model's)."""
    return mn.replace(".base_model.model", "")


def run_pruner(name, device="cpu", dtype=torch.float32, prefix="llm_model", **extra):
    from lavis.compression import load_pruner
    G = golden()
    lora = bool(G[f"{name}/lora"])
    model, batches = build_model(lora, device, dtype)
    cfg = dict(t5_prune_spec="2-0.5-1.0-1.0", vit_prune_spec="2-0.5-1.0-1.0", t5_pruning_method="sparsegpt",
               vit_pruning_method="sparsegpt", num_samples=6, prune_n=int(G[f"{name}/n"]), prune_m=int(G[f"{name}/m"]),
               max_sparsity_per_layer=1.01, t5_model_prefix=prefix, **extra)
    if lora:
        cfg["peft_postfix"] = ".base_model.model"
    weights0 = {golden_name(mn): mod.weight.data.clone() for mn, mod in model.named_modules()
                if isinstance(getattr(mod, "weight", None), torch.Tensor)}
    pruner = load_pruner("blipt5_sparsegpt_pruner", model, batches, cfg=cfg)
    pruned, sd = pruner.prune(lora_model=True) if lora else pruner.prune()
    assert sd is None
    return {golden_name(mn): mod for mn, mod in pruned.named_modules()}, weights0


def expected_weight(name, mn, W0):
    G = golden()
    pruned = G[f"{name}/lin/{mn}/pruned"]
    if G[f"{name}/lora"]:
        return W0
    W = torch.zeros(W0.shape, dtype=torch.float32)
    W[~pruned] = G[f"{name}/lin/{mn}/Wn_kept"]
    return W.to(W0.dtype)


# ---- CPU stand-ins for the kernels --------------------------------------------------------------------------------------------
def cpu_fasterprune(layer, H, sparsity, prune_n=0, prune_m=0, blocksize=128, percdamp=0.01, return_mask=False, factor_cache=None,
                    score_sink=None, mask_only=False):
    """vlmc.sparsegpt.fasterprune on the oracle (the reference's statements): `mask_only` leaves the weight and returns ~pruned."""
    Wn, imp, pruned = OS.prune(layer.weight.data, H.clone(), sparsity, prune_n, prune_m, blocksize, percdamp)
    setattr(layer.weight, "importance_score", imp)
    if mask_only:
        return ~pruned
    layer.weight.data = Wn
    return pruned if return_mask else None


def install_cpu(mp_):
    import oracle_ops
    from vlmc import sparsegpt
    oracle_ops.install_sparsegpt(mp_)
    mp_.setattr(sparsegpt, "fasterprune", cpu_fasterprune)


def check_against_golden(name, mods, weights0, exact=True):
    """(zero / mask pattern agreement, relative RMS of the weights on the rows whose pattern agrees) over every pruned linear."""
    G = golden()
    lora = bool(G[f"{name}/lora"])
    agree = tot = 0
    num = den = 0.0
    for mn in linears(name):
        mod = mods[mn]
        ref_pruned = G[f"{name}/lin/{mn}/pruned"]
        if lora:
            assert torch.equal(mod.weight.data.cpu(), weights0[mn].cpu()), mn             # not one bit of the weight changed
            got_pruned = ~mod.mask.cpu()
        else:
            got_pruned = mod.weight.data.cpu() == 0
        same = got_pruned == ref_pruned
        agree += int(same.sum())
        tot += same.numel()
        if not lora:
            ref = expected_weight(name, mn, weights0[mn].cpu()).float()
            g = mod.weight.data.cpu().float()
            rows = same.all(dim=1)
            num += float((g[rows] - ref[rows]).pow(2).sum())
            den += float(ref[rows].pow(2).sum())
            if exact:
                assert torch.equal(mod.weight.data.cpu(), expected_weight(name, mn, weights0[mn].cpu())), mn
                assert mod.weight.importance_score == pytest.approx(float(G[f"{name}/lin/{mn}/imp"]), rel=1e-6), mn
        if exact:
            assert torch.equal(got_pruned, ref_pruned), mn
    return agree / tot, (num / den) ** 0.5 if den else 0.0


# ---- the golden ------------------------------------------------------------------------------------------------------------
def test_golden_covers_both_towers_both_routes_and_both_patterns():
    G = golden()
    for name in VARIANTS:
        names = linears(name)
        assert len(names) == 2 * 4 + 3 * 7, name
        assert sum(n.startswith("llm_model.model.layers.") for n in names) == 21
        frac = sum(int(G[f"{name}/lin/{n}/pruned"].sum()) for n in names) / sum(G[f"{name}/lin/{n}/pruned"].numel() for n in names)
        assert 0.49 < frac < 0.51, (name, frac)
        if G[f"{name}/n"]:
            for n in names:
                p = G[f"{name}/lin/{n}/pruned"]
                assert bool((p.view(p.shape[0], -1, 4).sum(-1) == 2).all()), (name, n)
    # the two routes decide differently from the second block on: the lora route calibrates on dense activations
    assert any(not torch.equal(G[f"prune_u50/lin/{n}/pruned"], G[f"lora_u50/lin/{n}/pruned"]) for n in linears("prune_u50"))
    for n in linears("prune_u50")[:4]:                          # block 0 of the ViT sees the same inputs on both routes
        if n.startswith("visual_encoder.blocks.0."):
            assert torch.equal(G[f"prune_u50/lin/{n}/pruned"], G[f"lora_u50/lin/{n}/pruned"]), n


def _generator_module():
    spec = importlib.util.spec_from_file_location("make_golden_sparsegpt_vicuna",
                                                  os.path.join(HERE, "golden", "make_golden_sparsegpt_vicuna.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class OracleHelper:
    """The reference's `SparseGPT` helper surface (add_batch / fasterprune / free, sparsegpt_pruner.py:53-219) on the oracle's
    restatement of its statements (oracle/sparsegpt.py)."""

    def __init__(self, layer):
        self.layer = layer
        self.H = torch.zeros((layer.weight.shape[1], layer.weight.shape[1]))
        self.nsamples = 0

    def add_batch(self, inp, out):
        self.nsamples = OS.hessian_update(self.H, self.nsamples, inp)

    def fasterprune(self, sparsity, prune_n=0, prune_m=0, blocksize=128, percdamp=0.01):
        Wn, imp, _ = OS.prune(self.layer.weight.data, self.H, sparsity, prune_n, prune_m, blocksize, percdamp)
        self.layer.weight.data = Wn
        setattr(self.layer.weight, "importance_score", imp)

    def free(self):
        self.H = None


@pytest.mark.parametrize("name", VARIANTS)
def test_cpu_restatement_reproduces_the_golden(name):
    """The generator's block loop with the oracle in place of the reference's helper: pruned sets (seen through the sweep's own
    `q[mask1[:, i]] = 0`), weights and importance scores of the reference's run, bit for bit."""
    import types
    from lavis.peft.src.peft.tuners.lora import Linear
    gen = _generator_module()
    G = golden()
    v = dict(lora=bool(G[f"{name}/lora"]), ratio=float(G[f"{name}/ratio"]), n=int(G[f"{name}/n"]), m=int(G[f"{name}/m"]))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        model, batches = gen.build_model()
        if v["lora"]:
            gen.wrap_block_linears(model, Linear)
        record = {}
        for tower, vit in gen.TOWERS:
            gen.restated_tower(types.SimpleNamespace(SparseGPT=OracleHelper), model, batches, tower, vit, v, record)
    finally:
        torch.set_num_threads(threads)
    assert sorted(record) == linears(name)
    for mn, (pruned, Wn, imp) in record.items():
        assert torch.equal(pruned, G[f"{name}/lin/{mn}/pruned"]), mn
        assert imp == pytest.approx(float(G[f"{name}/lin/{mn}/imp"]), rel=1e-6), mn
        if not v["lora"]:
            assert torch.equal(Wn[~pruned], G[f"{name}/lin/{mn}/Wn_kept"]), mn


# ---- the drop-in pruners with CPU stand-ins ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_pruner_with_cpu_stand_ins_matches_the_golden(name, monkeypatch):
    """blipt5_sparsegpt_pruner on the Vicuna branch -- prune-only and lora_model=True on the PEFT-wrapped model -- with the kernels
    replaced by the oracle and the reference's per-sample Hessian recurrence: every weight, pruned set, mask and importance score
    of the golden, bit for bit."""
    install_cpu(monkeypatch)
    monkeypatch.setenv("VLMC_BATCH_REPLAY", "1")
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        mods, w0 = run_pruner(name)
    finally:
        torch.set_num_threads(threads)
    assert check_against_golden(name, mods, w0) == (1.0, 0.0)
    masked = [mn for mn in linears(name) if isinstance(getattr(mods[mn], "mask", None), torch.Tensor)]
    if golden()[f"{name}/lora"]:
        assert len(masked) == len(linears(name))
        for mn in masked:
            assert mods[mn].mask.dtype == torch.bool and mods[mn].mask.shape == mods[mn].weight.shape
    else:
        assert not masked                                            # prune-only attaches no mask (sparsegpt_pruner.py:215)


def test_tower_pruners_take_lora_model(monkeypatch):
    """t5_sparsegpt_pruner and vit_sparsegpt_pruner run prune(lora_model=...) (the reference's :511-543 / :838-864 plus the flag):
    with True every block linear gets a mask of the requested sparsity and no parameter changes; with False the weights are
    pruned in place and no mask is attached."""
    from lavis.compression import load_pruner
    install_cpu(monkeypatch)
    batches = toy_models.make_batches(6, seed=11)

    def toy():
        model = toy_models.init_toy(toy_models.ToyBlipT5(), seed=7).eval()
        model.encode_image = lambda image: _encode(model, image)
        return model

    def block_linears(model, prefix):
        return {n: m for n, m in model.named_modules() if n.startswith(prefix) and type(m) is torch.nn.Linear}

    for name, prefix, n_lin in (("vit_sparsegpt_pruner", "visual_encoder", 2 * 4), ("t5_sparsegpt_pruner", "t5_model", 2 * 7 + 2 * 11)):
        cfg = dict(prune_spec="2-0.5-1.0-1.0", num_samples=6, model_prefix=prefix, max_sparsity_per_layer=1.01)
        model = toy()
        w0 = {n: p.detach().clone() for n, p in model.named_parameters()}
        pruned, sd = load_pruner(name, model, batches, cfg=cfg).prune(lora_model=True)
        assert sd is not None
        lins = block_linears(pruned, prefix)
        assert len(lins) == n_lin
        for n, m in lins.items():
            assert m.mask.dtype == torch.bool and 0.45 < float((~m.mask).float().mean()) < 0.55, n
        for n, p in pruned.named_parameters():
            assert torch.equal(p, w0[n]), n
        pruned, _ = load_pruner(name, toy(), batches, cfg=cfg).prune()
        for n, m in block_linears(pruned, prefix).items():
            assert not hasattr(m, "mask") and 0.45 < float((m.weight == 0).float().mean()) < 0.55, n


def _encode(model, image):
    x = image
    for blk in model.visual_encoder.blocks:
        x = blk(x, None)
    return x


def test_other_llm_prefixes_keep_the_opt_walk(monkeypatch):
    """Only a prefix containing "llm_model" takes the LLaMA layout; any other non-T5 prefix walks `...model.decoder.layers` as
    the reference does (:1084) -- here a model without it raises as the reference would."""
    install_cpu(monkeypatch)
    with pytest.raises(AttributeError, match="decoder"):
        model, batches = build_model(False)
        model.opt_model = model.llm_model
        from lavis.compression import load_pruner
        load_pruner("blipt5_sparsegpt_pruner", model, batches,
                    cfg=dict(t5_prune_spec="2-0.5-1.0-1.0", vit_prune_spec=None, t5_pruning_method="sparsegpt",
                             vit_pruning_method="sparsegpt", num_samples=6, t5_model_prefix="opt_model",
                             max_sparsity_per_layer=1.01)).prune()


# ---- refusals without a GPU ------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_gpu():
    """No CPU fallback on the new route, and the C entry points the Vicuna shapes go through refuse what they cannot take before
    touching a device; the workspaces of the 11008-wide factorization and Hessian are sized on the host."""
    from vlmc import _lib, sparsegpt
    lin = torch.nn.Linear(256, 32, bias=False)
    with pytest.raises(RuntimeError, match="GPU only"):
        sparsegpt.fasterprune(lin, torch.eye(256), 0.5, mask_only=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        sparsegpt.SparseGPT(lin)
    lib = _lib.load()
    P = ctypes.c_void_p(1 << 20)
    nblk = 11008 // 128
    assert lib.vlmc_chol_inverse_workspace(11008) == -(-(2 + 2 * nblk * nblk) * 4 // 256) * 256
    info = ctypes.c_void_p(1 << 21)
    ws = lib.vlmc_chol_inverse_workspace(11008)
    assert lib.vlmc_chol_inverse(P, 11000, 11008, P, 11008, P, 11008, info, P, ws, 0, None) == _lib.VLMC_EINVAL   # n % 128
    assert lib.vlmc_chol_inverse(P, 11008, 11000, P, 11008, P, 11008, info, P, ws, 0, None) == _lib.VLMC_EINVAL   # lda < n
    assert lib.vlmc_chol_inverse(P, 11008, 11008, P, 11008, P, 11008, info, P, ws - 256, 0, None) == _lib.VLMC_EWORKSPACE
    assert lib.vlmc_hessian_workspace(_lib.F16, 128 * 60, 11008) > 0
    assert lib.vlmc_hessian_accum(P, _lib.F16, 64, 1 << 20, 1 << 20, P, 1 << 20, ctypes.c_float(1.0), ctypes.c_float(1.0), P,
                                  1 << 30, None) == _lib.VLMC_EINVAL                                              # in >= 2^20
    err = ctypes.c_void_p(1 << 22)
    sweep = lambda rows, count, ldw, n, m, mask1, ldmo: lib.vlmc_sparsegpt_sweep(
        P, rows, count, ldw, P, 11008, mask1, 128, n, m, err, 128, P, ldmo, None)
    assert sweep(11008, 129, 4096, 2, 4, None, 4096) == _lib.VLMC_EINVAL                                       # count > 128
    assert sweep(11008, 128, 64, 2, 4, None, 4096) == _lib.VLMC_EINVAL                                         # ldw < count
    assert sweep(11008, 128, 4096, 4, 16, None, 4096) == _lib.VLMC_EINVAL                                      # m > 8
    assert sweep(11008, 128, 4096, 0, 0, None, 4096) == _lib.VLMC_EINVAL                                       # no block mask
    blocks = lambda bs, n, m: lib.vlmc_sparsegpt_prune_blocks(P, 4096, 11008, 11008, P, 11008, bs, n, m, 0, None, None, err, 128,
                                                              P, 11008, None, None)
    assert blocks(256, 2, 4) == _lib.VLMC_EINVAL                                                               # blocksize > 128
    assert blocks(128, 0, 0) == _lib.VLMC_EINVAL                                                               # unstructured: scopes
    assert b"vlmc_sparsegpt_prune_blocks" in lib.vlmc_last_error()


# ---- worlds of two (gloo) --------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, name, shard_layers):
    for p in (ROOT, os.path.join(ROOT, "vlm-compression_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["VLMC_SGPT_SHARD_LAYERS"] = shard_layers
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    import test_sparsegpt_vicuna as T
    from vlmc import sparsegpt

    class MP:
        @staticmethod
        def setattr(obj, attr, val):
            setattr(obj, attr, val)
    T.install_cpu(MP)
    calls = []
    real = sparsegpt.fasterprune

    def counting(layer, *a, **k):
        calls.append(tuple(layer.weight.shape))
        return real(layer, *a, **k)
    sparsegpt.fasterprune = counting
    mods, w0 = T.run_pruner(name)
    out = {"calls": len(calls), "agree": T.check_against_golden(name, mods, w0, exact=False),
           "w": {mn: mods[mn].weight.data.clone() for mn in T.linears(name)},
           "mask": {mn: mods[mn].mask.clone() for mn in T.linears(name) if isinstance(getattr(mods[mn], "mask", None), torch.Tensor)},
           "imp": {mn: mods[mn].weight.importance_score for mn in T.linears(name)}}
    torch.save(out, os.path.join(out_dir, f"{name}_{shard_layers}_{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["prune_2_4", "lora_u50"])
def test_layer_sharded_world2_equals_replicated_pruning(name, tmp_path):
    """Every linear pruned by one rank and its result broadcast -- the weights, or under lora_model the mask -- equals every rank
    pruning everything, bit for bit: weights, masks and importance scores; the layer-sharded ranks split the linears."""
    for mode in ("1", "0"):
        mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), name, mode), nprocs=2, join=True)
    s0, s1 = torch.load(tmp_path / f"{name}_1_0.pt"), torch.load(tmp_path / f"{name}_1_1.pt")
    r0 = torch.load(tmp_path / f"{name}_0_0.pt")
    n = len(linears(name))
    assert r0["calls"] == n and s0["calls"] + s1["calls"] == n and 0 < s0["calls"] < n
    for key in ("w", "mask"):
        assert r0[key].keys() == s0[key].keys() == s1[key].keys()
        for mn in r0[key]:
            assert torch.equal(s0[key][mn], r0[key][mn]) and torch.equal(s1[key][mn], r0[key][mn]), (key, mn)
    assert s0["imp"] == s1["imp"] == r0["imp"]
    if name.startswith("lora"):
        assert len(r0["mask"]) == n


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["prune_u50", "lora_2_4"])
def test_sample_sharded_world2_tracks_the_golden(name, tmp_path):
    """Each rank accumulates the Hessians of its samples, one all-reduce forms the sample-weighted mean; the sum order differs from
    the sequential running mean, so the ranks agree bit for bit with each other and track the reference's single-process run."""
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), name, "1"), nprocs=2, join=True)
    a, b = torch.load(tmp_path / f"{name}_1_0.pt"), torch.load(tmp_path / f"{name}_1_1.pt")
    for key in ("w", "mask"):
        for mn in a[key]:
            assert torch.equal(a[key][mn], b[key][mn]), (key, mn)
    agree, rel = a["agree"]
    print(f"{name}: world-2 pattern agreement {agree:.5f}, relative RMS {rel:.2e}")
    assert agree >= 0.97 and rel < 2e-2
