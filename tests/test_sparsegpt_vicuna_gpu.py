"""SparseGPT pruners on InstructBLIP-Vicuna and under `prune(lora_model=True)` on the GPU: the toy Vicuna against the reference's
run (tests/golden/sparsegpt_vicuna.npz), the lora route's masks against prune-only sweeps on the same Hessians, and one
full-size Vicuna-7B layer (4096 / 11008) against fp64 -- every Hessian, factor chain and sweep at the widths of that model
(`vlmc_hessian_accum` at in = 11008, `vlmc_chol_inverse` at n = 11008, the sweeps at 4096 x 11008, 11008 x 4096 and the
stacked q/k/v and gate/up rows).  The CPU side is in tests/test_sparsegpt_vicuna.py."""
import pytest
import torch
import torch.nn.functional as F

import test_sparsegpt_vicuna as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _nm_exact(pruned, m=4, n=2):
    return pruned.shape[1] % m == 0 and bool((pruned.view(pruned.shape[0], -1, m).sum(-1) == n).all())


# ---- the toy Vicuna against the reference's run ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["prune_u50", "prune_2_4"])
def test_toy_vicuna_prune_only_tracks_the_reference_run(name):
    """Whole blipt5_sparsegpt_pruner on the Vicuna branch with the kernels: the GPU factorization and Hessians accumulate in
    another order than the reference's CPU run, so the zero pattern agrees up to near-ties, the weights are close on the rows
    whose pattern agrees, and 2:4 is exact."""
    mods, w0 = T.run_pruner(name, DEV)
    agree, rel = T.check_against_golden(name, mods, w0, exact=False)
    print(f"{name}: pattern agreement {agree:.5f}, relative RMS {rel:.2e}")
    assert agree >= 0.97 and rel < 2e-2
    for mn in T.linears(name):
        assert not hasattr(mods[mn], "mask")
        if name.endswith("2_4"):
            assert _nm_exact(mods[mn].weight.data == 0), mn


class _SameSweepCheck:
    """Around the pruner's mask-only sweeps: the same linear swept by the prune-only route (a copy of it, the factor of the same
    Hessian) must hand back exactly the complement of the mask."""

    def __init__(self, monkeypatch):
        from vlmc import sparsegpt
        self.checked = 0
        real_one, real_group = sparsegpt.fasterprune, sparsegpt.fasterprune_group

        def prune_only_mask(layer, sparsity, cache, prune_n, prune_m):
            twin = torch.nn.Linear(layer.in_features, layer.out_features, bias=False, device=layer.weight.device,
                                   dtype=layer.weight.dtype)
            twin.weight.data.copy_(layer.weight.data)
            return real_one(twin, None, sparsity, prune_n=prune_n, prune_m=prune_m, blocksize=128, factor_cache=cache,
                            return_mask=True)

        def one(layer, H, sparsity, prune_n=0, prune_m=0, factor_cache=None, mask_only=False, **kw):
            out = real_one(layer, H, sparsity, prune_n=prune_n, prune_m=prune_m, factor_cache=factor_cache, mask_only=mask_only, **kw)
            if mask_only:
                assert torch.equal(prune_only_mask(layer, sparsity, factor_cache, prune_n, prune_m), ~out)
                self.checked += 1
            return out

        def group(layers, sparsities, factor_cache, prune_n=0, prune_m=0, mask_only=False, **kw):
            out = real_group(layers, sparsities, factor_cache, prune_n=prune_n, prune_m=prune_m, mask_only=mask_only, **kw)
            if mask_only:
                for layer, sp, keep in zip(layers, sparsities, out):
                    assert torch.equal(prune_only_mask(layer, sp, factor_cache, prune_n, prune_m), ~keep)
                    self.checked += 1
            return out
        monkeypatch.setattr(sparsegpt, "fasterprune", one)
        monkeypatch.setattr(sparsegpt, "fasterprune_group", group)


@pytest.mark.parametrize("name", ["lora_u50", "lora_2_4"])
def test_lora_route_keeps_weights_and_attaches_the_sweeps_masks(name, monkeypatch):
    """prune(lora_model=True) on the get_peft_model-wrapped toy: every weight keeps its bytes, every mask tracks the reference's
    pruned set (2:4 exact), each mask is the prune-only sweep's decision on the same factor bit for bit, and a second run is
    identical."""
    check = _SameSweepCheck(monkeypatch)
    mods, w0 = T.run_pruner(name, DEV)
    agree, _ = T.check_against_golden(name, mods, w0, exact=False)                      # (asserts the weights' bytes)
    print(f"{name}: mask agreement {agree:.5f}")
    assert agree >= 0.97
    assert check.checked == len(T.linears(name))
    for mn in T.linears(name):
        mask = mods[mn].mask
        assert mask.is_cuda and mask.dtype == torch.bool and mask.shape == mods[mn].weight.shape
        if name.endswith("2_4"):
            assert _nm_exact(~mask), mn
    again, _ = T.run_pruner(name, DEV)
    for mn in T.linears(name):
        assert torch.equal(again[mn].mask, mods[mn].mask), mn
        assert torch.equal(again[mn].weight, mods[mn].weight), mn


def test_lora_masks_are_what_the_sparse_lora_linear_trains_with():
    """The masked SparseLoRA forward (the RESSA student) zeroes exactly the pruned weights; the dense one (the teacher) reads
    the untouched weight."""
    mods, w0 = T.run_pruner("lora_u50", DEV)
    lin = mods["llm_model.model.layers.1.mlp.down_proj"]
    x = torch.randn(5, lin.in_features, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    with torch.no_grad():
        lin.lora_B.weight.zero_()                                   # the adapter's delta out of the way
        dense = lin(x, dense=True)
        masked = lin(x)
    torch.testing.assert_close(dense, F.linear(x, w0["llm_model.model.layers.1.mlp.down_proj"]), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(masked, F.linear(x, lin.weight * lin.mask), rtol=1e-4, atol=1e-5)
    assert not torch.allclose(masked, dense)


# ---- one full-size Vicuna-7B layer ------------------------------------------------------------------------------------------------
_FULL = {}


def _full_layer_prune(n, m):
    """blipt5_sparsegpt_pruner over ONE InstructBLIP-Vicuna-7B layer (fp16, 4096 / 11008) with 128 calibration samples of 112
    tokens (14336 rows > 11008: every Hessian positive definite).  Returns (weights before, layer after, [(H, U)] per input)."""
    key = (n, m)
    if key in _FULL:
        return _FULL[key]
    from lavis.compression import load_pruner
    from vlmc import sparsegpt, synthetic
    model = synthetic.InstructBlipVicuna(vit_depth=1, depth=1).to(DEV).eval()
    synthetic.randomize_(model, seed=3)
    batches = synthetic.calibration_batches(128, DEV, text_len=64, out_len=16, vocab=32000, seed=2)
    layer = model.llm_model.model.layers[0]
    w0 = {name: mod.weight.data.clone() for name, mod in layer.named_modules() if isinstance(mod, torch.nn.Linear)}
    factors = []
    real = sparsegpt.factorize_many

    def recording(items, *a, **k):
        hs = [H.clone() for H, _ in items]
        real(items, *a, **k)
        factors.extend((h, c) for h, (_, c) in zip(hs, items))
    sparsegpt.factorize_many = recording
    stats0 = dict(sparsegpt.factor_stats)
    try:
        load_pruner("blipt5_sparsegpt_pruner", model, batches,
                    cfg=dict(t5_prune_spec="1-0.5-1.0-1.0", vit_prune_spec=None, t5_pruning_method="sparsegpt",
                             vit_pruning_method="sparsegpt", num_samples=128, prune_n=n, prune_m=m, t5_model_prefix="llm_model",
                             max_sparsity_per_layer=1.01)).prune()
    finally:
        sparsegpt.factorize_many = real
    assert sparsegpt.factor_stats["direct"] - stats0.get("direct", 0) == 4                # q/k/v, o, gate/up, down: undamped
    assert [H.shape[0] for H, _ in factors] == [4096, 4096, 4096, 11008]    # the accumulators in the block's order: q/k/v, o, gate/up, down
    _FULL.clear()
    _FULL[key] = (w0, layer, [(H, c["U"]) for H, c in factors])
    return _FULL[key]


def _fp64_factor(H):
    """The reference's chain (sparsegpt_pruner.py:112-150) in float64 on an undamped positive definite H."""
    H64 = H.double()
    return torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H64)), upper=True)


def _fp64_sweep(W, U, pruned, blocksize=128):
    """sparsegpt_pruner.py:167-210 in float64 with the pruned set given (rows are independent given the factor and the masks)."""
    W = W.double().clone()
    U = U.double()
    cols = W.shape[1]
    for i1 in range(0, cols, blocksize):
        i2 = min(i1 + blocksize, cols)
        W1 = W[:, i1:i2].clone()
        Err1 = torch.zeros_like(W1)
        for i in range(i2 - i1):
            w = W1[:, i]
            q = torch.where(pruned[:, i1 + i], torch.zeros_like(w), w)
            err = (w - q) / U[i1 + i, i1 + i]
            W1[:, i:] -= err.unsqueeze(1) * U[i1 + i, i1 + i:i2].unsqueeze(0)
            W1[:, i] = q
            Err1[:, i] = err
        W[:, i1:i2] = W1
        W[:, i2:] -= Err1 @ U[i1:i2, i2:]
    return W


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n,m", [(0, 0), (2, 4)])
def test_full_size_vicuna_layer_against_fp64(n, m):
    """Every linear of a Vicuna-7B layer, unstructured 50 % and 2:4: the pruned fraction (or 2:4 structure) exact, and on 256
    rows the weights equal an fp64 restatement of the same sweep (the GPU's factor, its pruned set) to fp16 rounding; the
    factors of the 4096- and 11008-wide Hessians equal the fp64 chain."""
    w0, layer, factors = _full_layer_prune(n, m)
    for H, U in factors:
        truth = _fp64_factor(H)
        rel = float((U.double() - truth).norm() / truth.norm())
        print(f"factor n={H.shape[0]}: relative error against fp64 {rel:.2e}")
        assert rel < 2e-3, (H.shape[0], rel)
    source = {"self_attn.q_proj": 0, "self_attn.k_proj": 0, "self_attn.v_proj": 0, "self_attn.o_proj": 1, "mlp.gate_proj": 2,
              "mlp.up_proj": 2, "mlp.down_proj": 3}
    assert sorted(source) == sorted(w0)
    rows = torch.arange(0, 256, device=DEV) * 11 % 4096
    mods = dict(layer.named_modules())
    for name, W0 in w0.items():
        Wn = mods[name].weight.data
        pruned = Wn == 0
        frac = float(pruned.float().mean())
        if n:
            assert _nm_exact(pruned), name
        else:
            assert abs(frac - 0.5) < 2e-3, (name, frac)
        ref = _fp64_sweep(W0[rows], factors[source[name]][1], pruned[rows])
        rel = float((Wn[rows].double() - ref).norm() / ref.norm())
        print(f"{name} {tuple(W0.shape)}: pruned {frac:.4f}, weights against fp64 {rel:.2e}")
        assert rel < 2e-3, (name, rel)
