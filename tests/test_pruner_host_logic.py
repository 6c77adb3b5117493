"""CPU: the drop-in pruners' host logic (capture, block walk, tower order, inps/outs swap,
hook de-duplication, lora_model semantics, importance read-back) against whole-pruner golden
runs of the REFERENCE on the toy InstructBLIP (tests/golden/wanda_e2e.npz).

The numeric kernels are GPU-only, so `vlmc.ops` is monkeypatched with oracle-backed
stand-ins (tests/oracle_ops.py) -- a test fixture, not a product fallback.  On CPU the toy
model's forward is the same PyTorch code the reference ran, so everything must match the
golden bit for bit."""
import pytest
import torch

import oracle_ops
import pruner_helpers as H


@pytest.mark.parametrize("name", list(H.VARIANTS))
def test_blipt5_wanda_pruner_matches_reference_run(name, monkeypatch):
    oracle_ops.install(monkeypatch)
    pruned, sd = H.run_pruner(name, "cpu")
    assert sd is None                                  # granularity none -> (model, None)
    st = H.compare_with_golden(name, pruned, exact=True, min_mask_agreement=1.0)
    assert st["masks"] == 2 * 4 + 2 * 7 + 2 * 11       # every prunable linear of the toy got a mask


def test_lora_model_keeps_weights_dense_and_sets_mask_buffers(monkeypatch):
    oracle_ops.install(monkeypatch)
    model, _, _ = H.build("fp32_r40_lora")
    before = {k: v.clone() for k, v in model.state_dict().items() if k.endswith("weight")}
    pruned, _ = H.run_pruner("fp32_r40_lora")
    for k, v in pruned.state_dict().items():
        if k.endswith(".weight") and "lora_" not in k and k in before:
            assert torch.equal(v, before[k]), k        # wanda_pruner.py:340-341: no zeroing under lora_model
    masks = [v for k, v in pruned.state_dict().items() if k.endswith(".mask")]
    assert masks and all(m.dtype == torch.bool for m in masks)
    sparsity = 1 - sum(m.sum().item() for m in masks) / sum(m.numel() for m in masks)
    assert 0.37 < sparsity <= 0.40     # int(in*0.4)/in per row, e.g. 12/32


def test_registry_and_load_pruner_contract():
    from lavis.common.registry import registry
    from lavis.compression import load_pruner
    for n in ("t5_wanda_pruner", "vit_wanda_pruner", "blipt5_wanda_pruner"):
        assert registry.get_pruner_class(n) is not None
    with pytest.raises(SystemExit):                    # reference: TypeError -> message + exit(1)
        load_pruner("no_such_pruner", None, None, cfg={})


def test_pruner_has_no_cpu_fallback():
    """Without the test stand-ins a CPU model must raise, not silently compute on the host."""
    with pytest.raises(RuntimeError, match="GPU only"):
        H.run_pruner("fp32_r50", "cpu")


# ---- SparseGPT pruner host logic ---------------------------------------------------------
import golden_io  # noqa: E402

SG_E2E = golden_io.load("sparsegpt_e2e")


def _run_sparsegpt_pruner(name, device="cpu", n_samples=6):
    import toy_models
    from lavis.compression import load_pruner
    v = {"fp32_u50": dict(ratio=0.5, n=0, m=0), "fp32_2_4": dict(ratio=0.5, n=2, m=4)}[name]
    model = toy_models.init_toy(toy_models.ToyBlipT5(), seed=7).eval().to(device)
    batches = [{k: t.to(device) for k, t in b.items()} for b in toy_models.make_batches(n_samples, seed=11)]
    spec = "2-%r-1.0-1.0" % (1 - v["ratio"])
    cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method="sparsegpt", vit_pruning_method="sparsegpt",
               num_samples=n_samples, prune_n=v["n"], prune_m=v["m"], max_sparsity_per_layer=1.01)
    pruner = load_pruner("blipt5_sparsegpt_pruner", model, batches, cfg=cfg)
    return pruner.prune()


@pytest.mark.parametrize("name", ["fp32_u50", "fp32_2_4"])
def test_blipt5_sparsegpt_pruner_matches_reference_run(name, monkeypatch):
    oracle_ops.install_sparsegpt(monkeypatch)
    # bit-exact against the reference's run needs its per-sample Hessian recurrence (one rounding pattern per update);
    # the default grouped replay feeds all samples in one update and is held to SparseGPT's tolerance below
    # (test_batched_replay_keeps_per_sample_statistics[sparsegpt])
    monkeypatch.setenv("VLMC_BATCH_REPLAY", "1")
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)                      # the goldens' BLAS configuration (see test_oracle_golden.py)
    try:
        pruned, sd = _run_sparsegpt_pruner(name)
    finally:
        torch.set_num_threads(nthreads)
    assert sd is None
    got = pruned.state_dict()
    n_checked = 0
    for key in [k for k in SG_E2E if k.startswith(f"{name}/sd/")]:
        assert torch.equal(got[key[len(name) + 4:]], SG_E2E[key]), key
        n_checked += 1
    assert n_checked > 40
    for mn, mod in pruned.named_modules():
        ik = f"{name}/imp/{mn}"
        if ik in SG_E2E:
            assert mod.weight.importance_score == pytest.approx(float(SG_E2E[ik]), rel=1e-6)
            assert not hasattr(mod, "mask")       # SparseGPT attaches no mask (sparsegpt_pruner.py:215)


# ---- DSnoT pruner host logic ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.DSNOT_VARIANTS))
def test_blipt5_dsnot_pruner_matches_reference_run(name, monkeypatch):
    """Whole blipt5_dsnot_pruner (ViT -> encoder -> decoder) with oracle stand-ins for the kernels
    vs the reference's own run (tests/golden/dsnot_e2e.npz): every state tensor and mask identical."""
    oracle_ops.install_dsnot(monkeypatch)
    pruned, sd = H.run_dsnot_pruner(name, "cpu")
    assert sd is None
    st = H.compare_with_golden(name, pruned, exact=True, min_mask_agreement=1.0, which="dsnot_e2e")
    assert st["masks"] == 2 * 4 + 2 * 7 + 2 * 11
    for mn, mod in pruned.named_modules():
        if hasattr(mod, "weight") and isinstance(mod.weight, torch.Tensor):
            assert not hasattr(mod.weight, "importance_score")      # dsnot_pruner.py:365 is commented out


def test_dsnot_registry_and_tower_pruners(monkeypatch):
    from lavis.common.registry import registry
    import lavis.compression  # noqa: F401  (registers the pruners)
    for n in ("t5_dsnot_pruner", "vit_dsnot_pruner", "blipt5_dsnot_pruner"):
        assert registry.get_pruner_class(n) is not None
    # the standalone T5 tower pruner runs on its own here (the reference's cannot: `initial_method` is only set by
    # the BLIP pruner) and equals the BLIP pruner with the ViT tower left dense
    import toy_models
    from lavis.compression import load_pruner
    oracle_ops.install_dsnot(monkeypatch)

    def fresh():
        return toy_models.init_toy(toy_models.ToyBlipT5(), seed=7).eval(), toy_models.make_batches(6, seed=11)

    model, batches = fresh()
    pr = load_pruner("t5_dsnot_pruner", model, batches,
                     cfg=dict(prune_spec="2-0.5-1.0-1.0", model_prefix="t5_model", num_samples=6, max_cycle_time=20,
                              max_sparsity_per_layer=1.01))
    a, sd = pr.prune()
    assert sd is not None and all(abs(v - 0.5) < 1e-12 for v in [sd["t5_model.encoder.block.0.SelfAttention.q.weight"]])
    model, batches = fresh()
    pr = load_pruner("blipt5_dsnot_pruner", model, batches,
                     cfg=dict(t5_prune_spec="2-0.5-1.0-1.0", vit_prune_spec="2-1.0-1.0-1.0", t5_pruning_method="dsnot",
                              vit_pruning_method="dsnot", num_samples=6, max_cycle_time=20, max_sparsity_per_layer=1.01))
    b, _ = pr.prune()
    n = 0
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
        n += 1
    assert n > 40
    masks = [m.mask for m in a.modules() if hasattr(m, "mask")]
    assert len(masks) == 2 * 7 + 2 * 11 and all(bool((mk.sum(1) == mk.shape[1] // 2).all()) for mk in masks)


def test_dsnot_pruner_has_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="GPU only"):
        H.run_dsnot_pruner("fp32_r50", "cpu")


# ---- batched block replay -------------------------------------------------------
@pytest.mark.parametrize("method", ["wanda", "dsnot", "sparsegpt"])
def test_batched_replay_keeps_per_sample_statistics(method, monkeypatch):
    """VLMC_BATCH_REPLAY=4: up to 4 equal-shape samples per block forward.  Per-sample statistics records are kept,
    so on this CPU (whose matmul gives the same rows for any batch) Wanda and DSnoT reproduce the reference's golden
    run exactly; SparseGPT's Hessian sees batch-4 updates and stays within its tolerance."""
    monkeypatch.setenv("VLMC_BATCH_REPLAY", "4")
    from lavis.compression.pruners import calibration as cal
    calls = {"n": 0, "stacked": 0}
    real = cal._stack_caches

    def counting(group, b0):
        calls["stacked"] += 1
        return real(group, b0)
    monkeypatch.setattr(cal, "_stack_caches", counting)
    if method == "wanda":
        oracle_ops.install(monkeypatch)
        pruned, _ = H.run_pruner("fp32_r50", "cpu")
        st = H.compare_with_golden("fp32_r50", pruned, exact=False, min_mask_agreement=0.999)
    elif method == "dsnot":
        oracle_ops.install_dsnot(monkeypatch)
        pruned, _ = H.run_dsnot_pruner("fp32_r50", "cpu")
        st = H.compare_with_golden("fp32_r50", pruned, exact=False, min_mask_agreement=0.999, which="dsnot_e2e")
    else:
        oracle_ops.install_sparsegpt(monkeypatch)
        torch.set_num_threads(1)
        pruned, _ = _run_sparsegpt_pruner("fp32_u50")
        got = pruned.state_dict()
        tot = agree = 0
        for key in [k for k in SG_E2E if k.startswith("fp32_u50/sd/")]:
            ref, g = SG_E2E[key], got[key[len("fp32_u50/sd/"):]]
            if ref.dim() == 2 and ".block" in key:
                tot += ref.numel()
                agree += int(((g == 0) == (ref == 0)).sum())
        assert agree / tot > 0.97
        st = {"mask_diff": None}
    # 6 samples in groups of 4 + 2; the cached kwargs of a group are the same for every block of a tower (the reference replays
    # block 0's kwargs throughout, wanda_pruner.py:247-249), so they are stacked once per group and tower: 2 groups x 3 towers
    assert calls["stacked"] == 2 * 3
    print(method, st)


@pytest.mark.parametrize("method", ["wanda", "dsnot"])
def test_grouped_replay_of_ragged_calibration_text_keeps_the_sample_order(method, monkeypatch):
    """Real calibration text is ragged: samples of equal shape are grouped even when they are not neighbours
    (calibration.plan_groups), and the statistics still run the reference's recurrence in SAMPLE order -- the masks of
    the grouped replay equal those of the per-sample loop (this CPU's matmul gives the same rows for any batch)."""
    import toy_models
    from lavis.compression import load_pruner
    from lavis.compression.pruners import calibration as cal
    (oracle_ops.install if method == "wanda" else oracle_ops.install_dsnot)(monkeypatch)
    lens = [5, 7, 5, 5, 7, 3, 5, 7]                                  # text lengths: three shapes, interleaved

    def run(group):
        monkeypatch.setenv("VLMC_BATCH_REPLAY", str(group))
        model = toy_models.init_toy(toy_models.ToyBlipT5(), seed=7).eval()
        batches = []
        for j, n in enumerate(lens):
            b = toy_models.make_batches(1, txt_len=n, out_len=2 + n % 3, seed=100 + j)[0]
            batches.append(b)
        spec = "2-0.5-1.0-1.0"
        cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method=method, vit_pruning_method=method,
                   num_samples=len(lens), max_sparsity_per_layer=1.01)
        if method == "dsnot":
            cfg["max_cycle_time"] = 8
        pruned, _ = load_pruner(f"blipt5_{method}_pruner", model, batches, cfg=cfg).prune()
        return {n: m.mask.clone() for n, m in pruned.named_modules() if hasattr(m, "mask")}

    plans = []
    real = cal.plan_groups

    def spy(cur_in, caches, n, g):
        out = real(cur_in, caches, n, g)
        plans.append(out)
        return out
    monkeypatch.setattr(cal, "plan_groups", spy)
    per_sample = run(1)
    assert not plans                                                  # the per-sample loop plans nothing
    grouped = run(128)
    assert [5, 7, 3] and any(len(c) > 1 and c != list(range(c[0], c[0] + len(c))) for p in plans for c in p), \
        "no group of non-neighbouring samples was formed"
    assert all(sorted(j for c in p for j in c) == list(range(len(lens))) for p in plans)
    assert per_sample.keys() == grouped.keys() and len(grouped) == 2 * 4 + 2 * 7 + 2 * 11
    for k in per_sample:
        assert torch.equal(per_sample[k], grouped[k]), k


# ---- the first pass ends where its last hook has fired -------------------------------------------------------------
@pytest.mark.parametrize("method", ["wanda", "dsnot", "sparsegpt"])
def test_statistics_pass_skips_the_dead_tail_and_changes_nothing(method, monkeypatch):
    """The pass that feeds the hooks does not compute the block's last linear (nor what follows it) from the tower's
    second block on -- the order of the linears is learned on the first block -- and the pruned model is the same, bit
    for bit, as with VLMC_SKIP_DEAD_TAIL=0."""
    import toy_models
    from lavis.compression import load_pruner
    {"wanda": oracle_ops.install, "dsnot": oracle_ops.install_dsnot, "sparsegpt": oracle_ops.install_sparsegpt}[method](monkeypatch)
    torch.set_num_threads(1)
    real_linear = torch.nn.functional.linear
    computed = {}

    def counting(x, weight, bias=None):                     # every product with a weight, whoever asks for it
        computed[id(weight)] = computed.get(id(weight), 0) + 1
        return real_linear(x, weight, bias)
    monkeypatch.setattr(torch.nn.functional, "linear", counting)

    def run(skip):
        monkeypatch.setenv("VLMC_SKIP_DEAD_TAIL", "1" if skip else "0")
        computed.clear()
        model = toy_models.init_toy(toy_models.ToyBlipT5(), seed=11).eval()
        batches = toy_models.make_batches(6, seed=5)
        spec = "2-0.5-1.0-1.0"
        cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method=method, vit_pruning_method=method,
                   num_samples=6, max_sparsity_per_layer=1.01)
        if method == "dsnot":
            cfg["max_cycle_time"] = 8
        pruned, _ = load_pruner(f"blipt5_{method}_pruner", model, batches, cfg=cfg).prune()
        last = {n: computed.get(id(m.weight), 0) for n, m in pruned.named_modules()
                if n.endswith((".mlp.fc2", "DenseReluDense.wo")) and ("blocks.1." in n or "block.1." in n)}
        return {k: v.clone() for k, v in pruned.state_dict().items()}, last

    full, n_full = run(False)
    cut, n_cut = run(True)
    assert full.keys() == cut.keys()
    for k in full:
        assert torch.equal(full[k], cut[k]), k
    # second block of each tower: its last linear is computed once less per forward of the first pass
    assert len(n_full) == 3 and n_cut.keys() == n_full.keys()
    assert all(n_cut[k] == n_full[k] - 1 for k in n_full), (n_cut, n_full)      # one grouped forward less


def test_statistics_pass_runs_to_the_end_when_the_order_is_not_the_learned_one():
    """`statistics_only` cuts a forward only when its calls so far are exactly the learned sequence: a block that uses a
    linear twice never learns an order; a block that calls its linears in another order than the first block computes
    everything."""
    from lavis.compression.pruners import calibration as cal

    class Twice(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Linear(4, 4), torch.nn.Linear(4, 4)

        def forward(self, x):
            return self.a(self.b(self.a(x)))

    class Ordered(torch.nn.Module):
        def __init__(self, flip=False):
            super().__init__()
            self.a, self.b, self.flip = torch.nn.Linear(4, 4), torch.nn.Linear(4, 4), flip

        def forward(self, x):
            return self.a(self.b(x)) if self.flip else self.b(self.a(x))

    x = torch.randn(3, 4)
    blk, learned = Twice().eval(), {}
    for _ in range(2):
        with cal.statistics_only(cal.find_layers(blk), learned) as so:
            so.new_forward()
            y = blk(x)
            so.end_forward(True)
        assert torch.equal(y, blk.a(blk.b(blk.a(x))))
    assert learned["order"] is False

    first, same, flipped, learned = Ordered().eval(), Ordered().eval(), Ordered(flip=True).eval(), {}
    seen_inputs = []
    with cal.statistics_only(cal.find_layers(first), learned) as so:
        so.new_forward()
        first(x)
        so.end_forward(True)
    assert learned["order"] == ("a", "b")
    h = same.b.register_forward_hook(lambda m, i, o: seen_inputs.append(i[0].clone()))
    with cal.statistics_only(cal.find_layers(same), learned) as so:
        so.new_forward()
        with pytest.raises(cal._TailStop):
            same(x)
    h.remove()
    assert len(seen_inputs) == 1 and torch.equal(seen_inputs[0], same.a(x))      # the hook saw b's input; b was not computed
    assert "forward" not in same.b.__dict__ and not same.b._forward_hooks and not same.a._forward_pre_hooks
    with cal.statistics_only(cal.find_layers(flipped), learned) as so:
        so.new_forward()
        y = flipped(x)                                                           # b first: not the learned order
        so.end_forward(True)
    assert torch.equal(y, flipped.a(flipped.b(x)))


# ---- round 3: advisor findings ----------------------------------------------------------------------------------------
def test_dead_tail_hands_hooks_no_product_and_stays_off_in_training_mode():
    """The cut linear's product is never formed: forward hooks get `None` for it (a hook that reads `out` fails loudly instead
    of reading uninitialised memory), and a training-mode block is never cut."""
    from lavis.compression.pruners import calibration as cal

    class Two(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Linear(4, 4), torch.nn.Linear(4, 4)

        def forward(self, x):
            return self.b(self.a(x))

    x = torch.randn(3, 4)
    first, second, learned = Two().eval(), Two().eval(), {}
    with cal.statistics_only(cal.find_layers(first), learned) as so:
        so.new_forward()
        first(x)
        so.end_forward(True)
    outs = []
    h = second.b.register_forward_hook(lambda m, i, o: outs.append(o))
    with cal.statistics_only(cal.find_layers(second), learned) as so:
        so.new_forward()
        with pytest.raises(cal._TailStop):
            second(x)
    assert outs == [None]
    second.train()
    outs.clear()
    with cal.statistics_only(cal.find_layers(second), learned) as so:
        so.new_forward()
        y = second(x)                                        # runs to the end
        so.end_forward(True)
    h.remove()
    assert len(outs) == 1 and torch.equal(outs[0], y)


def test_stacked_kwargs_only_concatenate_what_has_the_batch_dimension():
    """`_stack_caches`: per-sample tensors are concatenated; a tensor without the samples' batch dimension (a ViT
    rel_pos_bias [heads, N, N], a layer_head_mask [heads]) is passed once when all samples agree; disagreeing ones send the
    group to the per-sample path (None)."""
    from lavis.compression.pruners import calibration as cal
    bias = torch.randn(4, 5, 5)
    head_mask = torch.ones(4)
    group = [dict(attention_mask=torch.full((1, 1, 1, 5), float(j)), rel_pos_bias=bias, layer_head_mask=head_mask.clone(),
                  use_cache=False) for j in range(3)]
    kw = cal._stack_caches(group, 1)
    assert kw["attention_mask"].shape == (3, 1, 1, 5) and kw["rel_pos_bias"] is bias and kw["use_cache"] is False
    assert kw["layer_head_mask"].shape == (4,)
    group[1]["rel_pos_bias"] = bias + 1
    assert cal._stack_caches(group, 1) is None


def test_walk_blocks_replays_sample_by_sample_when_kwargs_cannot_be_stacked(monkeypatch):
    """A block with a batch-free kwarg that differs between samples: the grouped replay falls back to the reference's
    per-sample loop for that group and every sample meets ITS kwarg."""
    from lavis.compression.pruners import calibration as cal
    monkeypatch.setenv("VLMC_LINEAR_FWD", "0")

    class Blk(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(4, 4)

        def forward(self, x, rel_pos_bias=None):
            assert rel_pos_bias.shape == (2, 3, 3)
            return self.lin(x) + rel_pos_bias.sum()

    model = torch.nn.Module()
    model.blocks = torch.nn.ModuleList([Blk(), Blk()]).eval()
    xs = [torch.randn(1, 3, 4) for _ in range(4)]
    caches = [dict(rel_pos_bias=torch.full((2, 3, 3), float(j))) for j in range(4)]
    want = []
    for x, c in zip(xs, caches):
        with torch.no_grad():
            want.append(model.blocks[1](model.blocks[0](x, **c), **c))
    inps, outs = list(xs), [None] * 4
    import contextlib
    cal.walk_blocks(model, inps, outs, caches, "blocks", 4, contextlib.nullcontext, lambda i, layer, subset, run, state: run(), False)
    final = inps if outs[0] is None or not torch.equal(outs[0], want[0]) else outs
    got = final
    for j in range(4):
        assert torch.equal(got[j], want[j]), j


@pytest.mark.parametrize("method", ["wanda", "dsnot", "sparsegpt"])
def test_unstackable_kwargs_keep_per_sample_statistics_of_every_method(method, monkeypatch):
    """when a group's kwargs cannot be stacked (`_stack_caches` -> None) the chunk is replayed sample by sample and
    every sample must be announced to the collectors (`before_sample(j)`), as in the `group_max == 1` loop: the pruned
    model equals the per-sample loop's bit for bit, for ragged (non-contiguous) chunks too."""
    import toy_models
    from lavis.compression import load_pruner
    from lavis.compression.pruners import calibration as cal
    {"wanda": oracle_ops.install, "dsnot": oracle_ops.install_dsnot, "sparsegpt": oracle_ops.install_sparsegpt}[method](monkeypatch)
    torch.set_num_threads(1)
    lens = [5, 7, 5, 5, 7, 3]                                        # interleaved shapes: chunks of non-neighbouring samples

    def run(group, unstackable):
        monkeypatch.setenv("VLMC_BATCH_REPLAY", str(group))
        if unstackable:
            monkeypatch.setattr(cal, "_stack_caches", lambda grp, b0: None)
        model = toy_models.init_toy(toy_models.ToyBlipT5(), seed=3).eval()
        batches = [toy_models.make_batches(1, txt_len=n, out_len=2 + n % 3, seed=40 + j)[0] for j, n in enumerate(lens)]
        spec = "2-0.5-1.0-1.0"
        cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method=method, vit_pruning_method=method,
                   num_samples=len(lens), max_sparsity_per_layer=1.01)
        if method == "dsnot":
            cfg["max_cycle_time"] = 8
        pruned, _ = load_pruner(f"blipt5_{method}_pruner", model, batches, cfg=cfg).prune()
        return {k: v.clone() for k, v in pruned.state_dict().items()}

    announced = []
    if method != "sparsegpt":
        from lavis.compression.pruners import dsnot_pruner, wanda_pruner
        klass = wanda_pruner.WandaStatCollector if method == "wanda" else dsnot_pruner.DsnotStatCollector
        real_next = klass.next_sample

        def spy(self, j=None):
            announced.append(j)
            return real_next(self, j)
        monkeypatch.setattr(klass, "next_sample", spy)
    per_sample = run(1, False)
    n_loop = len(announced)
    forced = run(128, True)
    if method != "sparsegpt":
        # every sample of every statistics pass is announced, exactly as often as in the per-sample loop
        assert n_loop and len(announced) == 2 * n_loop
        assert sorted(announced[:n_loop]) == sorted(announced[n_loop:])
    assert per_sample.keys() == forced.keys()
    if method == "sparsegpt":
        # the Hessian's running mean takes the samples chunk by chunk (0, 2, 3 | 1, 4 | 5): another fp32 summation order,
        # the same matrix -- every sample counted once (the pruner asserts nsamples), masks agree up to near-ties
        tot = agree = 0
        for k in per_sample:
            if per_sample[k].dim() == 2 and ".block" in k:
                tot += per_sample[k].numel()
                agree += int(((per_sample[k] == 0) == (forced[k] == 0)).sum())
        assert tot and agree / tot > 0.97
        return
    for k in per_sample:
        assert torch.equal(per_sample[k], forced[k]), k


def test_deferred_importance_scores_survive_a_failing_tower(monkeypatch):
    """`prune()` postpones the importance-score readback to its end; if a tower raises, the flag must not outlive the call
    and the towers already pruned still get their scores."""
    import toy_models
    from lavis.compression import load_pruner
    from lavis.compression.pruners import wanda_pruner as wp
    oracle_ops.install(monkeypatch)
    model = toy_models.init_toy(toy_models.ToyBlipT5(), seed=3).eval()
    batches = toy_models.make_batches(4, seed=1)
    spec = "2-0.5-1.0-1.0"
    pruner = load_pruner("blipt5_wanda_pruner", model, batches, cfg=dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method="wanda",
                                                                         vit_pruning_method="wanda", num_samples=4, max_sparsity_per_layer=1.01))
    real = wp.BLIPT5LayerWandaPruner._prune

    def boom(self, kind, *a, **k):
        if kind.vit:
            return real(self, kind, *a, **k)
        raise RuntimeError("tower failed")
    monkeypatch.setattr(wp.BLIPT5LayerWandaPruner, "_prune", boom)
    with pytest.raises(RuntimeError, match="tower failed"):
        pruner.prune()
    assert pruner._defer_score_readback is False and not pruner.__dict__.get("_score_backlog")
    scored = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and "visual_encoder.blocks" in n
              and hasattr(m.weight, "importance_score")]
    assert len(scored) == 2 * 4                                # the ViT tower was done: its scores are there
    monkeypatch.setattr(wp.BLIPT5LayerWandaPruner, "_prune", real)


@pytest.mark.parametrize("method", ["wanda", "dsnot"])
def test_simulated_world_is_rank_0_of_w_with_its_own_rows_in_place_of_the_exchange(method, monkeypatch):
    """`VLMC_SIMULATE_WORLD=2` (bench.py --calib-local): one process captures and replays samples 0..3 of 8 and fills the
    statistics exchange with its own rows -- i.e. exactly the single-process prune of the sample list [0..3, 0..3]."""
    import toy_models
    from lavis.compression import load_pruner
    (oracle_ops.install if method == "wanda" else oracle_ops.install_dsnot)(monkeypatch)
    monkeypatch.setenv("VLMC_BATCH_REPLAY", "1")
    torch.set_num_threads(1)

    def run(batches, n):
        model = toy_models.init_toy(toy_models.ToyBlipT5(), seed=5).eval()
        spec = "2-0.5-1.0-1.0"
        cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method=method, vit_pruning_method=method, num_samples=n,
                   max_sparsity_per_layer=1.01)
        if method == "dsnot":
            cfg["max_cycle_time"] = 8
        pruned, _ = load_pruner(f"blipt5_{method}_pruner", model, batches, cfg=cfg).prune()
        return {k: v.clone() for k, v in pruned.state_dict().items()}

    eight = toy_models.make_batches(8, seed=21)
    want = run(eight[:4] + eight[:4], 8)
    monkeypatch.setenv("VLMC_SIMULATE_WORLD", "2")
    got = run(eight, 8)
    assert want.keys() == got.keys()
    for k in want:
        assert torch.equal(want[k], got[k]), k


def test_prune_freezes_the_collector_for_its_duration_only(monkeypatch):
    """calibration.quiet_gc: the objects alive at entry sit in the permanent generation while a prune runs (no full collection over
    the model's 10^5 objects in the middle of it), and are back afterwards -- also when the prune raises, not when somebody else froze."""
    import gc
    from lavis.compression.pruners import calibration as cal
    seen = []

    @cal.quiet_gc
    def outer(fail=False):
        seen.append(gc.get_freeze_count())
        inner()
        if fail:
            raise ValueError("x")
        return 7

    @cal.quiet_gc
    def inner():
        seen.append(gc.get_freeze_count())                     # nested: the outermost call owns the freeze

    assert gc.get_freeze_count() == 0
    assert outer() == 7 and seen[0] > 1000 and seen[1] >= seen[0] and gc.get_freeze_count() == 0
    with pytest.raises(ValueError):
        outer(fail=True)
    assert gc.get_freeze_count() == 0
    monkeypatch.setenv("VLMC_GC_FREEZE", "0")
    seen.clear()
    outer()
    assert seen == [0, 0]
    monkeypatch.delenv("VLMC_GC_FREEZE")
    gc.freeze()                                                # somebody else's freeze is left alone
    try:
        n = gc.get_freeze_count()
        seen.clear()
        outer()
        assert seen[0] == n and gc.get_freeze_count() == n
    finally:
        gc.unfreeze()
