"""CPU: what `lavis/compression/pruners/tower_walk.py` decides for all three layer-wise methods -- which towers a BLIP
pruner walks, in which order, which one it announces as the last, what `_done_towers` holds after each; and that a tower
that raises leaves `config.use_cache` as it found it."""
import pytest

import oracle_ops

VIT = "visual_encoder.blocks"
METHODS = ["wanda", "dsnot", "sparsegpt"]


def _towers(t5_prefix, peft, method):
    if t5_prefix == "t5_model":
        return [VIT, "t5_model.encoder.block", "t5_model.decoder.block"]
    if t5_prefix == "opt_model" and method == "sparsegpt":
        return [VIT, "opt_model.model.decoder.layers"]           # the reference SparseGPT pruner's OPT walk
    return [VIT, f"{t5_prefix}{peft}.model.layers"]


def _sequenced(method, t5_prefix, peft, **sparsity):
    """The BLIP pruner of `method` without a model, its tower step replaced by a recorder -> (pruner, calls)."""
    import lavis.compression  # noqa: F401  (registers the pruners)
    from lavis.common.registry import registry
    cls = registry.get_pruner_class(f"blipt5_{method}_pruner")
    pruner = object.__new__(cls)
    pruner.model, pruner.data_loader, pruner.num_samples = "model", "loader", 7
    pruner.vit_model_prefix, pruner.t5_model_prefix, pruner.peft_postfix = "visual_encoder", t5_prefix, peft
    calls = []

    def step(kind, model, dataloader, **kw):
        assert (model, dataloader, kw["n_samples"]) == ("model", "loader", 7)
        calls.append(dict(kw, vit=kind.vit, kind=kind, done=list(getattr(pruner, "_done_towers", [])),
                          last=pruner.__dict__.get("_proxy_cache", {}).get(("last_tower",))))
        return model
    pruner._prune = step
    pruner._prune_towers("lora", **sparsity)
    return pruner, calls


@pytest.mark.parametrize("peft", ["", ".base_model.model"])
@pytest.mark.parametrize("t5_prefix", ["t5_model", "llm_model", "opt_model"])
@pytest.mark.parametrize("method", METHODS)
def test_blip_pruners_walk_the_towers_in_order_and_mark_the_last(method, t5_prefix, peft):
    asked = []
    pruner, calls = _sequenced(method, t5_prefix, peft, vit=lambda: asked.append("vit") or "V", llm=lambda: asked.append("llm") or "L")
    want = _towers(t5_prefix, peft, method)
    assert [c["module_to_process"] for c in calls] == want
    assert [c["model_prefix"] for c in calls] == ["visual_encoder"] + [t5_prefix] * (len(want) - 1)
    assert [c["vit"] for c in calls] == [True] + [False] * (len(want) - 1)
    assert [c["kind"] for c in calls] == [pruner.vit_kind] + [pruner.llm_kind] * (len(want) - 1)
    assert [c["sparsity_ratio"] for c in calls] == ["V"] + ["L"] * (len(want) - 1)
    assert asked == ["vit", "llm"]                                # each part's sparsity dict is asked for once
    assert all(c["lora_model"] == "lora" for c in calls)
    # the finished towers, as the capture of each tower sees them, and after the last
    assert [c["done"] for c in calls] == [want[:k] for k in range(len(want))]
    assert pruner._done_towers == want
    # only the last tower's capture is told that nothing follows
    assert [c["last"] for c in calls] == [None] * (len(want) - 1) + [want[-1]]


@pytest.mark.parametrize("method", METHODS)
def test_a_part_without_sparsity_is_left_alone(method):
    pruner, calls = _sequenced(method, "t5_model", "", vit=lambda: "V", llm=None)
    assert [(c["module_to_process"], c["last"]) for c in calls] == [(VIT, VIT)] and pruner._done_towers == [VIT]
    pruner, calls = _sequenced(method, "t5_model", "", vit=None, llm=lambda: "L")
    want = _towers("t5_model", "", method)[1:]
    assert [c["module_to_process"] for c in calls] == want and [c["last"] for c in calls] == [None, want[-1]]
    assert [c["done"] for c in calls] == [[], want[:1]] and pruner._done_towers == want
    pruner, calls = _sequenced(method, "t5_model", "", vit=None, llm=None)
    assert calls == [] and not hasattr(pruner, "_done_towers")


def test_a_sparsegpt_t5_tower_that_raises_leaves_use_cache_as_it_was(monkeypatch):
    import toy_models
    from lavis.compression import load_pruner
    from lavis.compression.pruners import sparsegpt_pruner as sp
    oracle_ops.install_sparsegpt(monkeypatch)
    model = toy_models.init_toy(toy_models.ToyBlipT5(), seed=3).eval()
    batches = toy_models.make_batches(4, seed=1)
    pruner = load_pruner("t5_sparsegpt_pruner", model, batches, cfg=dict(prune_spec="2-0.5-1.0-1.0", num_samples=4,
                                                                         max_sparsity_per_layer=1.01))
    seen = []

    def boom(self, i, subset, run_pass, *a, **k):
        seen.append(model.t5_model.config.use_cache)
        raise RuntimeError("block failed")
    monkeypatch.setattr(sp.T5LayerSparseGPTPruner, "_block_step", boom)
    for before in (True, False):
        model.t5_model.config.use_cache = before
        with pytest.raises(RuntimeError, match="block failed"):
            pruner.prune()
        assert model.t5_model.config.use_cache is before
    assert seen == [False, False]                                  # the tower itself runs without key/value caches
