"""DSnoT with `initial_method="sparsegpt"` on the CPU: the restatement of the branch (dsnot_pruner.py:380-402 fed the Hessian of
sparsegpt_pruner.py:68-79) against the reference's run (tests/golden/dsnot_sgpt.npz, tests/golden/make_golden_dsnot_sgpt.py),
what the new C-ABI entry points refuse without a GPU, and the drop-in pruners with CPU stand-ins for the kernels (single process
and a sample-sharded world of two).  The GPU kernels are held against the same restatement in tests/test_dsnot_sgpt_gpu.py."""
import ctypes
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import golden_io
import oracle_ops
import pruner_helpers as PH
import toy_models
from oracle import dsnot as OD

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the golden generator's variants (tests/golden/make_golden_dsnot_sgpt.py: VARIANTS)
VARIANTS = {
    "t5bf16_2_4": dict(model="t5", dtype=torch.bfloat16, ratio=0.5, n=2, m=4, lora=False, kw=dict(max_cycle_time=4)),
    "t5fp32_u40_lora": dict(model="t5", dtype=torch.float32, ratio=0.4, n=0, m=0, lora=True,
                            kw=dict(max_cycle_time=16, update_threshold=0.02)),
    "t5fp32_u50_dead": dict(model="t5", dtype=torch.float32, ratio=0.5, n=0, m=0, lora=False, dead=True, kw=dict(max_cycle_time=20)),
    "vicuna_u50": dict(model="vicuna", dtype=torch.float32, ratio=0.5, n=0, m=0, lora=False, kw=dict(max_cycle_time=12)),
}
_G = {}


def golden():
    if not _G:
        _G.update(golden_io.load("dsnot_sgpt"))
    return _G


# ---- the restatement ------------------------------------------------------------------------------------------------------
def restated_divisor(H):
    """(diag(U) with +inf at dead columns, dead): the reference's statements :382-398 on a copy of H, torch CPU, one thread as
    the golden generator ran them (a threaded LAPACK rounds some widths differently)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _restated_divisor(H.clone())
    finally:
        torch.set_num_threads(threads)


def _restated_divisor(H):
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    damp = 0.01 * torch.mean(torch.diag(H))
    diag = torch.arange(H.shape[0])
    H[diag, diag] += damp
    H = torch.linalg.cholesky(H)
    H = torch.cholesky_inverse(H)
    H = torch.linalg.cholesky(H, upper=True)
    return torch.where(dead, torch.full_like(torch.diag(H), float("inf")), torch.diag(H)), dead


_orig_metrics = OD._metrics


def sgpt_metrics(W, stat, initial_method):
    """oracle.dsnot._metrics with the sparsegpt branch (:380-402): initial_metric = fp32(w*w) / diag(U)[c], dead columns 0."""
    if initial_method != "sparsegpt":
        return _orig_metrics(W, stat, initial_method)
    D, wanda, _ = _orig_metrics(W, stat, "wanda")
    Wf = W.float().clone()
    dead = torch.isinf(stat.divisor)
    Wf[:, dead] = 0
    return D, wanda, Wf ** 2 / torch.where(dead, torch.ones_like(stat.divisor), stat.divisor).reshape(1, -1)


def restated_prune(W, stat, ratio, n, m, **kw):
    """Keep mask (True = keep) of the DSnoT branch with the sparsegpt initial metric; `stat` carries `divisor`."""
    if n != 0:
        return ~OD.prune_nm(W, stat, n, m, initial_method="sparsegpt", **kw)
    pruned = OD.prune_unstructured(W, stat, ratio, initial_method="sparsegpt", **kw)
    return None if pruned is None else ~pruned


@pytest.fixture
def sgpt_oracle(monkeypatch):
    monkeypatch.setattr(OD, "_metrics", sgpt_metrics)


def golden_hessian(G, p):
    t = G[f"{p}/H_triu"]
    n = int(round(((8 * t.numel() + 1) ** 0.5 - 1) / 2))
    H = torch.zeros((n, n))
    iu = torch.triu_indices(n, n)
    H[iu[0], iu[1]] = t
    H[iu[1], iu[0]] = t
    return H


def build_model(v, device="cpu"):
    if v["model"] == "t5":
        model = toy_models.init_toy(toy_models.ToyBlipT5(vit_dtype=torch.float32, t5_dtype=v["dtype"]), seed=7)
        batches = toy_models.make_batches(6, seed=11)
    else:
        torch.manual_seed(0)
        model = toy_models.init_toy(toy_models.ToyBlipVicuna(llm_dtype=v["dtype"]), seed=5)
        batches = toy_models.make_batches(6, seed=13)
    if v.get("dead"):
        norm = model.visual_encoder.blocks[0].norm1
        norm.weight.data[3] = 0
        norm.bias.data[3] = 0
    if v["lora"]:
        PH.wrap_lora(model)
    model.eval().to(device)
    return model, [{k: t.to(device) for k, t in b.items()} for b in batches]


def run_pruner(name, device="cpu", **extra):
    from lavis.compression import load_pruner
    v = VARIANTS[name]
    model, batches = build_model(v, device)
    spec = "2-%r-1.0-1.0" % (1 - v["ratio"])
    cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method="dsnot", vit_pruning_method="dsnot", num_samples=6,
               prune_n=v["n"], prune_m=v["m"], max_sparsity_per_layer=1.01, initial_method="sparsegpt", **v["kw"], **extra)
    if v["model"] == "vicuna":
        cfg["t5_model_prefix"] = "llm_model"
    weights0 = {mn: mod.weight.data.clone() for mn, mod in model.named_modules() if isinstance(getattr(mod, "weight", None), torch.Tensor)}
    pruned, _ = load_pruner("blipt5_dsnot_pruner", model, batches, cfg=cfg).prune(lora_model=v["lora"])
    return pruned, weights0


def linears(name):
    G = golden()
    pre = f"{name}/lin/"
    return sorted({k[len(pre):].rsplit("/", 1)[0] for k in G if k.startswith(pre)})


def source(G, name, mn):
    """Key prefix holding the shared per-input data (H, divU, stats) of linear `mn`."""
    p = f"{name}/lin/{mn}"
    return f"{name}/lin/{G[p + '/shares']}" if f"{p}/shares" in G else p


def expected_weight(G, name, mn, W0):
    mask = G[f"{name}/lin/{mn}/mask"]
    if VARIANTS[name]["lora"]:
        return W0
    W = torch.zeros_like(W0)
    W[mask] = G[f"{name}/lin/{mn}/Wn_kept"]
    return W


# ---- the restatement reproduces the reference's run --------------------------------------------------------------------------
def test_golden_has_a_dead_column_and_every_variant():
    G = golden()
    for name in VARIANTS:
        assert linears(name), name
    dead = [k for k in G if k.endswith("/H_triu") and bool((torch.diag(golden_hessian(G, k[:-7])) == 0).any())]
    assert dead and any(k.replace("/H_triu", "/xs") in G for k in dead)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_restatement_reproduces_reference_divisor_masks_and_weights(name, sgpt_oracle):
    """Fed each golden H and the golden statistics, the restated branch gives the golden diag(U), masks and weights bit for bit."""
    G = golden()
    v = VARIANTS[name]
    model, _ = build_model(v)
    mods = dict(model.named_modules())
    n_lin = 0
    for mn in linears(name):
        src = source(G, name, mn)
        H = golden_hessian(G, src)
        div, dead = restated_divisor(H)
        assert torch.equal(div[~dead], G[f"{src}/divU"][~dead]), mn
        st = G[f"{src}/stats"]
        stat = OD.DSnoTStat(H.shape[0])
        stat.scaler_row, stat.sum_metric_row, stat.var = st[0].clone(), st[1].clone(), st[2].reshape(-1, 1).clone()
        stat.divisor = div
        W0 = mods[mn].weight.data.clone()
        keep = restated_prune(W0, stat, v["ratio"], v["n"], v["m"], **{k: val for k, val in v["kw"].items()})
        assert torch.equal(keep, G[f"{name}/lin/{mn}/mask"]), mn
        Wn = W0.clone() if v["lora"] else W0.masked_fill(~keep, 0)
        assert torch.equal(Wn, expected_weight(G, name, mn, W0)), mn
        n_lin += 1
    assert n_lin >= 10


# ---- C ABI: refusals before the device is touched ------------------------------------------------------------------------------
def test_new_exports_refuse_bad_arguments_without_a_gpu():
    from vlmc import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(1 << 20)          # 16-byte aligned, never dereferenced: every call below is refused first
    sel = lambda table, kind, mode, in_f, k, n, m: lib.vlmc_dsnot_initial_select(
        P, _lib.F16, 64, in_f, in_f, table, kind, mode, k, n, m, P, None)
    assert sel(None, _lib.DSNOT_INIT_SPARSEGPT, _lib.SEL_ROW, 256, 128, 0, 0) == _lib.VLMC_EINVAL           # NULL divisor
    assert sel(P, 7, _lib.SEL_ROW, 256, 128, 0, 0) == _lib.VLMC_EINVAL                                        # unknown kind
    assert sel(P, _lib.DSNOT_INIT_MAGNITUDE, _lib.SEL_ROW, 256, 128, 0, 0) == _lib.VLMC_EINVAL                # (unit table + WANDA)
    assert sel(P, _lib.DSNOT_INIT_SPARSEGPT, _lib.SEL_MATRIX, 256, 128, 0, 0) == _lib.VLMC_EINVAL             # no matrix rule
    assert sel(P, _lib.DSNOT_INIT_SPARSEGPT, _lib.SEL_ROW, 16392, 128, 0, 0) == _lib.VLMC_EINVAL              # in > 16384
    assert sel(P, _lib.DSNOT_INIT_SPARSEGPT, _lib.SEL_NM, 264, 0, 2, 16) == _lib.VLMC_EINVAL                  # in % m != 0
    assert sel(P, _lib.DSNOT_INIT_SPARSEGPT, _lib.SEL_NM, 260, 0, 2, 4) == _lib.VLMC_EINVAL                   # in % 8 != 0
    assert b"vlmc_dsnot_initial_select" in lib.vlmc_last_error()

    ref = lambda kind, div, in_f, n, m: lib.vlmc_dsnot_refine_kind(
        P, _lib.F16, 64, in_f, in_f, P, P, P, P, kind, div, n, m, 20, ctypes.c_float(0.1), ctypes.c_float(1.0), 1, P, P, None)
    assert ref(_lib.DSNOT_INIT_SPARSEGPT, None, 256, 0, 0) == _lib.VLMC_EINVAL                                # NULL divisor
    assert ref(3, P, 256, 0, 0) == _lib.VLMC_EINVAL                                                           # unknown kind
    assert ref(_lib.DSNOT_INIT_SPARSEGPT, P, 16392, 0, 0) == _lib.VLMC_EINVAL                                 # in > 16384
    assert ref(_lib.DSNOT_INIT_SPARSEGPT, P, 264, 2, 16) == _lib.VLMC_EINVAL                                  # in % m != 0
    assert ref(_lib.DSNOT_INIT_SPARSEGPT, P, 256, 2, 3) == _lib.VLMC_EINVAL                                   # m not in {2,4,8}
    assert lib.vlmc_dsnot_divisor(None, 64, 64, P, P, None) == _lib.VLMC_EINVAL
    assert lib.vlmc_dsnot_divisor(P, 64, 32, P, P, None) == _lib.VLMC_EINVAL
    assert lib.vlmc_dsnot_divisor(P, 64, 64, P, None, None) == _lib.VLMC_EINVAL


# ---- the drop-in pruners with CPU stand-ins ------------------------------------------------------------------------------------
def cpu_divisors(hessians, percdamp=0.01):
    return [restated_divisor(H)[0] for H in hessians]


def cpu_prune_linear(weight, stat, ratio, *, prune_n=0, prune_m=0, initial_method="wanda", without_DSnoT=False,
                     max_cycle_time=100, update_threshold=0.1, pow_of_var_regrowing=1.0, without_same_sign=True, apply_zero=True):
    """oracle_ops.oracle_dsnot_prune_linear with the restated metric and the statistic's divisor."""
    assert initial_method == "sparsegpt" and stat.divisor is not None
    ost = oracle_ops._ostat(stat)
    ost.divisor = stat.divisor
    kw = dict(max_cycle_time=max_cycle_time, update_threshold=update_threshold, pow_of_var_regrowing=pow_of_var_regrowing)
    if prune_n != 0:
        keep = ~OD.prune_nm(weight.data, ost, prune_n, prune_m, initial_method="sparsegpt", **kw)
    else:
        pruned = OD.prune_unstructured(weight.data, ost, ratio, initial_method="sparsegpt", without_DSnoT=without_DSnoT,
                                       without_same_sign=without_same_sign, **kw)
        if pruned is None:
            return None
        keep = ~pruned
    if apply_zero:
        weight[~keep] = 0
    return keep


def install_cpu(mp_):
    from vlmc import dsnot
    oracle_ops.install_dsnot(mp_)
    oracle_ops.install_sparsegpt(mp_)
    mp_.setattr(dsnot, "sparsegpt_divisors", cpu_divisors)
    mp_.setattr(dsnot, "prune_linear", cpu_prune_linear)
    mp_.setattr(OD, "_metrics", sgpt_metrics)


def check_against_golden(name, pruned, weights0, exact=True):
    G = golden()
    mods = dict(pruned.named_modules())
    agree = tot = 0
    for mn in linears(name):
        keep = mods[mn].mask.cpu()
        ref = G[f"{name}/lin/{mn}/mask"]
        agree += int((keep == ref).sum())
        tot += ref.numel()
        if exact:
            assert torch.equal(keep, ref), mn
            assert torch.equal(mods[mn].weight.data.cpu(), expected_weight(G, name, mn, weights0[mn].cpu())), mn
    return agree / tot


@pytest.mark.parametrize("name", list(VARIANTS))
def test_pruner_with_cpu_stand_ins_matches_reference_run(name, monkeypatch):
    """blipt5_dsnot_pruner(initial_method="sparsegpt") -- ViT, T5 encoder / decoder or the Vicuna llm_model branch, lora_model
    both ways -- with the kernels replaced by CPU stand-ins: the Hessians (oracle recurrence), divisors, masks and weights of
    the reference's run, bit for bit."""
    install_cpu(monkeypatch)
    pruned, w0 = run_pruner(name)
    assert check_against_golden(name, pruned, w0) == 1.0
    for mod in pruned.modules():
        if hasattr(mod, "mask") and hasattr(mod, "weight"):
            assert not hasattr(mod.weight, "importance_score")


def test_tower_pruners_accept_sparsegpt_init(monkeypatch):
    """t5_dsnot_pruner takes initial_method="sparsegpt" on its own and equals the BLIP pruner with the ViT left dense (the ViT
    tower's own class is the BLIP pruner's first step, covered by the golden runs above)."""
    from lavis.compression import load_pruner
    install_cpu(monkeypatch)
    v = VARIANTS["t5fp32_u50_dead"]
    common = dict(prune_spec="2-0.5-1.0-1.0", num_samples=6, max_cycle_time=20, initial_method="sparsegpt", max_sparsity_per_layer=1.01)
    model, batches = build_model(v)
    a, _ = load_pruner("t5_dsnot_pruner", model, batches, cfg=dict(common, model_prefix="t5_model")).prune()
    model, batches = build_model(v)
    b, _ = load_pruner("blipt5_dsnot_pruner", model, batches,
                       cfg=dict(t5_prune_spec="2-0.5-1.0-1.0", vit_prune_spec="2-1.0-1.0-1.0", t5_pruning_method="dsnot",
                                vit_pruning_method="dsnot", num_samples=6, max_cycle_time=20, initial_method="sparsegpt",
                                max_sparsity_per_layer=1.01)).prune()
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    assert sum(hasattr(m, "mask") for m in a.modules()) == 2 * 7 + 2 * 11


def test_wanda_route_builds_no_hessian(monkeypatch):
    """The other initial methods accumulate no Hessian (no launches, no memory)."""
    from lavis.compression.pruners import dsnot_pruner as DP
    from vlmc import sparsegpt
    oracle_ops.install_dsnot(monkeypatch)

    def boom(*a, **k):
        raise AssertionError("a Hessian accumulator was created on the wanda route")
    monkeypatch.setattr(sparsegpt, "SparseGPT", boom)
    pruned, _ = PH.run_dsnot_pruner("fp32_r50", "cpu")
    assert any(hasattr(m, "mask") for m in pruned.modules())
    assert DP.DsnotStatCollector({}, hessians=False).hessians is None


def test_simulated_world_is_refused(monkeypatch):
    monkeypatch.setenv("VLMC_SIMULATE_WORLD", "2")
    install_cpu(monkeypatch)
    with pytest.raises(RuntimeError, match="VLMC_SIMULATE_WORLD"):
        with pytest.warns(RuntimeWarning):
            run_pruner("t5fp32_u50_dead")


# ---- sample-sharded world of two (gloo) ---------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "vlm-compression_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    import test_dsnot_sgpt as T

    class MP:
        @staticmethod
        def setattr(obj, name, val):
            setattr(obj, name, val)
    T.install_cpu(MP)
    pruned, w0 = T.run_pruner("t5fp32_u50_dead")
    torch.save({mn: m.mask for mn, m in pruned.named_modules() if hasattr(m, "mask") and torch.is_tensor(m.mask)},
               os.path.join(out_dir, f"masks_{rank}.pt"))
    torch.save(T.check_against_golden("t5fp32_u50_dead", pruned, w0, exact=False), os.path.join(out_dir, f"agree_{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_sample_sharded_world2_tracks_reference_golden(tmp_path):
    """Each rank accumulates the Hessian and the statistics of its samples; the Hessians are exchanged as the SparseGPT pruner
    exchanges them (the sample-weighted mean), the statistics as DSnoT's.  The Hessian's sum order differs from the sequential
    running mean, so the ranks agree bit for bit with each other and the masks track the reference's single-process run."""
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    m0, m1 = torch.load(tmp_path / "masks_0.pt"), torch.load(tmp_path / "masks_1.pt")
    assert m0.keys() == m1.keys() and all(torch.equal(m0[k], m1[k]) for k in m0)
    agree = torch.load(tmp_path / "agree_0.pt")
    print(f"world-2 mask agreement with the reference run: {agree:.5f}")
    assert agree >= 0.98
