"""CPU: DSnoT and SparseGPT walk ragged calibration text as ONE padded group per block pass -- the host logic, with the kernels
replaced by torch stand-ins that honour `call_tokens` / `rows` (tests/oracle_ops.py, extended below) and `plan_padded` made
runnable on the host as tests/test_llama_lazy_host.py's `host_padding` fixture does.

* the DSnoT collector inside a padded group gives the statistics of `oracle/dsnot.py`'s `DSnoTStat` fed the samples one by one, the
  Hessian accumulator those of the oracle's recurrence -- with NaN in every padding row;
* the DSnoT and SparseGPT pruners form ONE padded group per block pass for ragged samples, groups of equal shape with their switch off;
* world size 2 over gloo, samples sharded: DSnoT's masks are the single process's, SparseGPT tracks it;
* the two switches are registered and read through `config.flag` only."""
import math
import os
import socket
import sys

import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- stand-ins --------------------------------------------------------------------------------------------------------------------
def moments_calls(x, calls, call_tokens=None):
    """vlmc.dsnot.act_moments_calls: with lengths, call c reduces its first call_tokens[c] token rows and nothing else"""
    import oracle_ops
    x = x.reshape(calls, -1, x.shape[-1])
    if call_tokens is None:
        return torch.stack([oracle_ops.dsnot_act_moments(c) for c in x], dim=1)
    assert call_tokens.dtype == torch.int32 and call_tokens.numel() == calls
    return torch.stack([oracle_ops.dsnot_act_moments(x[c, :int(n)]) for c, n in enumerate(call_tokens.tolist())], dim=1)


def _rows_sparsegpt():
    import oracle_ops

    class RowsSparseGPT(oracle_ops.OracleSparseGPT):
        """oracle.sparsegpt.hessian_update over the rows a row map names; the call's samples are counted as ever"""

        def add_batch(self, inp, out=None, rows=None):
            if rows is None:
                return super().add_batch(inp, out)
            b = inp.shape[0]
            x = inp.reshape(-1, inp.shape[-1])[rows[0][:rows[1]].long()]
            self.H *= self.nsamples / (self.nsamples + b)
            self.nsamples += b
            xt = math.sqrt(2 / self.nsamples) * x.t().float()
            self.H += xt.matmul(xt.t())
    return RowsSparseGPT


def install(mp_):
    """`mp_.setattr(obj, name, value)`: pytest's monkeypatch, or a plain setter inside a spawned worker"""
    import oracle_ops
    oracle_ops.install(mp_)
    oracle_ops.install_dsnot(mp_)
    oracle_ops.install_sparsegpt(mp_)
    overrides(mp_)


def overrides(mp_):
    """on top of tests/oracle_ops.py's stand-ins: the two that take lengths / a row map, and `plan_padded` on the host"""
    from lavis.compression.pruners import calibration, replay_padding as rp
    from vlmc import dsnot, sparsegpt
    mp_.setattr(dsnot, "act_moments_calls", moments_calls)
    mp_.setattr(sparsegpt, "SparseGPT", _rows_sparsegpt())
    # `plan_padded` on the host (tests/test_llama_lazy_host.py: host_padding): it asks for CUDA inputs, only while it plans, and builds
    # its row maps through a pinned staging buffer
    mp_.setattr(rp, "int32_on", lambda values, device: torch.as_tensor(values, dtype=torch.int32))
    real_plan = rp.plan_padded

    def plan_padded(*a):
        saved = torch.Tensor.is_cuda
        torch.Tensor.is_cuda = property(lambda self: True)
        try:
            return real_plan(*a)
        finally:
            torch.Tensor.is_cuda = saved
    mp_.setattr(calibration, "plan_padded", plan_padded)


class _Setter:
    @staticmethod
    def setattr(obj, name, val):
        setattr(obj, name, val)


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ---- 1. the collector inside a padded group ------------------------------------------------------------------------------------------
def _group_context(lens, padded):
    from lavis.compression.pruners import replay_padding as rp
    from lavis.compression.pruners.replay_state import _CTX
    spec = {"T": list(lens), "S": [None] * len(lens), "tp": padded, "sp": None,
            "lengths": {padded: torch.tensor(lens, dtype=torch.int32)}, "rows": {(len(lens), padded): rp.row_map(lens, padded, "cpu")}}
    _CTX.stacked, _CTX.stacked_lengths, _CTX.stacked_spec = (len(lens), 1, tuple(range(len(lens)))), spec["lengths"], spec
    return _CTX


def test_collector_in_a_padded_group_gives_the_statistics_of_the_samples_one_by_one(monkeypatch, one_thread):
    from oracle import dsnot as OD, sparsegpt as OS
    from lavis.compression.pruners.dsnot_pruner import DsnotStatCollector
    install(monkeypatch)
    lens, padded, in_f = [5, 9, 7], 16, 24
    g = torch.Generator().manual_seed(3)
    samples = [torch.randn(1, t, in_f, generator=g) * 0.8 + 0.1 for t in lens]
    x = torch.full((3, padded, in_f), float("nan"))
    for c, s in enumerate(samples):
        x[c, :lens[c]] = s[0]
    lin = nn.Linear(in_f, 8, bias=False)
    col = DsnotStatCollector({"lin": lin}, hessians=True)
    ctx = _group_context(lens, padded)
    try:
        col.next_sample(0)
        with torch.no_grad():
            lin(x)
    finally:
        ctx.stacked = ctx.stacked_lengths = ctx.stacked_spec = None
        col.close()
    acc = col.hessians["lin"]
    H = acc.H.clone()
    monkeypatch.setattr(col, "_divisors", lambda stats: None)              # (the divisor's factorization is not under test here)
    st = col.finalize()["lin"]
    want = OD.DSnoTStat(in_f)
    Hw, n = torch.zeros(in_f, in_f), 0
    for s in samples:
        want.add_batch(s)
        n = OS.hessian_update(Hw, n, s)
    assert st.nsamples == want.nsamples == 3 and st.ntokens == want.ntokens == sum(lens)
    assert torch.equal(st.scaler_row, want.scaler_row) and torch.equal(st.sum_row, want.sum_metric_row)
    assert torch.allclose(st.var_row, want.var.reshape(-1), rtol=2e-6, atol=0)
    assert acc.nsamples == 3 and bool(torch.isfinite(H).all())
    assert torch.allclose(H, Hw, rtol=1e-5, atol=1e-6 * float(Hw.abs().max()))       # (one update of three samples against three updates)


def test_a_hook_input_without_lengths_inside_a_padded_group_is_refused(monkeypatch):
    from lavis.compression.pruners.dsnot_pruner import DsnotStatCollector
    install(monkeypatch)
    lin = nn.Linear(24, 8, bias=False)
    col = DsnotStatCollector({"lin": lin})
    ctx = _group_context([5, 9, 7], 16)
    try:
        col.next_sample(0)
        with torch.no_grad(), pytest.raises(RuntimeError, match="per-sample token counts"):
            lin(torch.zeros(3, 12, 24))                                    # 12 is no padded length of this group
    finally:
        ctx.stacked = ctx.stacked_lengths = ctx.stacked_spec = None
        col.close()


def test_lengths_feed_the_token_weighted_variance_and_an_empty_sample_is_refused(monkeypatch):
    from vlmc import dsnot
    install(monkeypatch)
    x = torch.randn(3, 16, 24, generator=torch.Generator().manual_seed(1))
    ct = torch.tensor([5, 9, 7], dtype=torch.int32)
    st = dsnot.DsnotInputStat(24, "cpu")
    st.add_calls(x, 3, [0, 1, 2], call_tokens=ct, host_tokens=[5, 9, 7])
    assert st.blocks[0][1] == [5, 9, 7] and st.blocks[0][2] == [1, 1, 1]   # each sample's OWN count, not b * padded tokens
    with pytest.raises(ValueError, match="token counts"):
        dsnot.DsnotInputStat(24, "cpu").add_calls(x, 3, [0, 1, 2], call_tokens=ct, host_tokens=[5, 0, 7])
    with pytest.raises(ValueError, match="one host count per call"):
        dsnot.DsnotInputStat(24, "cpu").add_calls(x, 3, [0, 1, 2], call_tokens=ct, host_tokens=None)


# ---- 2. the towers' walks ------------------------------------------------------------------------------------------------------------
def _run_toy(method, env=None, n_samples=8, **extra):
    """the ragged reference-op toy (tests/toy_llama_ops.py: additive masks, position ids) through blipt5_<method>_pruner on the stand-ins"""
    import toy_llama_ops as TL
    import toy_models
    from lavis.compression import load_pruner
    from lavis.compression.pruners import calibration
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        model = toy_models.init_toy(TL.ToyBlipVicunaOps(), seed=5).eval()
        batches = TL.make_batches(n_samples, True)
        spec = "2-0.5-1.0-1.0"
        cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method=method, vit_pruning_method=method, num_samples=n_samples,
                   t5_model_prefix="llm_model", max_sparsity_per_layer=1.01, **extra)
        p0 = calibration.graph_stats.get("padded_forwards", 0)
        pruned, _ = load_pruner(f"blipt5_{method}_pruner", model, batches, cfg=cfg).prune()
        n_pad = calibration.graph_stats.get("padded_forwards", 0) - p0
    finally:
        for k in (env or {}):
            del os.environ[k]
    out = {n: (m.weight.data.clone(), m.mask.clone() if torch.is_tensor(getattr(m, "mask", None)) else None)
           for n, m in pruned.named_modules() if isinstance(m, nn.Linear) and (".layers." in n or ".blocks." in n)}
    return out, n_pad


@pytest.mark.parametrize("method,switch", [("dsnot", "VLMC_DSNOT_PAD"), ("sparsegpt", "VLMC_SGPT_PAD")])
def test_the_towers_walk_ragged_samples_as_one_padded_group(method, switch, monkeypatch, one_thread):
    """(fails before this change: neither tower passed `pad_ragged` to `walk_blocks`).  DSnoT's switch is on by default, SparseGPT's is
    opt-in (profiles/ragged_dsnot_sparsegpt.md): the run below sets both, each `off` run clears one."""
    import toy_llama_ops as TL
    install(monkeypatch)
    kw = dict(max_cycle_time=8) if method == "dsnot" else {}
    both = {"VLMC_DSNOT_PAD": "1", "VLMC_SGPT_PAD": "1"}
    on, n_on = _run_toy(method, both, **kw)
    assert n_on == 2 * TL.DEPTH, f"{method}: {n_on} padded forwards, expected ONE per block pass"
    off, n_off = _run_toy(method, {**both, switch: "0"}, **kw)
    assert n_off == 0, f"{switch}=0 must forward groups of equal shape"
    other, n_other = _run_toy(method, {**both, "VLMC_SGPT_PAD" if method == "dsnot" else "VLMC_DSNOT_PAD": "0"}, **kw)
    assert n_other == n_on                                                 # each switch is its own method's
    assert on.keys() == off.keys() and len(on) == 2 * 4 + TL.DEPTH * 7
    if method == "dsnot":
        loop, _ = _run_toy(method, {"VLMC_BATCH_REPLAY": "1"}, **kw)
        _default, n_default = _run_toy(method, **kw)
        assert n_default == n_on                                           # DSnoT pads by default
        for k in on:
            assert torch.equal(on[k][1], off[k][1]) and torch.equal(on[k][0], off[k][0]), k
            assert torch.equal(on[k][1], loop[k][1]) and torch.equal(on[k][0], loop[k][0]), k
    else:
        agree, rel = _agreement(on, off)
        print(f"sparsegpt stand-ins, padded groups against groups of equal shape: pattern agreement {agree:.5f}, relative RMS {rel:.2e}")
        assert agree >= 0.97 and rel < 2e-2
        _default, n_default = _run_toy(method, **kw)
        assert n_default == 0                                              # SparseGPT's padded walk is opt-in


def _agreement(got, want):
    """tests/test_sparsegpt_vicuna_gpu.py's figures: zero-pattern agreement, relative RMS of the weights on the rows that agree"""
    agree = tot = 0
    num = den = 0.0
    for n in want:
        a, b = got[n][0].float(), want[n][0].float()
        same = (a == 0) == (b == 0)
        agree += int(same.sum())
        tot += same.numel()
        rows = same.all(dim=1)
        num += float((a[rows] - b[rows]).pow(2).sum())
        den += float(b[rows].pow(2).sum())
    return agree / tot, (num / den) ** 0.5 if den else 0.0


def test_dsnot_with_the_sparsegpt_start_hands_the_groups_row_map_to_its_hessians(monkeypatch, one_thread):
    import test_dsnot_sgpt as S
    import toy_llama_ops as TL
    from vlmc import sparsegpt
    S.install_cpu(monkeypatch)
    overrides(monkeypatch)                                                  # (after it: the accumulator that takes `rows`)
    seen = {"rows": 0, "plain": 0}
    base = sparsegpt.SparseGPT

    class Counting(base):
        def add_batch(self, inp, out=None, rows=None):
            seen["rows" if rows is not None else "plain"] += 1
            return super().add_batch(inp, out, rows=rows)
    monkeypatch.setattr(sparsegpt, "SparseGPT", Counting)
    on, n_on = _run_toy("dsnot", initial_method="sparsegpt", max_cycle_time=8)
    assert n_on == 2 * TL.DEPTH and seen["rows"] == 4 * TL.DEPTH, seen      # q/k/v, o, gate/up, down: four distinct inputs per layer
    off, n_off = _run_toy("dsnot", {"VLMC_DSNOT_PAD": "0"}, initial_method="sparsegpt", max_cycle_time=8)
    assert n_off == 0 and seen["rows"] == 4 * TL.DEPTH
    worst = min(float((on[k][1] == off[k][1]).float().mean()) for k in on)
    print(f"dsnot/sparsegpt stand-ins: worst per-linear mask agreement, padded groups against groups of equal shape {worst:.5f}")
    assert worst >= 0.99                                                    # tests/test_dsnot_sgpt_gpu.py's bar


# ---- 3. world size 2 -----------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist
    for p in (ROOT, os.path.join(ROOT, "vlm-compression_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import test_ragged_stats_host as me
    me.install(_Setter)
    for method, kw in (("dsnot", dict(max_cycle_time=8)), ("sparsegpt", {})):
        out, n_pad = me._run_toy(method, {"VLMC_SGPT_PAD": "1"}, **kw)
        torch.save({"out": out, "n_pad": n_pad}, os.path.join(out_dir, f"{method}_{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_sample_sharded_world2_walks_padded_groups_and_matches_the_single_process(tmp_path, monkeypatch, one_thread):
    """8 ragged samples over 2 ranks, each rank ONE padded group of its 4 (another padded length than the single process's): DSnoT's masks
    and weights are the single process's bit for bit (per-call token counts are all-gathered with the moments); SparseGPT's Hessians are
    exchanged as ever and the result tracks the single process's within the project's tolerance."""
    import toy_llama_ops as TL
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    install(monkeypatch)
    for method, kw in (("dsnot", dict(max_cycle_time=8)), ("sparsegpt", {})):
        want, n_want = _run_toy(method, {"VLMC_SGPT_PAD": "1"}, **kw)
        assert n_want == 2 * TL.DEPTH
        for r in range(2):
            got = torch.load(tmp_path / f"{method}_{r}.pt")
            assert got["n_pad"] == 2 * TL.DEPTH, (method, r, got["n_pad"])
            assert got["out"].keys() == want.keys()
            if method == "dsnot":
                for k in want:
                    assert torch.equal(got["out"][k][1], want[k][1]) and torch.equal(got["out"][k][0], want[k][0]), (r, k)
            else:
                agree, rel = _agreement(got["out"], want)
                print(f"rank {r}: sparsegpt pattern agreement with the single process {agree:.5f}, relative RMS {rel:.2e}")
                assert agree >= 0.97 and rel < 2e-2


# ---- 4. the switches -----------------------------------------------------------------------------------------------------------------
def test_the_two_switches_are_registered_and_read_through_config_flag_only(monkeypatch):
    import re
    from vlmc import config, crosscheck
    # (DSnoT's padded walk is the default, SparseGPT's is opt-in: each route names the walk that is NOT the default)
    for name, route, default in (("VLMC_DSNOT_PAD", "dsnot_equal_shapes", "1"), ("VLMC_SGPT_PAD", "sparsegpt_padded_groups", "0")):
        other = "0" if default == "1" else "1"
        monkeypatch.delenv(name, raising=False)
        assert config.CROSSCHECK[name][0] == default and config.flag(name) is (default == "1")
        assert crosscheck.ROUTES[route][0] == {name: other}
        env = {"VLMC_CROSSCHECK": route}
        assert crosscheck.apply(env) == [route] and env[name] == other
        monkeypatch.setenv(name, other)
        assert config.flag(name) is (other == "1")
    pruners = os.path.join(ROOT, "vlm-compression_amd", "lavis", "compression", "pruners")
    for f in ("dsnot_pruner.py", "sparsegpt_pruner.py", "replay_padding.py"):
        src = open(os.path.join(pruners, f)).read()
        assert not re.search(r"environ|getenv", src), f"{f} reads the environment around config.flag"
    src = open(os.path.join(pruners, "dsnot_pruner.py")).read() + open(os.path.join(pruners, "sparsegpt_pruner.py")).read()
    assert 'config.flag("VLMC_DSNOT_PAD")' in src and 'config.flag("VLMC_SGPT_PAD")' in src
