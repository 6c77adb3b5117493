"""GPU: DSnoT and SparseGPT over ragged calibration text forwarded as ONE padded group per block pass.

* `vlmc_act_moments_lens` (per-call token counts) and `vlmc_hessian_accum_rows` (a row map) through the C ABI, bit for bit against
  their unpadded siblings on each sample alone / on the compacted rows, with NaN in every padding row: a row that is read shows.
* Whole ragged prunes: DSnoT with the padded walk == the groups of equal shape (`VLMC_DSNOT_PAD=0`) == groups of 3 == the per-sample
  loop, bit for bit; SparseGPT and DSnoT with the SparseGPT initial metric against their CPU restatements within the project's
  tolerances (tests/test_sparsegpt_vicuna_gpu.py, tests/test_dsnot_sgpt_gpu.py); the samples really were padded.
* One LLaMA layer at Vicuna-7B width: the DSnoT statistics of its 7 linears from the padded group equal the per-sample forwards'."""
import contextlib
import ctypes
from types import SimpleNamespace

import pytest
import torch

import toy_llama_ops as TL
import toy_models

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _nan_padded(samples, padded, row_stride, call_stride):
    """[T_j, in] samples -> one strided buffer [calls, padded, in] (row / call pitch in elements) whose every other element is NaN"""
    n, in_f = len(samples), samples[0].shape[1]
    buf = torch.full((n * call_stride,), float("nan"), dtype=samples[0].dtype, device=DEV)
    view = buf.as_strided((n, padded, in_f), (call_stride, row_stride, 1))
    for c, s in enumerate(samples):
        view[c, :s.shape[0]] = s
    return buf, view


# ---- 5. vlmc_act_moments_lens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_f", [1408, 4096, 11008])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
def test_moments_with_lengths_give_every_sample_the_bits_of_its_own_launch(dtype, in_f):
    """1 .. 6 calls, lengths from 1 to the padded length (53: the kernel's chains take 16 tokens at a time, then one by one), rows and
    calls strided, NaN behind every sample's own rows."""
    from vlmc import _lib, ops
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(in_f)
    padded = 53
    for calls in range(1, 7):
        lens = [1, padded, 17, 32, 16, 33][:calls] if calls % 2 else \
            [int(t) for t in torch.randint(1, padded + 1, (calls,), generator=g, device=DEV).cpu()]
        samples = [(torch.randn(t, in_f, generator=g, device=DEV) * 0.7 + 0.2).to(dtype) for t in lens]
        row_stride, call_stride = in_f + 64, (padded + 3) * (in_f + 64)
        _buf, view = _nan_padded(samples, padded, row_stride, call_stride)
        ct = torch.tensor(lens, dtype=torch.int32, device=DEV)
        out = torch.full((3, calls, in_f), float("nan"), dtype=torch.float32, device=DEV)
        _lib.check(lib.vlmc_act_moments_lens(view.data_ptr(), ops._dtype_code(view), calls, padded, in_f, row_stride, call_stride,
                                             ct.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ops._stream()))
        for c, s in enumerate(samples):
            one = torch.empty((3, in_f), dtype=torch.float32, device=DEV)
            _lib.check(lib.vlmc_act_moments(s.data_ptr(), ops._dtype_code(s), 1, s.shape[0], in_f, in_f, 0, one[0].data_ptr(),
                                            one[1].data_ptr(), one[2].data_ptr(), ops._stream()))
            assert bool(torch.isfinite(one).all())
            assert torch.equal(out[:, c], one), (dtype, in_f, calls, c, lens)
        # NULL lengths: the old export; a count above the padded length is the padded length
        full = [(torch.randn(padded, in_f, generator=g, device=DEV) * 0.5).to(dtype) for _ in range(calls)]
        _buf2, view2 = _nan_padded(full, padded, row_stride, call_stride)
        want, got, over = (torch.empty((3, calls, in_f), dtype=torch.float32, device=DEV) for _ in range(3))
        big = torch.full((calls,), padded + 9, dtype=torch.int32, device=DEV)
        args = (view2.data_ptr(), ops._dtype_code(view2), calls, padded, in_f, row_stride, call_stride)
        _lib.check(lib.vlmc_act_moments(*args, want[0].data_ptr(), want[1].data_ptr(), want[2].data_ptr(), ops._stream()))
        _lib.check(lib.vlmc_act_moments_lens(*args, None, got[0].data_ptr(), got[1].data_ptr(), got[2].data_ptr(), ops._stream()))
        _lib.check(lib.vlmc_act_moments_lens(*args, big.data_ptr(), over[0].data_ptr(), over[1].data_ptr(), over[2].data_ptr(), ops._stream()))
        assert torch.equal(got, want) and torch.equal(over, want)


def test_moments_wrapper_takes_lengths_and_rejects_an_empty_sample():
    from vlmc import dsnot
    g = torch.Generator(device=DEV).manual_seed(2)
    lens = [5, 9, 7]
    samples = [(torch.randn(t, 1408, generator=g, device=DEV)).half() for t in lens]
    _buf, view = _nan_padded(samples, 16, 1408, 16 * 1408)
    ct = torch.tensor(lens, dtype=torch.int32, device=DEV)
    got = dsnot.act_moments_calls(view, 3, call_tokens=ct)
    for c, s in enumerate(samples):
        assert torch.equal(got[:, c], dsnot.act_moments(s[None]))
    st = dsnot.DsnotInputStat(1408, torch.device(DEV))
    st.add_calls(view, 3, [0, 1, 2], call_tokens=ct, host_tokens=lens)
    st.finalize()
    assert st.ntokens == sum(lens) and st.nsamples == 3 and bool(torch.isfinite(st.var_row).all())
    with pytest.raises(ValueError, match="token counts"):
        dsnot.DsnotInputStat(1408, torch.device(DEV)).add_calls(view, 3, [0, 1, 2], call_tokens=ct, host_tokens=[5, 0, 7])


# ---- 6. vlmc_hessian_accum_rows -------------------------------------------------------------------------------------------------
def _accum(lib, x, rows_total, in_f, ldx, row_map, n_rows, H, alpha, beta):
    """row_map False: the sibling `vlmc_hessian_accum` on the contiguous matrix x [n_rows, in]"""
    from vlmc import _lib, ops
    code = ops._dtype_code(x)
    need = lib.vlmc_hessian_workspace(code, n_rows, in_f)                    # sized by the REAL rows
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    if row_map is False:
        _lib.check(lib.vlmc_hessian_accum(x.data_ptr(), code, n_rows, in_f, ldx, H.data_ptr(), H.stride(0), ctypes.c_float(alpha),
                                          ctypes.c_float(beta), ws.data_ptr(), need, ops._stream()))
    else:
        _lib.check(lib.vlmc_hessian_accum_rows(x.data_ptr(), code, rows_total, in_f, ldx, None if row_map is None else row_map.data_ptr(),
                                               n_rows, H.data_ptr(), H.stride(0), ctypes.c_float(alpha), ctypes.c_float(beta), ws.data_ptr(),
                                               need, ops._stream()))
    torch.cuda.synchronize()


# (lengths, padded length): 1, 21, 605, 193 and 2273 real rows -- a single one, counts that are not multiples of the K steps (32 / 64),
# and one that the SYRK splits into two slabs along the rows at in = 1408 / 2048
_ROWS = (([1], 8), ([5, 9, 7], 16), ([44, 176, 60, 97, 176, 52], 176), ([63, 64, 65, 1], 72), ([300] * 7 + [173], 301))
HESSIAN_CASES = [(in_f, lens, tp) for in_f in (1408, 2048, 5120) for lens, tp in _ROWS] + [(11008, [44, 176, 60, 97], 176)]


@pytest.mark.parametrize("in_f,lens,tp", HESSIAN_CASES, ids=[f"in{c[0]}-rows{sum(c[1])}" for c in HESSIAN_CASES])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
def test_hessian_over_a_row_map_equals_the_hessian_of_the_compacted_rows(dtype, in_f, lens, tp):
    """alpha zero (H holds NaN and must not be read) and non-zero; every padding row of X is NaN; against fp64 within the 1e-5 of
    tests/test_gemm_gpu.py::test_hessian_accum_matches_fp64."""
    from vlmc import _lib, ops
    from lavis.compression.pruners import replay_padding as rp
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(in_f + len(lens))
    n_rows, rows_total = sum(lens), len(lens) * tp
    ldx = in_f + 8
    x = torch.full((rows_total, ldx), float("nan"), dtype=dtype, device=DEV)
    real = torch.cat([torch.arange(t) + c * tp for c, t in enumerate(lens)]).to(DEV)
    x[real, :in_f] = (torch.randn(n_rows, in_f, generator=g, device=DEV) * 0.6 + 0.2).to(dtype)
    row_map, n_real = rp.row_map(lens, tp, DEV)
    assert n_real == n_rows and torch.equal(row_map[:n_rows].long(), real)
    compact = x[real, :in_f].contiguous()
    ref64 = compact.double().t() @ compact.double()
    H0 = torch.randn(in_f, in_f, generator=g, device=DEV)
    low = torch.ones(in_f, in_f, dtype=torch.bool, device=DEV).tril()        # (both maintain the tiles on and below the diagonal)
    for alpha, beta in ((0.0, 2.0 / len(lens)), (0.75, 0.25)):
        start = torch.full((in_f, in_f), float("nan"), device=DEV) if alpha == 0.0 else H0
        got, want = start.clone(), start.clone()
        _accum(lib, x, rows_total, in_f, ldx, row_map, n_rows, got, alpha, beta)
        _accum(lib, compact, n_rows, in_f, in_f, False, n_rows, want, alpha, beta)
        assert bool(torch.isfinite(got[low]).all()), "a padding row was read"
        assert torch.equal(got[low], want[low]), (dtype, in_f, lens, alpha)
        if alpha == 0.0:
            ops.symmetrize_lower(got)
            err = float((got.double() - beta * ref64).abs().max() / (beta * ref64).abs().max())
            print(f"hessian rows {dtype} in={in_f} rows={n_rows}: max error against fp64 {err:.2e}")
            assert err < 1e-5
    # NULL map = the identity = the sibling
    ident, sib = (torch.zeros(in_f, in_f, device=DEV) for _ in range(2))
    _accum(lib, compact, n_rows, in_f, in_f, None, n_rows, ident, 0.0, 1.0)
    _accum(lib, compact, n_rows, in_f, in_f, False, n_rows, sib, 0.0, 1.0)
    assert torch.equal(ident, sib)


def test_hessian_rows_in_four_slabs_and_through_the_accumulator():
    """4096 real rows at in = 1408: the SYRK splits into four slabs along the rows -- of the GATHERED operand; and
    `SparseGPT.add_batch(x, rows=...)` counts the samples of the call and never reads a padding row."""
    from vlmc import _lib, sparsegpt
    from lavis.compression.pruners import replay_padding as rp
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(11)
    lens, tp, in_f = [128] * 31 + [64, 64], 130, 1408
    x = torch.full((len(lens), tp, in_f), float("nan"), dtype=torch.float16, device=DEV)
    for c, t in enumerate(lens):
        x[c, :t] = (torch.randn(t, in_f, generator=g, device=DEV) * 0.5).half()
    rows = rp.row_map(lens, tp, DEV)
    compact = x.reshape(-1, in_f)[rows[0][:rows[1]].long()].contiguous()
    got, want = (torch.zeros(in_f, in_f, device=DEV) for _ in range(2))
    _accum(lib, x, len(lens) * tp, in_f, in_f, rows[0], rows[1], got, 0.0, 1.0)
    _accum(lib, compact, rows[1], in_f, in_f, False, rows[1], want, 0.0, 1.0)
    assert rows[1] == 4096 and torch.equal(got, want) and bool(torch.isfinite(got).all())
    lin = torch.nn.Linear(in_f, 8, bias=False).to(DEV).half()
    a, b = sparsegpt.SparseGPT(lin), sparsegpt.SparseGPT(lin)
    a.add_batch(x, None, rows=rows)
    b._accumulate(compact, 0.0, 2.0 / len(lens))                            # the same update on the compacted rows
    assert a.nsamples == len(lens) and a.factor_cache["rows_seen"] == 4096
    assert torch.equal(a.H, b.H) and bool(torch.isfinite(a.H).all())


def test_hessian_rows_refuses_what_the_grid_cannot_hold():
    from vlmc import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(64)                                                 # (never dereferenced: the arguments are refused first)
    one, big = ctypes.c_float(1.0), 16 * 65535 + 8
    assert lib.vlmc_hessian_accum_rows(P, _lib.F16, 64, big, big, None, 64, P, big, one, one, P, 1 << 40, None) == _lib.VLMC_EINVAL
    assert b"launch grid" in lib.vlmc_last_error()
    assert lib.vlmc_hessian_accum_rows(P, _lib.F16, 64, 128, 128, None, 65, P, 128, one, one, P, 1 << 40, None) == _lib.VLMC_EINVAL
    assert lib.vlmc_hessian_accum_rows(P, _lib.F16, 64, 128, 128, None, 0, P, 128, one, one, P, 1 << 40, None) == _lib.VLMC_EINVAL


# ---- 7. whole ragged prunes -----------------------------------------------------------------------------------------------------
def _state(pruned):
    sd = {k: v.clone() for k, v in pruned.state_dict().items()}
    for n, m in pruned.named_modules():
        if hasattr(m, "mask") and torch.is_tensor(m.mask):
            sd[n + ".mask*"] = m.mask.clone()
    return sd


def _toy(lora, dtype=torch.float16, n_samples=8):
    """the ragged toy that pads: toy_llama_ops (the reference's LLaMA layer with its additive masks).  pruner_helpers.run_16bit_toy's T5 toy
    hands its blocks no mask, so its ragged samples are grouped by shape on every route: nothing of this change reaches it, and
    tests/test_replay_invariance_gpu.py keeps it; the padded T5 route is the cross-attention test below."""
    import pruner_helpers as H
    model = toy_models.init_toy(TL.ToyBlipVicunaOps(vit_dtype=torch.float16, llm_dtype=dtype), seed=7)
    batches = TL.make_batches(n_samples, True, seed0=100)
    if lora:
        H.wrap_lora(model)
    return model.eval().to(DEV), [{k: t.to(DEV) for k, t in b.items()} for b in batches]


_SWITCHES = ("VLMC_BATCH_REPLAY", "VLMC_TOWER_BATCH", "VLMC_DSNOT_PAD", "VLMC_SGPT_PAD")
PER_SAMPLE = {"VLMC_BATCH_REPLAY": "1", "VLMC_TOWER_BATCH": "0"}


def _prune(method, lora, nm, monkeypatch, env, dtype=torch.float16, **extra):
    from lavis.compression import load_pruner
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model, batches = _toy(lora, dtype)
    spec = "2-0.5-1.0-1.0"
    cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method=method, vit_pruning_method=method, num_samples=len(batches),
               max_sparsity_per_layer=1.01, prune_n=nm[0], prune_m=nm[1], t5_model_prefix="llm_model", **extra)
    if method == "dsnot":
        cfg.setdefault("max_cycle_time", 8)
    pruned, _ = load_pruner(f"blipt5_{method}_pruner", model, batches, cfg=cfg).prune(lora_model=lora)
    return pruned


@pytest.mark.parametrize("lora", [False, True], ids=["prune", "lora_model"])
@pytest.mark.parametrize("nm", [(0, 0), (2, 4)], ids=["u50", "2_4"])
@pytest.mark.parametrize("initial_method", ["wanda", "magnitude"])
def test_ragged_dsnot_prune_is_identical_padded_grouped_and_per_sample(initial_method, nm, lora, monkeypatch):
    from vlmc import forward
    from lavis.compression.pruners import calibration
    kw = dict(initial_method=initial_method)
    lens0, pad0 = forward.stats["attn_fused_lens"], calibration.graph_stats.get("padded_forwards", 0)
    on = _state(_prune("dsnot", lora, nm, monkeypatch, {}, **kw))
    grew = forward.stats["attn_fused_lens"] - lens0, calibration.graph_stats.get("padded_forwards", 0) - pad0
    assert grew[0] > 0 and grew[1] == 2 * TL.DEPTH, f"ragged samples were not padded into one group per block pass: {grew}"
    pad1 = calibration.graph_stats.get("padded_forwards", 0)
    off = _state(_prune("dsnot", lora, nm, monkeypatch, {"VLMC_DSNOT_PAD": "0"}, **kw))
    assert calibration.graph_stats.get("padded_forwards", 0) == pad1, "VLMC_DSNOT_PAD=0 must forward groups of equal shape"
    three = _state(_prune("dsnot", lora, nm, monkeypatch, {"VLMC_BATCH_REPLAY": "3"}, **kw))
    loop = _state(_prune("dsnot", lora, nm, monkeypatch, PER_SAMPLE, **kw))
    n_masks = sum(k.endswith(".mask*") and ("layers." in k or "block" in k) for k in on)
    assert n_masks == 2 * 4 + TL.DEPTH * 7
    for other, name in ((off, "switch off"), (three, "groups of 3"), (loop, "per-sample loop")):
        assert other.keys() == on.keys()
        bad = [k for k in on if not torch.equal(on[k], other[k])]
        assert not bad, f"{name}: {len(bad)} tensors differ, e.g. {bad[:4]}"


@pytest.mark.parametrize("nm", [(0, 0), (2, 4)], ids=["u50", "2_4"])
def test_ragged_dsnot_prune_with_a_cross_attention_is_identical_padded_grouped_and_per_sample(nm, monkeypatch):
    """The T5 stand-in on the reference's op sequence (extended masks): its decoder's cross-attention k / v hooks see the ENCODER's padded
    length, whose per-sample counts are not the decoder's own."""
    from vlmc import synthetic
    from lavis.compression.pruners import calibration
    dev = torch.device(DEV)

    def run(env):
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        torch.manual_seed(0)
        model = synthetic.InstructBlipT5(vit_dim=64, vit_hidden=128, vit_heads=4, vit_depth=2, d_model=64, d_ff=128, heads=4, d_kv=16,
                                         enc_depth=2, dec_depth=2, vocab=100, query_tokens=4, reference_ops=True, qformer_dim=64,
                                         qformer_heads=4, qformer_hidden=128, qformer_depth=2, qformer_vocab=50).to(dev).eval()
        batches = synthetic.calibration_batches(16, dev, vit_tokens=9, vit_dim=64, vocab=100, ragged=True)
        p0 = calibration.graph_stats.get("padded_forwards", 0)
        synthetic.time_prune(dev, pruner_name="blipt5_dsnot_pruner", n_samples=16, model=model, batches=batches,
                             t5_prune_spec="2-0.5-1.0-1.0", max_cycle_time=8, prune_n=nm[0], prune_m=nm[1])
        return {n: (m.weight.detach().clone(), m.mask.clone()) for n, m in model.named_modules()
                if isinstance(m, torch.nn.Linear) and (".block." in n or ".blocks." in n)}, calibration.graph_stats.get("padded_forwards", 0) - p0
    on, n_on = run({})
    off, n_off = run({"VLMC_DSNOT_PAD": "0"})
    loop, _ = run(PER_SAMPLE)
    assert n_on == 2 * 2 * 2 and n_off == 0, (n_on, n_off)                  # two towers, two passes, two blocks: ONE forward each
    assert on.keys() == off.keys() == loop.keys() and len(on) == 2 * 4 + 2 * 7 + 2 * 11
    for k in on:
        for other, name in ((off, "switch off"), (loop, "per-sample loop")):
            assert torch.equal(on[k][0], other[k][0]) and torch.equal(on[k][1], other[k][1]), (k, name)


def _pattern_and_rms(got, want, nm):
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
    return agree / tot, (num / den) ** 0.5 if den else 0.0


@pytest.mark.parametrize("nm", [(0, 0), (2, 4)], ids=["u50", "2_4"])
def test_ragged_sparsegpt_prune_through_padded_groups_tracks_its_cpu_restatement(nm, monkeypatch):
    """tests/test_llama_replay_gpu.py's comparison and tolerance (pattern agreement >= 0.97, relative RMS of the weights < 2e-2 on agreeing
    rows): the padded walk against the restatement's per-sample loop.  The restatement is fp32, and fp32 activations keep the library GEMM
    (`VLMC_SGPT_SYRK_F32` is off), so THIS comparison runs the accumulator's gather-then-`addmm_` route of a padded group, not the new kernel.
    The kernel itself is pinned bit for bit by the tests above; the fp16 toy, whose Hessians do come from `vlmc_hessian_accum_rows` (counted),
    is held with the same tolerance against this build's groups of equal shape (the default, `VLMC_SGPT_PAD` unset).  The figures are printed."""
    import test_sparsegpt_vicuna as T
    from lavis.compression.pruners import calibration
    from vlmc import ops

    def weights(pruned):
        return {n: m.weight.data.float().cpu() for n, m in pruned.named_modules()
                if isinstance(m, torch.nn.Linear) and (".layers." in n or ".blocks." in n)}

    def run_cpu():
        from lavis.compression import load_pruner
        model = toy_models.init_toy(TL.ToyBlipVicunaOps(), seed=5).eval()
        batches = TL.make_batches(6, True)
        cfg = dict(t5_prune_spec="2-0.5-1.0-1.0", vit_prune_spec="2-0.5-1.0-1.0", t5_pruning_method="sparsegpt", vit_pruning_method="sparsegpt",
                   num_samples=6, prune_n=nm[0], prune_m=nm[1], max_sparsity_per_layer=1.01, t5_model_prefix="llm_model")
        return weights(load_pruner("blipt5_sparsegpt_pruner", model, batches, cfg=cfg).prune()[0])
    with monkeypatch.context() as mp:
        T.install_cpu(mp)
        mp.setenv("VLMC_BATCH_REPLAY", "1")
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            want = run_cpu()
        finally:
            torch.set_num_threads(threads)

    def run_gpu(env, dtype):
        from lavis.compression import load_pruner
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model = toy_models.init_toy(TL.ToyBlipVicunaOps(llm_dtype=dtype), seed=5).eval().to(DEV)
        batches = [{k: t.to(DEV) for k, t in b.items()} for b in TL.make_batches(6, True)]
        cfg = dict(t5_prune_spec="2-0.5-1.0-1.0", vit_prune_spec="2-0.5-1.0-1.0", t5_pruning_method="sparsegpt", vit_pruning_method="sparsegpt",
                   num_samples=6, prune_n=nm[0], prune_m=nm[1], max_sparsity_per_layer=1.01, t5_model_prefix="llm_model")
        p0 = calibration.graph_stats.get("padded_forwards", 0)
        out = weights(load_pruner("blipt5_sparsegpt_pruner", model, batches, cfg=cfg).prune()[0])
        return out, calibration.graph_stats.get("padded_forwards", 0) - p0
    padded = {"VLMC_SGPT_PAD": "1"}                                         # (opt-in: profiles/ragged_dsnot_sparsegpt.md)
    got, n_pad = run_gpu(padded, torch.float32)
    assert n_pad == 2 * TL.DEPTH, "ragged samples were not padded into one group per block pass"
    assert got.keys() == want.keys() and len(got) == 2 * 4 + TL.DEPTH * 7
    agree, rel = _pattern_and_rms(got, want, nm)
    print(f"ragged sparsegpt {nm}, padded groups against the CPU restatement: pattern agreement {agree:.5f}, relative RMS {rel:.2e}")
    assert agree >= 0.97 and rel < 2e-2
    seen = {"rows": 0}
    real = ops.hessian_accum

    def counted(H, x, alpha, beta, rows=None):
        seen["rows"] += rows is not None
        return real(H, x, alpha, beta, rows=rows)
    monkeypatch.setattr(ops, "hessian_accum", counted)
    on, n_on = run_gpu(padded, torch.float16)
    assert n_on == 2 * TL.DEPTH and seen["rows"] == 4 * TL.DEPTH, (n_on, seen)     # q/k/v, o, gate/up, down: four distinct inputs per layer
    off, n_off = run_gpu({}, torch.float16)                                 # the default: groups of equal shape
    assert n_off == 0 and seen["rows"] == 4 * TL.DEPTH
    agree, rel = _pattern_and_rms(on, off, nm)
    print(f"ragged sparsegpt {nm}, fp16, padded groups against groups of equal shape: pattern agreement {agree:.5f}, relative RMS {rel:.2e}")
    assert agree >= 0.97 and rel < 2e-2


@pytest.mark.parametrize("nm", [(0, 0), (2, 4)], ids=["u50", "2_4"])
def test_ragged_dsnot_with_the_sparsegpt_start_matches_its_restatement_linear_by_linear(nm, monkeypatch):
    """tests/test_dsnot_sgpt_gpu.py's bar on ragged text through padded groups: every linear bit-identical to the restatement fed the GPU's own
    statistics and divisor, the divisors within its DIV_RTOL of fp64 on the GPU's own H.  No reference run of this ragged toy is recorded, so
    its >= 0.99 mask agreement is held against the per-sample loop of this build instead; the figure is printed.  The Hessians of the padded
    groups are those of the groups of equal shape up to the sum order: relative error < 1e-5, what tests/test_gemm_gpu.py holds
    `vlmc_hessian_accum` to against the library's product."""
    import test_dsnot_sgpt as S
    import test_dsnot_sgpt_gpu as SG
    from oracle import dsnot as OD
    from vlmc import dsnot
    from lavis.compression.pruners import calibration
    monkeypatch.setattr(OD, "_metrics", S.sgpt_metrics)
    real_prune, real_div = dsnot.prune_linear, dsnot.sparsegpt_divisors
    seen = {"linears": 0, "div_err": 0.0, "H": []}

    def divisors(hessians, percdamp=0.01):
        seen["H"] += [H.clone() for H in hessians]
        want = [SG._fp64_divisor(H.cpu()) for H in hessians]
        out = real_div(hessians, percdamp)
        for w, d in zip(want, out):
            fin = ~torch.isinf(w)
            assert torch.equal(torch.isinf(w), torch.isinf(d.cpu()))
            seen["div_err"] = max(seen["div_err"], float(((d.cpu().double()[fin] - w[fin]).abs() / w[fin]).max()))
        return out

    def checked(weight, stat, ratio, **kw):
        W0 = weight.detach().clone().cpu()
        keep = real_prune(weight, stat, ratio, **kw)
        ost = SimpleNamespace(scaler_row=stat.scaler_row.cpu(), sum_metric_row=stat.sum_row.cpu(), var=stat.var_row.cpu().reshape(-1, 1),
                              divisor=stat.divisor.cpu())
        okw = {k: kw[k] for k in ("max_cycle_time", "update_threshold", "pow_of_var_regrowing")}
        if kw["prune_n"]:
            want = ~OD.prune_nm(W0, ost, kw["prune_n"], kw["prune_m"], initial_method="sparsegpt", **okw)
        else:
            want = ~OD.prune_unstructured(W0, ost, ratio, initial_method="sparsegpt", without_DSnoT=kw["without_DSnoT"],
                                          without_same_sign=kw["without_same_sign"], **okw)
        assert torch.equal(keep.cpu(), want)
        assert torch.equal(weight.detach().cpu(), W0.masked_fill(~want, 0))
        seen["linears"] += 1
        return keep

    monkeypatch.setattr(dsnot, "prune_linear", checked)
    monkeypatch.setattr(dsnot, "sparsegpt_divisors", divisors)
    p0 = calibration.graph_stats.get("padded_forwards", 0)
    on = _state(_prune("dsnot", False, nm, monkeypatch, {}, initial_method="sparsegpt"))
    assert calibration.graph_stats.get("padded_forwards", 0) - p0 == 2 * TL.DEPTH, "ragged samples were not padded into one group"
    assert seen["linears"] == 2 * 4 + TL.DEPTH * 7 and seen["div_err"] <= SG.DIV_RTOL, seen["div_err"]
    H_on, seen["H"] = seen["H"], []
    _prune("dsnot", False, nm, monkeypatch, {"VLMC_DSNOT_PAD": "0"}, initial_method="sparsegpt")
    H_off, seen["H"] = seen["H"], []
    loop = _state(_prune("dsnot", False, nm, monkeypatch, PER_SAMPLE, initial_method="sparsegpt"))
    # four distinct inputs per block: the two ViT blocks' (never padded), then the first language layer's -- whose inputs are the same bits
    # on both routes (the later layer sees what the first one's masks made of them)
    assert len(H_on) == len(H_off) == 4 * (2 + TL.DEPTH)
    h_err = max(float((a - b).norm() / b.norm()) for a, b in zip(H_on[:12], H_off[:12]))
    worst = min(float((on[k] == loop[k]).float().mean()) for k in on if k.endswith(".mask*"))
    print(f"ragged dsnot/sparsegpt {nm}: divisor vs fp64 {seen['div_err']:.2e}; H of the padded groups vs groups of equal shape {h_err:.2e}; "
          f"worst per-linear mask agreement with the per-sample loop {worst:.5f}")
    assert h_err < 1e-5
    assert worst >= 0.99


# ---- 8. one LLaMA layer at Vicuna-7B width --------------------------------------------------------------------------------------
def test_dsnot_statistics_of_a_vicuna_width_layer_from_the_padded_group_equal_the_per_sample_forwards(monkeypatch):
    from test_llama_replay_gpu import _layer_and_samples
    from lavis.compression.pruners import calibration as cal
    from lavis.compression.pruners.dsnot_pruner import DsnotStatCollector
    from vlmc import forward
    lengths = [44, 176, 60, 97, 176, 52]
    layer, xs, caches = _layer_and_samples(lengths)
    model = SimpleNamespace(layers=torch.nn.ModuleList([layer]))

    def walk(env, pad):
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = {}

        def prune_block(i, lyr, subset, run_pass, state):
            col = DsnotStatCollector(subset)
            try:
                run_pass(col.next_sample, outputs=False)
            finally:
                col.close()
            got.update(col.finalize())
        n = len(xs)
        cal.walk_blocks(model, list(xs), [None] * n, caches, "layers", n, contextlib.nullcontext, prune_block, True, pad_ragged=pad)
        return got
    p0, l0 = cal.graph_stats.get("padded_forwards", 0), forward.stats["attn_fused_lens"]
    padded = walk({}, True)
    assert cal.graph_stats.get("padded_forwards", 0) - p0 == 2 and forward.stats["attn_fused_lens"] > l0
    single = walk(PER_SAMPLE, False)
    assert len(padded) == 7 and padded.keys() == single.keys()
    for name in padded:
        a, b = padded[name], single[name]
        assert a.nsamples == b.nsamples == 6 and a.ntokens == b.ntokens == sum(lengths), name
        ma, ta, _ = a.ordered()
        mb, tb, _ = b.ordered()
        assert ta == tb == lengths and torch.equal(ma, mb), name
        for f in ("scaler_row", "sum_row", "var_row", "sqrt_row"):
            assert torch.equal(getattr(a, f), getattr(b, f)) and bool(torch.isfinite(getattr(a, f)).all()), (name, f)
