"""GPU: DSnoT with `initial_method="sparsegpt"` -- the saliency select (vlmc_dsnot_initial_select), the refinement with the third
initial-metric kind (vlmc_dsnot_refine_kind: list kernel and cycle kernel), the divisor (sparsegpt_divisors, vlmc_dsnot_divisor)
and the drop-in pruners end to end, against the CPU restatement of tests/test_dsnot_sgpt.py and the reference's run
(tests/golden/dsnot_sgpt.npz)."""
from types import SimpleNamespace

import pytest
import torch

import test_dsnot_sgpt as S
from oracle import dsnot as OD
from test_dsnot_sgpt import sgpt_oracle  # noqa: F401  (fixture: the oracle's metrics with the sparsegpt branch)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case(rows, in_f, dtype, seed, ties=False, dead=0):
    """W, sqrt(scaler), sum_row, var_row, divisor (+inf at `dead` columns) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(rows, in_f, generator=g) * 0.02
    scaler = torch.rand(in_f, generator=g) * 4 + 0.05
    div = torch.rand(in_f, generator=g) * 2 + 0.1
    if ties:                                     # tie floods: equal |w| on a third of the rows, equal divisors everywhere else
        W[: rows // 3] = torch.where(torch.rand(rows // 3, in_f, generator=g) < 0.5, 0.01, -0.01)
        div[in_f // 2:] = 0.75
        scaler[in_f // 2:] = 1.0
    if dead:
        div[torch.randperm(in_f, generator=g)[:dead]] = float("inf")
    W = W.to(dtype)
    sum_row = torch.randn(in_f, generator=g) * 0.3
    var_row = torch.rand(in_f, generator=g) + 0.05
    return W, scaler, torch.sqrt(scaler), sum_row, var_row, div


def _restated(W, scaler, sum_row, var_row, div, ratio, n, m, max_cycle):
    ost = SimpleNamespace(scaler_row=scaler, sum_metric_row=sum_row, var=var_row.reshape(-1, 1), divisor=div)
    return S.restated_prune(W, ost, ratio, n, m, max_cycle_time=max_cycle)


def _gpu(W, sq, sum_row, var_row, div, ratio, n, m, max_cycle):
    from vlmc import dsnot
    st = SimpleNamespace(sqrt_row=sq.to(DEV), sum_row=sum_row.to(DEV), var_row=var_row.to(DEV), divisor=div.to(DEV))
    Wd = W.to(DEV).contiguous()
    keep = dsnot.prune_linear(Wd, st, ratio, prune_n=n, prune_m=m, initial_method="sparsegpt", max_cycle_time=max_cycle)
    return keep.cpu(), Wd.cpu()


SHAPES = [(torch.bfloat16, w) for w in (1408, 2048, 4096, 5120, 6144, 11008)] + \
         [(torch.float16, 2048), (torch.float16, 5120), (torch.float32, 1408), (torch.float32, 4096)]


@pytest.mark.parametrize("route", ["lists", "cycles"])
@pytest.mark.parametrize("mode", ["u50", "2:4", "4:8"])
@pytest.mark.parametrize("dtype,in_f", SHAPES)
def test_select_and_refine_bit_exact_against_restatement(dtype, in_f, mode, route, monkeypatch, sgpt_oracle):
    """The initial select and the refinement (list kernel, or the cycle kernel with VLMC_DSNOT_LISTS=0) with the sparsegpt kind:
    masks and zeroed weights bit for bit against the restatement, with dead columns and tie floods."""
    if route == "cycles":
        monkeypatch.setenv("VLMC_DSNOT_LISTS", "0")
    n, m, ratio = {"u50": (0, 0, 0.5), "2:4": (2, 4, 0.5), "4:8": (4, 8, 0.5)}[mode]
    rows = 256 if in_f <= 6144 else 192
    for k, ties in enumerate((False, True) if n == 0 else (False,)):    # (n:m: the selects' tie rule is Wanda's topk order)
        W, scaler, sq, sum_row, var_row, div = _case(rows, in_f, dtype, seed=in_f + k, ties=ties, dead=5)
        want = _restated(W, scaler, sum_row, var_row, div, ratio, n, m, 100)
        keep, Wn = _gpu(W, sq, sum_row, var_row, div, ratio, n, m, 100)
        assert torch.equal(keep, want), (dtype, in_f, mode, route, ties, int((keep != want).sum()))
        assert torch.equal(Wn, W.masked_fill(~want, 0))


def test_without_dsnot_gives_the_plain_saliency_mask(sgpt_oracle):
    from vlmc import dsnot
    W, scaler, sq, sum_row, var_row, div = _case(128, 2048, torch.bfloat16, seed=9, dead=3)
    st = SimpleNamespace(sqrt_row=sq.to(DEV), sum_row=sum_row.to(DEV), var_row=var_row.to(DEV), divisor=div.to(DEV))
    keep = dsnot.prune_linear(W.to(DEV), st, 0.5, initial_method="sparsegpt", without_DSnoT=True).cpu()
    ost = SimpleNamespace(scaler_row=scaler, sum_metric_row=sum_row, var=var_row.reshape(-1, 1), divisor=div)
    assert torch.equal(keep, ~OD.prune_unstructured(W, ost, 0.5, initial_method="sparsegpt", without_DSnoT=True))


@pytest.mark.parametrize("nm", [(0, 0), (2, 4)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_old_refine_export_equals_new_export_with_the_same_kind(nm, dtype):
    """vlmc_dsnot_refine (use_wanda_init 1 / 0) and vlmc_dsnot_refine_kind (WANDA / MAGNITUDE): the same events and stop cycles."""
    from vlmc import _lib, ops
    lib = _lib.load()
    n, m = nm
    W, scaler, sq, sum_row, var_row, div = _case(192, 4096, dtype, seed=3)
    Wd, sqd, sd, vd = W.to(DEV), sq.to(DEV), sum_row.to(DEV), var_row.to(DEV)
    for use_wanda, kind in ((1, _lib.DSNOT_INIT_WANDA), (0, _lib.DSNOT_INIT_MAGNITUDE)):
        scale = sqd if use_wanda else torch.ones_like(sqd)
        keep, _ = ops.wanda_select(Wd, scale, "nm" if n else "row", k=0 if n else 2048, n=n, m=m, apply_zero=False)
        keep2 = torch.empty_like(keep)
        _lib.check(lib.vlmc_dsnot_initial_select(Wd.data_ptr(), ops._dtype_code(Wd), 192, 4096, 4096, scale.data_ptr(),
                                                 _lib.DSNOT_INIT_WANDA, _lib.SEL_NM if n else _lib.SEL_ROW, 0 if n else 2048, n, m,
                                                 keep2.data_ptr(), ops._stream()))
        assert torch.equal(keep, keep2)
        outs = []
        for new in (False, True):
            ev = torch.empty((192, 100), dtype=torch.int32, device=DEV)
            stop = torch.empty(192, dtype=torch.int32, device=DEV)
            args = (Wd.data_ptr(), ops._dtype_code(Wd), 192, 4096, 4096, keep.data_ptr(), sqd.data_ptr(), sd.data_ptr(), vd.data_ptr())
            tail = (n, m, 100, 0.1, 1.0, 1, ev.data_ptr(), stop.data_ptr(), ops._stream())
            if new:
                _lib.check(lib.vlmc_dsnot_refine_kind(*args, kind, None, *tail))
            else:
                _lib.check(lib.vlmc_dsnot_refine(*args, use_wanda, *tail))
            outs.append((ev.cpu(), stop.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# The divisor is an fp32 factorization, as the reference's: its own fp32 chain (torch CPU) is up to 2.7e-5 off the fp64 chain on the
# golden toy Hessians (T5 decoder `o`), so agreement with fp64 is bounded by the conditioning, not by a fixed 1e-5.
DIV_RTOL = 5e-4


def _fp64_divisor(H):
    H = H.double().clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    H.diagonal().add_(0.01 * torch.mean(torch.diag(H)))
    U = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True)
    return torch.where(dead, torch.full_like(torch.diag(U), float("inf")), torch.diag(U))


def test_divisor_against_fp64_on_golden_and_rank_deficient_hessians():
    from vlmc import dsnot
    G = S.golden()
    Hs = [S.golden_hessian(G, k[:-len("/H_triu")]) for k in G if k.endswith("/H_triu")][:24]
    g = torch.Generator().manual_seed(5)
    for n in (2048, 5120, 6144):
        X = torch.randn(n // 2, n, generator=g)
        X[:, 7] = 0                                                     # a dead column as well
        Hs.append((2.0 / X.shape[0]) * (X.t() @ X))
    want = [_fp64_divisor(H) for H in Hs]
    got = dsnot.sparsegpt_divisors([H.to(DEV) for H in Hs])
    worst = 0.0
    for w, d in zip(want, got):
        d = d.cpu().double()
        assert torch.equal(torch.isinf(w), torch.isinf(d))
        fin = ~torch.isinf(w)
        worst = max(worst, float(((d[fin] - w[fin]).abs() / w[fin].abs()).max()))
    print(f"divisor: worst relative error against fp64 {worst:.3e}")
    assert worst <= DIV_RTOL


def test_not_positive_definite_raises():
    from vlmc import _lib, dsnot
    H = -torch.eye(256, device=DEV)
    with pytest.raises(_lib.VlmcError) as e:
        dsnot.sparsegpt_divisors([H, torch.eye(128, device=DEV)])
    assert e.value.code == _lib.VLMC_ENOTPD


@pytest.mark.parametrize("name", list(S.VARIANTS))
def test_pruner_on_gpu_every_linear_matches_restatement(name, monkeypatch, sgpt_oracle):
    """load_pruner("blipt5_dsnot_pruner", initial_method="sparsegpt") on toy BLIP-T5 / Vicuna: every linear bit-identical to the
    restatement fed the GPU's own statistics and divisor; the divisors within DIV_RTOL of fp64 on the GPU's own H; masks track the
    reference's run; weights zero exactly where the mask is False (untouched under lora_model); two runs identical."""
    from vlmc import dsnot
    real_prune, real_div = dsnot.prune_linear, dsnot.sparsegpt_divisors
    seen = {"linears": 0, "div_err": 0.0}

    def divisors(hessians, percdamp=0.01):
        want = [_fp64_divisor(H.cpu()) for H in hessians]
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
        assert torch.equal(weight.detach().cpu(), W0.masked_fill(~want, 0) if kw["apply_zero"] else W0)
        seen["linears"] += 1
        return keep

    monkeypatch.setattr(dsnot, "prune_linear", checked)
    monkeypatch.setattr(dsnot, "sparsegpt_divisors", divisors)
    pruned, w0 = S.run_pruner(name, DEV)
    assert seen["linears"] == len(S.linears(name))
    assert seen["div_err"] <= DIV_RTOL, seen["div_err"]
    G = S.golden()
    mods = dict(pruned.named_modules())
    worst = 1.0
    for mn in S.linears(name):
        keep = mods[mn].mask.cpu()
        worst = min(worst, float((keep == G[f"{name}/lin/{mn}/mask"]).float().mean()))
        W = mods[mn].weight.data.cpu()
        assert torch.equal(W, w0[mn].cpu() if S.VARIANTS[name]["lora"] else w0[mn].cpu().masked_fill(~keep, 0)), mn
    print(f"{name}: worst per-linear mask agreement with the reference run {worst:.5f}; divisor vs fp64 {seen['div_err']:.2e}")
    assert worst >= 0.99
    monkeypatch.setattr(dsnot, "prune_linear", real_prune)
    monkeypatch.setattr(dsnot, "sparsegpt_divisors", real_div)
    again, _ = S.run_pruner(name, DEV)
    for (ka, va), (kb, vb) in zip(pruned.state_dict().items(), again.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    for mn in S.linears(name):
        assert torch.equal(mods[mn].mask, dict(again.named_modules())[mn].mask)
