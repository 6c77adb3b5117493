"""GPU: the kernel paths that are picked by operand LAYOUT -- pointer alignment, row pitch, width divisibility -- through the C ABI.

Almost every kernel chooses between 16-byte accesses and an element-by-element fallback by where the caller's buffers lie; both are
meant to give the same bits (the library is built with -ffp-contract=off).  The wrappers of vlmc/ops.py allocate every output contiguous
and torch's allocator aligns to 512 bytes, so the other tests run the wide paths almost everywhere (profiles/layout_paths.md lists every
predicate and what reaches its false side).  Here every family takes ONE set of operand values and calls the entry point on the canonical
layout (contiguous, 256-byte aligned) and on pitched / misaligned placements of the same values (tests/layout_views.py):

  (a) the return code is 0;
  (b) the outputs equal the canonical call's BIT FOR BIT;
  (c) the sentinel around every output is untouched, and every input's backing tensor is unchanged bit for bit;
  (d) the canonical result is anchored once to the sibling test file's reference (fp64 or oracle/*) under that file's own bound.

Every view lies wholly inside one torch allocation; no test looks outside a buffer it owns."""
import ctypes
import math

import numpy as np
import pytest
import torch

import layout_views as LV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT_IDS = {F16: "fp16", BF16: "bf16", F32: "fp32"}


def _abi():
    from vlmc import _lib, ops
    return _lib, _lib.load(), ops


def _ok(rc):
    """(a): the call was accepted"""
    if rc != 0:
        _lib, lib, _ = _abi()
        raise AssertionError(f"vlmc error {rc}: {lib.vlmc_last_error().decode()}")


def _code(dtype):
    return {F32: 0, F16: 1, BF16: 2}[dtype]


def _out(shape, dtype, ld=None, off=0):
    """an output operand: every element starts as the sentinel, so an element the kernel does not write shows in (b)"""
    idt, sent = LV._BITS[dtype]
    t = torch.full(shape, sent, dtype=idt, device=DEV)
    return LV.placed(t if dtype == idt else t.view(dtype), ld, off)


class Inputs:
    """(c) for inputs: snapshots of their backing tensors, compared after the calls"""

    def __init__(self):
        self.items = []

    def place(self, t, ld=None, off=0):
        view, backing = LV.placed(t, ld, off)
        self.items.append((backing, backing.clone()))
        return view

    def unchanged(self):
        return all(torch.equal(b, s) for b, s in self.items)


def _same(a, b):
    return torch.equal(LV.bits(a), LV.bits(b))


# =====================================================================================================================================
# Linear GEMM, 16-bit: vlmc_linear_fwd / _group / _rows (csrc/gemm_nt.hip: the epilogue's `vec_ok` and `bias4`, zero_pad_rows' `vec_ok`)
# =====================================================================================================================================
ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -10}                     # tests/test_gemm_gpu.py
LIN_M, LIN_K = 37, 72
# (ldy - N, Y's offset in elements): canonical first; pitched and still wide; pitched narrow; wide pitch, 8 bytes past alignment
LIN_Y_LAYOUTS = [(0, 0), (8, 0), (3, 0), (8, 4)]


def _lin_values(dtype, Ns, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(LIN_M, LIN_K, generator=g, device=DEV) * 0.5 + 0.1).to(dtype)
    ws = [(torch.randn(n, LIN_K, generator=g, device=DEV) * 0.05).to(dtype) for n in Ns]
    bs = [(torch.randn(n, generator=g, device=DEV) * 0.1).to(dtype) for n in Ns]
    return x, ws, bs


def _lin_fp64_ok(y, x, w, b, dtype):
    """the bound of tests/test_gemm_gpu.py::test_linear_fwd_matches_fp64_reference"""
    ref = x.double() @ w.double().t() + (b.double() if b is not None else 0)
    scale = x.double().abs() @ w.double().abs().t() + (b.double().abs() if b is not None else 0)
    err = (y.double() - ref).abs()
    bound = ULP[dtype] * ref.abs() + 4e-7 * math.sqrt(x.shape[1]) * scale + 1e-30
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("N", [24, 20, 136])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_linear_fwd_pitched_and_misaligned_outputs_and_bias(dtype, N):
    _lib, lib, ops = _abi()
    x, (w,), (b,) = _lin_values(dtype, [N], N)
    inp = Inputs()
    xv, wv = inp.place(x), inp.place(w)
    canon = None
    for bias_off in (0, 1, None):                           # 8-byte aligned; one element past it (`bias4` false); no bias
        bv = None if bias_off is None else inp.place(b, None, bias_off)
        first = None
        for dld, yoff in LIN_Y_LAYOUTS:
            yv, yb = _out((LIN_M, N), dtype, N + dld, yoff)
            _ok(lib.vlmc_linear_fwd(xv.data_ptr(), wv.data_ptr(), None if bv is None else bv.data_ptr(), _code(dtype), LIN_M, N, LIN_K,
                                    LIN_K, LIN_K, yv.data_ptr(), N + dld, ops._stream()))
            assert LV.untouched(yb, yv), (bias_off, dld, yoff)
            if first is None:
                first = yv.clone()
                _lin_fp64_ok(first, x, w, None if bias_off is None else b, dtype)
            assert _same(yv, first), (bias_off, dld, yoff)
        if bias_off == 0:
            canon = first
        elif bias_off == 1:
            assert _same(first, canon), "a bias one element past 8-byte alignment changed the result"
    assert inp.unchanged()


@pytest.mark.parametrize("ldy", [88, 87])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_linear_fwd_group_writes_column_slices_of_one_buffer(dtype, ldy):
    """q / k / v into column slices of ONE [37, 84 (+ gap)] buffer: the per-job `ldy` of vlmc_linear_job.  With ldy = 88 the slices at
    columns 0 and 24 are 16-byte aligned and the one at column 44 is not; with ldy = 87 every row of every slice is narrow."""
    _lib, lib, ops = _abi()
    Ns = [24, 20, 40]
    x, ws, bs = _lin_values(dtype, Ns, 7)
    bs[1] = None
    inp = Inputs()
    xv = inp.place(x)
    wvs = [inp.place(w) for w in ws]
    bvs = [None if b is None else inp.place(b, None, i) for i, b in enumerate(bs)]       # the third bias two elements (4 bytes) past alignment
    want = []
    for w, b, wv, bv, n in zip(ws, bs, wvs, bvs, Ns):                                     # every job alone, canonical layout
        yv, yb = _out((LIN_M, n), dtype)
        _ok(lib.vlmc_linear_fwd(xv.data_ptr(), wv.data_ptr(), None if bv is None else bv.data_ptr(), _code(dtype), LIN_M, n, LIN_K, LIN_K,
                                LIN_K, yv.data_ptr(), n, ops._stream()))
        assert LV.untouched(yb, yv)
        _lin_fp64_ok(yv, x, w, b, dtype)
        want.append(yv.clone())
    whole, backing = _out((LIN_M, sum(Ns)), dtype, ldy)
    jobs = (_lib.LinearJob * 3)()
    col = 0
    for i, n in enumerate(Ns):
        jobs[i] = _lib.LinearJob(wvs[i].data_ptr(), None if bvs[i] is None else bvs[i].data_ptr(), whole[:, col:].data_ptr(), n, LIN_K, ldy)
        col += n
    _ok(lib.vlmc_linear_fwd_group(xv.data_ptr(), jobs, 3, _code(dtype), LIN_M, LIN_K, LIN_K, ops._stream()))
    assert LV.untouched(backing, whole)
    assert _same(whole, torch.cat(want, dim=1))
    assert inp.unchanged()


@pytest.mark.parametrize("N", [24, 20, 136])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_linear_fwd_rows_pitched_outputs_and_zeroed_padding_rows(dtype, N):
    """n_real = 29 of 37 rows through a permutation: the real rows have the bits of vlmc_linear_fwd, the padding rows are zero on every
    layout (zero_pad_rows' scalar branch) and the gap beside them is untouched."""
    _lib, lib, ops = _abi()
    n_real = 29
    x, (w,), (b,) = _lin_values(dtype, [N], N + 1)
    g = torch.Generator().manual_seed(N)
    rowmap = torch.randperm(LIN_M, generator=g).to(torch.int32).to(DEV)
    real = rowmap[:n_real].long()
    inp = Inputs()
    xv, wv, mv = inp.place(x), inp.place(w), inp.place(rowmap)
    dense, db = _out((LIN_M, N), dtype)
    bv0 = inp.place(b)
    _ok(lib.vlmc_linear_fwd(xv.data_ptr(), wv.data_ptr(), bv0.data_ptr(), _code(dtype), LIN_M, N, LIN_K, LIN_K, LIN_K, dense.data_ptr(), N,
                            ops._stream()))
    _lin_fp64_ok(dense, x, w, b, dtype)
    want = torch.zeros_like(dense)
    want[real] = dense[real]
    for bias_off in (0, 1):
        bv = inp.place(b, None, bias_off)
        for dld, yoff in LIN_Y_LAYOUTS:
            yv, yb = _out((LIN_M, N), dtype, N + dld, yoff)
            job = (_lib.LinearJob * 1)(_lib.LinearJob(wv.data_ptr(), bv.data_ptr(), yv.data_ptr(), N, LIN_K, N + dld))
            _ok(lib.vlmc_linear_fwd_rows(xv.data_ptr(), job, 1, _code(dtype), LIN_M, LIN_K, LIN_K, mv.data_ptr(), n_real, ops._stream()))
            assert LV.untouched(yb, yv), (bias_off, dld, yoff)
            assert _same(yv, want), (bias_off, dld, yoff)
    assert inp.unchanged()


# =====================================================================================================================================
# Hessian: vlmc_hessian_accum / _rows / vlmc_symmetrize_lower (csrc/gemm_nt.hip: the SYRK epilogue's `vec_ok`, the transposing pre-pass
# chosen by `(ldx & 7) == 0 && aligned16(X)`)
# =====================================================================================================================================
HES_ROWS = 37


def _hessian_ref(xs):
    """tests/test_gemm_gpu.py::_hessian_ref: the reference's recurrence (sparsegpt_pruner.py:76-79) in float64"""
    n = 0
    H = torch.zeros(xs[0].shape[-1], xs[0].shape[-1], dtype=torch.float64, device=xs[0].device)
    for x in xs:
        x = x.double()
        H *= n / (n + 1)
        n += 1
        H += (2.0 / n) * (x.t() @ x)
    return H


def _hessian_layouts(n, dtype):
    """(ldh - n, H offset, ldx - n, X offset) in elements"""
    lay = [(0, 0, 0, 0), (4, 0, 0, 0), (1, 0, 0, 0), (4, 1, 0, 0), (0, 0, 8, 0), (4, 1, 1, 1)]
    if dtype == F32:
        lay.append((0, 0, 0, 1))                              # fp32 X one float past alignment
    return lay


@pytest.mark.parametrize("rows_variant", [False, True], ids=["accum", "accum_rows"])
@pytest.mark.parametrize("n", [8, 70, 129, 200])
@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=["fp16", "bf16", "fp32"])
def test_hessian_accum_into_pitched_and_misaligned_H(dtype, n, rows_variant):
    """Two updates -- alpha = 0 into an H that holds NaN, then alpha = 0.5 -- and the symmetrization.  `_rows`: X has 45 rows, the map
    keeps 37 of them (the dropped rows hold NaN) and the result has the bits of vlmc_hessian_accum on the compacted rows."""
    _lib, lib, ops = _abi()
    g = torch.Generator(device=DEV).manual_seed(n + HES_ROWS)
    xs = [(torch.randn(HES_ROWS, n, generator=g, device=DEV) * 0.7 + 0.3).to(dtype) for _ in range(2)]
    total = 45
    keep_rows = torch.randperm(total, generator=torch.Generator().manual_seed(n))[:HES_ROWS].sort().values
    rmap = keep_rows.to(torch.int32).to(DEV)
    code = _code(dtype)
    need = lib.vlmc_hessian_workspace(code, HES_ROWS, n)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    inp = Inputs()
    mv = inp.place(rmap)
    canon = None
    for dldh, hoff, dldx, xoff in _hessian_layouts(n, dtype):
        use_map = rows_variant and canon is not None           # the canonical call is always vlmc_hessian_accum on the compacted rows
        hv, hb = _out((n, n), F32, n + dldh, hoff)
        for x, (alpha, beta) in zip(xs, [(0.0, 2.0), (0.5, 1.0)]):
            if use_map:
                wide = torch.full((total, n), float("nan"), dtype=dtype, device=DEV)
                wide[keep_rows.to(DEV)] = x
                xv = inp.place(wide, n + dldx, xoff)
                _ok(lib.vlmc_hessian_accum_rows(xv.data_ptr(), code, total, n, n + dldx, mv.data_ptr(), HES_ROWS, hv.data_ptr(), n + dldh,
                                                alpha, beta, ws.data_ptr(), need, ops._stream()))
            else:
                xv = inp.place(x, n + dldx, xoff)
                _ok(lib.vlmc_hessian_accum(xv.data_ptr(), code, HES_ROWS, n, n + dldx, hv.data_ptr(), n + dldh, alpha, beta, ws.data_ptr(),
                                           need, ops._stream()))
        _ok(lib.vlmc_symmetrize_lower(hv.data_ptr(), n, n + dldh, ops._stream()))
        assert LV.untouched(hb, hv), (dldh, hoff, dldx, xoff)
        if canon is None:
            canon = hv.clone()
            ref = _hessian_ref(xs)                             # the bounds of tests/test_gemm_gpu.py::test_hessian_accum_matches_fp64
            assert float((canon.double() - ref).norm() / ref.norm()) < 1e-6
            assert float((canon.double() - ref).abs().max() / ref.abs().max()) < 1e-5
            assert torch.equal(canon, canon.t())
        assert _same(hv, canon), (dldh, hoff, dldx, xoff)
    assert inp.unchanged()


# =====================================================================================================================================
# SparseLoRA weight algebra: vlmc_lora_effective_weight (4 modes), vlmc_lora_grad (csrc/sparse_lora.hip: `vec` at :75 and :271)
# =====================================================================================================================================
def _close_lowp(got, ref, name, min_exact):
    """tests/test_sparse_lora_gpu.py::_close_lowp"""
    got, ref = got.float().cpu(), ref.float()
    exact = (got == ref).float().mean().item()
    assert exact >= min_exact, f"{name}: only {exact:.4f} of the entries bit-identical"
    ulp = ref.abs().clamp_min(1e-30) * 2.0 ** -7
    assert bool(((got - ref).abs() <= ulp + 1e-12).all()), f"{name}: differs by more than one bf16 ulp"


def _lora_values(shape, r, wd):
    out_f, in_f = shape
    g = torch.Generator().manual_seed(out_f + in_f + r)
    W = (torch.randn(out_f, in_f, generator=g) * 0.05).to(wd)
    A = torch.randn(r, in_f, generator=g) * 0.1
    B = torch.randn(out_f, r, generator=g) * 0.1
    M = torch.rand(out_f, in_f, generator=g) > 0.5
    Gw = (torch.randn(out_f, in_f, generator=g) * 0.1).to(wd)
    return W, A, B, M, Gw, 16 / r


LORA_SHAPES = [(33, 72), (40, 100), (257, 260)]


@pytest.mark.parametrize("r", [3, 8])
@pytest.mark.parametrize("shape", LORA_SHAPES, ids=[f"{o}x{i}" for o, i in LORA_SHAPES])
@pytest.mark.parametrize("wd", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
def test_lora_effective_weight_on_pitched_misaligned_and_aliased_operands(wd, shape, r):
    from oracle import sparse_lora as OL
    _lib, lib, ops = _abi()
    out_f, in_f = shape
    W, A, B, M, _, s = _lora_values(shape, r, wd)
    inp = Inputs()
    Av, Bv = inp.place(A.to(DEV)), inp.place(B.to(DEV))
    Wd, Md = W.to(DEV), M.to(DEV)
    # (ldw - in, W offset, ldo - in, W_out offset, mask offset in bytes, W_out aliases W)
    layouts = [(0, 0, 0, 0, 0, False), (8, 0, 8, 0, 0, False), (1, 0, 1, 0, 0, False), (8, 1, 8, 0, 0, False), (8, 0, 8, 1, 0, False),
               (0, 0, 0, 0, 1, False), (0, 0, 8, 0, 0, False), (8, 0, 8, 0, 0, True), (1, 1, 1, 1, 1, True)]
    for mode in range(4):                                       # FWD_SPARSE, FWD_MASKED, MERGE_SPARSE, MERGE_MASKED
        canon = None
        for dldw, woff, dldo, ooff, moff, alias in layouts:
            mv = inp.place(Md, None, moff)
            if alias:
                wv, wb = LV.placed(Wd, in_f + dldw, woff)        # input and output: only its surroundings are checked
                ov, ob, ldo = wv, wb, in_f + dldw
            else:
                wv = inp.place(Wd, in_f + dldw, woff)
                ov, ob = _out(shape, wd, in_f + dldo, ooff)
                ldo = in_f + dldo
            _ok(lib.vlmc_lora_effective_weight(wv.data_ptr(), _code(wd), out_f, in_f, in_f + dldw, Av.data_ptr(), Bv.data_ptr(), r, s,
                                               mv.data_ptr(), mode, 0, ov.data_ptr(), ldo, ops._stream()))
            assert LV.untouched(ob, ov), (mode, dldw, woff, dldo, ooff, moff, alias)
            if canon is None:
                canon = ov.clone()
                sparse = mode in (0, 2)
                want = OL.effective_weight(W, A, B, M, s, sparse).detach() if mode < 2 else OL.merge(W, A, B, M, s, sparse)
                if wd == F32:                                   # the bounds of test_kernels_vs_oracle_random_shapes
                    torch.testing.assert_close(canon.cpu(), want, rtol=1e-5, atol=1e-6)
                else:
                    _close_lowp(canon, want, f"mode {mode}", 0.99)
            assert _same(ov, canon), (mode, dldw, woff, dldo, ooff, moff, alias)
    assert inp.unchanged()


@pytest.mark.parametrize("r", [3, 8])
@pytest.mark.parametrize("shape", LORA_SHAPES, ids=[f"{o}x{i}" for o, i in LORA_SHAPES])
@pytest.mark.parametrize("wd", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
def test_lora_grad_on_pitched_and_misaligned_gradients(wd, shape, r):
    from oracle import sparse_lora as OL
    _lib, lib, ops = _abi()
    out_f, in_f = shape
    W, A, B, M, Gw, s = _lora_values(shape, r, wd)
    inp = Inputs()
    Av, Bv = inp.place(A.to(DEV)), inp.place(B.to(DEV))
    Gd, Md = Gw.to(DEV), M.to(DEV)
    need = lib.vlmc_lora_grad_workspace(out_f, in_f, r)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    layouts = [(0, 0, 0), (8, 0, 0), (1, 0, 0), (8, 1, 0), (0, 0, 1), (1, 1, 1)]        # (ldg - in, G offset, mask offset in bytes)
    for sparse in (1, 0):
        canon = None
        for dldg, goff, moff in layouts:
            gv, mv = inp.place(Gd, in_f + dldg, goff), inp.place(Md, None, moff)
            (dA, dAb), (dB, dBb) = _out((r, in_f), F32), _out((out_f, r), F32)
            _ok(lib.vlmc_lora_grad(gv.data_ptr(), _code(wd), out_f, in_f, in_f + dldg, Av.data_ptr(), Bv.data_ptr(), r, s, mv.data_ptr(),
                                   sparse, 0, dA.data_ptr(), dB.data_ptr(), ws.data_ptr(), need, ops._stream()))
            assert LV.untouched(dAb, dA) and LV.untouched(dBb, dB), (sparse, dldg, goff, moff)
            if canon is None:
                canon = (dA.clone(), dB.clone())
                Ar, Br = A.clone().requires_grad_(True), B.clone().requires_grad_(True)
                OL.effective_weight(W, Ar, Br, M, s, bool(sparse)).backward(Gw)
                gt = dict(rtol=1e-4, atol=1e-5) if wd == F32 else dict(rtol=2e-2, atol=2e-3 * (in_f / 500) ** 0.5)
                torch.testing.assert_close(canon[0].cpu(), Ar.grad, **gt)
                torch.testing.assert_close(canon[1].cpu(), Br.grad, **gt)
            assert _same(dA, canon[0]) and _same(dB, canon[1]), (sparse, dldg, goff, moff)
    assert inp.unchanged()


# =====================================================================================================================================
# Row kernels: vlmc_rms_norm, vlmc_softmax_rows, vlmc_gelu, vlmc_reorder_indices (csrc/row_reduce.hip, elementwise.hip)
# =====================================================================================================================================
ROWS = 9


# (vlmc_row_mean has no case here: tests/test_row_mean_gpu.py compares a pitched view one float past alignment with its contiguous copy
# and fails under a value change in the scalar loads -- profiles/layout_paths.md)


@pytest.mark.parametrize("n", [72, 1000])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_rms_norm_pitched_and_misaligned(dtype, n):
    """rsqrt_mode: the one vlmc/forward.py picks on this build; reference: the op sequence of tests/test_rms_norm_gpu.py, bit for bit."""
    from vlmc import forward
    _lib, lib, ops = _abi()
    mode = forward._rsqrt_modes(torch.device(DEV))[0]
    eps = 1e-6
    g = torch.Generator(device=DEV).manual_seed(n)
    x = (torch.randn(ROWS, n, generator=g, device=DEV) * 2).to(dtype)
    x[0] = 0
    w = (torch.randn(n, generator=g, device=DEV) * 0.3 + 1).to(dtype)
    inp = Inputs()
    canon = None
    # (ldx - n, x offset, ldy - n, y offset, weight offset)
    for dldx, xoff, dldy, yoff, woff in [(0, 0, 0, 0, 0), (4, 0, 4, 0, 0), (1, 0, 1, 0, 0), (4, 1, 4, 0, 0), (4, 0, 4, 1, 0), (0, 0, 0, 0, 1),
                                         (4, 0, 1, 0, 0), (1, 1, 4, 1, 1)]:
        xv, wv = inp.place(x, n + dldx, xoff), inp.place(w, None, woff)
        yv, yb = _out((ROWS, n), dtype, n + dldy, yoff)
        _ok(lib.vlmc_rms_norm(xv.data_ptr(), _code(dtype), ROWS, n, n + dldx, wv.data_ptr(), eps, mode, yv.data_ptr(), n + dldy, ops._stream()))
        assert LV.untouched(yb, yv), (dldx, xoff, dldy, yoff, woff)
        if canon is None:
            canon = yv.clone()
            if mode == 0:                                       # (the sibling's reference is torch.rsqrt: the flavour it equals)
                with torch.no_grad(), forward.invariant_matmuls():
                    v = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
                    want = w * (x * torch.rsqrt(v + eps)).to(w.dtype)
                assert _same(canon, want)
            ref = w.double() * (x.double() * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + eps))
            assert float((canon.double() - ref).abs().max() / ref.abs().max()) < 2.0 ** -7      # two roundings to the dtype
        assert _same(yv, canon), (dldx, xoff, dldy, yoff, woff)
    assert inp.unchanged()


@pytest.mark.parametrize("n", [5, 17, 257])
@pytest.mark.parametrize("pair", [(F32, F32), (F16, F16), (F16, F32), (BF16, BF16), (BF16, F32)], ids=lambda p: f"{DT_IDS[p[0]]}-{DT_IDS[p[1]]}")
def test_softmax_rows_pitched_and_in_place(pair, n):
    _lib, lib, ops = _abi()
    din, dout = pair
    rows = 37
    g = torch.Generator(device=DEV).manual_seed(n)
    x = (torch.randn(rows, n, generator=g, device=DEV) * 4).to(din)
    inp = Inputs()
    canon = None
    for dldx, xoff, dldy, yoff in [(0, 0, 0, 0), (8, 0, 8, 0), (1, 0, 1, 0), (3, 1, 1, 1), (0, 0, 3, 0)]:
        xv = inp.place(x, n + dldx, xoff)
        yv, yb = _out((rows, n), dout, n + dldy, yoff)
        _ok(lib.vlmc_softmax_rows(xv.data_ptr(), _code(din), rows, n, n + dldx, yv.data_ptr(), _code(dout), n + dldy, ops._stream()))
        assert LV.untouched(yb, yv), (dldx, xoff, dldy, yoff)
        if canon is None:
            canon = yv.clone()
            tol = {F32: 2e-6, F16: 1e-3, BF16: 8e-3}[dout]       # tests/test_attn_fused_gpu.py::test_softmax_rows_dtypes_and_padding_invariance
            assert float((canon.double() - torch.softmax(x.double(), -1)).abs().max()) <= tol
        assert _same(yv, canon), (dldx, xoff, dldy, yoff)
    if din == dout:                                             # in place in a pitched buffer
        for dld, off in [(1, 0), (3, 1)]:
            xv, xb = LV.placed(x, n + dld, off)
            _ok(lib.vlmc_softmax_rows(xv.data_ptr(), _code(din), rows, n, n + dld, xv.data_ptr(), _code(dout), n + dld, ops._stream()))
            assert LV.untouched(xb, xv) and _same(xv, canon), (dld, off)
    assert inp.unchanged()


@pytest.mark.parametrize("n", [1, 7, 1001])
@pytest.mark.parametrize("tanh", [0, 1], ids=["erf", "tanh"])
def test_gelu_fp32_misaligned_and_in_place(tanh, n, dtype=F32):
    """fp32 only: the 16-bit kernel's scalar branch is reached by tests/test_gelu_gpu.py (a view two bytes past alignment), which fails
    under a value change there; its fp32 sibling in tests/test_gemm_gpu.py passes only 16-byte aligned views."""
    import torch.nn.functional as F
    _lib, lib, ops = _abi()
    g = torch.Generator(device=DEV).manual_seed(n)
    x = (torch.randn(n, generator=g, device=DEV) * 3).to(dtype)
    inp = Inputs()
    canon = None
    for xoff, yoff in [(0, 0), (1, 0), (0, 1), (1, 1)]:
        xv = inp.place(x, None, xoff)
        yv, yb = _out((n,), dtype, None, yoff)
        _ok(lib.vlmc_gelu(xv.data_ptr(), yv.data_ptr(), n, _code(dtype), tanh, ops._stream()))
        assert LV.untouched(yb, yv), (xoff, yoff)
        if canon is None:
            canon = yv.clone()
            if tanh:                                            # tests/test_gemm_gpu.py::test_gelu_fp32_is_torchs_body_arithmetic_everywhere
                assert torch.allclose(canon, F.gelu(x, approximate="tanh"), rtol=1e-5, atol=1e-6)
            else:
                assert torch.allclose(canon, F.gelu(x.double()).float(), rtol=2e-6, atol=1e-7)
        assert _same(yv, canon), (xoff, yoff)
    for off in (0, 1):                                          # y == x
        xv, xb = LV.placed(x, None, off)
        _ok(lib.vlmc_gelu(xv.data_ptr(), xv.data_ptr(), n, _code(dtype), tanh, ops._stream()))
        assert LV.untouched(xb, xv) and _same(xv, canon), off
    assert inp.unchanged()


@pytest.mark.parametrize("cols", [1, 255, 257])
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
def test_reorder_indices_pitched_input_and_output(dtype, cols):
    from oracle import dsnot as OD
    _lib, lib, ops = _abi()
    rows = 7
    g = torch.Generator().manual_seed(rows * 131 + cols)
    x = torch.randn(rows, cols, generator=g)
    x[torch.rand(rows, cols, generator=g) < 0.2] = 0.0
    x[torch.rand(rows, cols, generator=g) < 0.02] = float("nan")
    x[torch.rand(rows, cols, generator=g) < 0.02] = -0.0
    x = x.to(dtype)
    want = OD.reorder_indices(x.float())
    inp = Inputs()
    for dldx, xoff, dldo, ooff in [(0, 0, 0, 0), (8, 0, 2, 0), (1, 0, 1, 0), (1, 1, 3, 1)]:
        xv = inp.place(x.to(DEV), cols + dldx, xoff)
        ov, ob = _out((rows, cols), torch.int64, cols + dldo, ooff)
        _ok(lib.vlmc_reorder_indices(xv.data_ptr(), _code(dtype), rows, cols, cols + dldx, ov.data_ptr(), cols + dldo, ops._stream()))
        assert LV.untouched(ob, ov), (dldx, xoff, dldo, ooff)
        assert torch.equal(ov.cpu(), want), (dldx, xoff, dldo, ooff)     # integers: the oracle's answer is the canonical call's
    assert inp.unchanged()


# =====================================================================================================================================
# 2:4 packing: vlmc_pack_24 / vlmc_unpack_24 (csrc/pack24.hip: no width switch, but `ldw` / `ldm` were never larger than the width)
# =====================================================================================================================================
@pytest.mark.parametrize("shape", [(5, 8), (33, 64)], ids=["5x8", "33x64"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_pack_24_round_trip_through_pitched_operands(dtype, shape):
    from oracle import pack24
    _lib, lib, ops = _abi()
    out_f, in_f = shape
    g = torch.Generator().manual_seed(out_f + in_f)
    W = torch.randn(out_f, in_f, generator=g).to(dtype)
    W[0, :4] = 0                                                 # kept zeros stay kept
    order = torch.rand(out_f, in_f // 4, 4, generator=g).argsort(-1)
    keep = (order < 2).reshape(out_f, in_f)
    ov, om, obad = pack24.pack(W.view(torch.int16).numpy().view(np.uint16), keep.numpy())
    assert obad == 0
    inp = Inputs()
    Wd, Kd = W.to(DEV), keep.to(DEV)
    packed = None
    for dldw, woff, dldm, moff in [(0, 0, 0, 0), (8, 0, 8, 0), (1, 0, 1, 0), (8, 1, 8, 1), (1, 1, 8, 3)]:
        wv, kv = inp.place(Wd, in_f + dldw, woff), inp.place(Kd, in_f + dldm, moff)
        (vals, vb), (meta, mb) = _out((out_f, in_f // 2), dtype), _out((out_f, in_f // 8), torch.uint8)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        _ok(lib.vlmc_pack_24(wv.data_ptr(), _code(dtype), out_f, in_f, in_f + dldw, kv.data_ptr(), in_f + dldm, vals.data_ptr(), meta.data_ptr(),
                             bad.data_ptr(), ops._stream()))
        assert int(bad.item()) == 0 and LV.untouched(vb, vals) and LV.untouched(mb, meta), (dldw, woff, dldm, moff)
        if packed is None:
            packed = (vals.clone(), meta.clone())
            assert np.array_equal(vals.cpu().view(torch.int16).numpy().view(np.uint16), ov) and np.array_equal(meta.cpu().numpy(), om)
        assert _same(vals, packed[0]) and _same(meta, packed[1]), (dldw, woff, dldm, moff)
    vals, meta = inp.place(packed[0]), inp.place(packed[1])
    want_w = torch.where(keep, W, torch.zeros_like(W))                  # a pruned weight is +0, whatever its sign was
    for dldw, woff, dldm, moff in [(0, 0, 0, 0), (8, 0, 8, 0), (1, 0, 1, 0), (8, 1, 8, 1), (1, 1, 8, 3)]:
        (w2, w2b), (k2, k2b) = _out(shape, dtype, in_f + dldw, woff), _out(shape, torch.bool, in_f + dldm, moff)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        _ok(lib.vlmc_unpack_24(vals.data_ptr(), meta.data_ptr(), _code(dtype), out_f, in_f, w2.data_ptr(), in_f + dldw, k2.data_ptr(),
                               in_f + dldm, bad.data_ptr(), ops._stream()))
        assert int(bad.item()) == 0 and LV.untouched(w2b, w2) and LV.untouched(k2b, k2), (dldw, woff, dldm, moff)
        assert _same(w2.cpu(), want_w) and torch.equal(k2.view(torch.uint8).cpu(), keep.view(torch.uint8)), (dldw, woff, dldm, moff)
    assert inp.unchanged()


# =====================================================================================================================================
# SparseGPT block: vlmc_chol_block (csrc/cholesky.hip `vec4` / `vec4o`), vlmc_sparsegpt_sweep / _prune_blocks (csrc/sparsegpt.hip :153)
# =====================================================================================================================================
@pytest.mark.parametrize("nb", [128, 70])
def test_chol_block_pitched_and_misaligned(nb):
    _lib, lib, ops = _abi()
    g = torch.Generator().manual_seed(nb)
    X = torch.randn(2 * nb, nb, generator=g)
    A = (X.t() @ X / X.shape[0] + 0.05 * torch.eye(nb)).to(DEV)
    inp = Inputs()
    canon = None
    # (lda - nb, A offset, ldl - nb, L offset, ldi - nb, Linv offset)
    for dlda, aoff, dldl, loff, dldi, ioff in [(0, 0, 0, 0, 0, 0), (4, 0, 4, 0, 4, 0), (1, 0, 1, 0, 1, 0), (4, 1, 4, 0, 4, 0), (4, 0, 4, 1, 4, 0),
                                               (4, 0, 4, 0, 4, 1), (0, 0, 1, 0, 0, 0), (0, 0, 0, 0, 1, 0)]:
        av = inp.place(A, nb + dlda, aoff)
        (L, Lb), (Li, Lib) = _out((nb, nb), F32, nb + dldl, loff), _out((nb, nb), F32, nb + dldi, ioff)
        info = torch.zeros(1, dtype=torch.int32, device=DEV)
        _ok(lib.vlmc_chol_block(av.data_ptr(), nb + dlda, nb, L.data_ptr(), nb + dldl, Li.data_ptr(), nb + dldi, info.data_ptr(), 0,
                                ops._stream()))
        assert int(info.item()) == 0 and LV.untouched(Lb, L) and LV.untouched(Lib, Li), (dlda, aoff, dldl, loff, dldi, ioff)
        if canon is None:
            canon = (L.clone(), Li.clone())
            ref = torch.linalg.cholesky(A.double())             # the bounds of test_blocked_cholesky_matches_library_factorization
            assert float((L.double() - ref).abs().max() / ref.abs().max()) < 2e-5
            assert float((L @ L.t() - A).abs().max() / A.abs().max()) < 1e-5
            assert float(torch.triu(L, 1).abs().max()) == 0.0
            eye = (Li.double() @ ref)                            # inv(L) L = I (the panel GEMM's operand)
            assert float((eye - torch.eye(nb, dtype=torch.float64, device=DEV)).abs().max()) < 1e-4
        assert _same(L, canon[0]) and _same(Li, canon[1]), (dlda, aoff, dldl, loff, dldi, ioff)
    assert inp.unchanged()


def _sweep_values(rows, count, nm, seed):
    from oracle import sparsegpt as OS
    g = torch.Generator().manual_seed(seed)
    W1 = torch.randn(rows, count, generator=g) * 0.05
    W1[torch.rand(rows, count, generator=g) < 0.1] = 0
    A = torch.randn(count, count * 2, generator=g)
    U = torch.linalg.cholesky(A @ A.t() / count + 0.1 * torch.eye(count), upper=True)
    n, _ = nm
    mask1 = OS.block_mask_unstructured(W1, torch.diag(U), 0.5) if n == 0 else torch.zeros_like(W1) == 1
    return W1, U, mask1


@pytest.mark.parametrize("nm", [(2, 4), (0, 0)], ids=["2of4", "unstructured"])
@pytest.mark.parametrize("count", [96, 128])
def test_sparsegpt_sweep_with_every_pitch_by_one(count, nm):
    from oracle import sparsegpt as OS
    _lib, lib, ops = _abi()
    rows = 37
    n, m = nm
    W1, U, mask1 = _sweep_values(rows, count, nm, count + rows)
    Q, Err, mask_ref = OS.sweep_block(W1.clone(), U, mask1.clone(), n, m)       # tests/test_sparsegpt_gpu.py: bit-exact given the factor
    inp = Inputs()
    # (ldw, ldu, ldm, lde, ldmo) - count; offsets of W, U, mask1, Err, mask_out
    for pitch, offs in [((0,) * 5, (0,) * 5), ((4,) * 5, (0,) * 5), ((1,) * 5, (0,) * 5), ((4,) * 5, (1, 0, 0, 0, 0)), ((4,) * 5, (0, 1, 0, 0, 0)),
                        ((4,) * 5, (0, 0, 1, 1, 1)), ((1,) * 5, (1, 1, 1, 1, 3))]:
        wv, wb = LV.placed(W1.to(DEV), count + pitch[0], offs[0])
        uv = inp.place(U.to(DEV), count + pitch[1], offs[1])
        m1 = inp.place(mask1.to(DEV), count + pitch[2], offs[2]) if n == 0 else None
        (ev, eb), (mo, mob) = _out((rows, count), F32, count + pitch[3], offs[3]), _out((rows, count), torch.bool, count + pitch[4], offs[4])
        _ok(lib.vlmc_sparsegpt_sweep(wv.data_ptr(), rows, count, count + pitch[0], uv.data_ptr(), count + pitch[1],
                                     None if m1 is None else m1.data_ptr(), count + pitch[2] if m1 is not None else 0, n, m, ev.data_ptr(),
                                     count + pitch[3], mo.data_ptr(), count + pitch[4], ops._stream()))
        assert LV.untouched(wb, wv) and LV.untouched(eb, ev) and LV.untouched(mob, mo), (pitch, offs)
        assert _same(wv.cpu(), Q) and _same(ev.cpu(), Err), (pitch, offs)
        assert torch.equal(mo.view(torch.uint8).cpu(), mask_ref.view(torch.uint8)), (pitch, offs)
    assert inp.unchanged()


@pytest.mark.parametrize("nm", [(2, 4), (0, 0)], ids=["2of4", "unstructured"])
def test_sparsegpt_prune_blocks_pitched_with_a_short_last_block(nm):
    """[37, 320] with blocksize 128: the last block has 64 columns.  Canonical: the block loop on contiguous operands, anchored to the oracle's
    sweep and a plain trailing product block by block, under the bounds of tests/test_sparsegpt_gpu.py::test_fasterprune_larger_layer_vs_oracle
    (masks agree up to near-ties at a block's threshold, rows without a flipped entry within 1e-3 relative)."""
    from oracle import sparsegpt as OS
    _lib, lib, ops = _abi()
    rows, cols, bs = 37, 320, 128
    n, m = nm
    g = torch.Generator().manual_seed(cols + n)
    W = torch.randn(rows, cols, generator=g) * 0.05
    A = torch.randn(cols, cols * 2, generator=g)
    U = torch.linalg.cholesky(A @ A.t() / cols + 0.1 * torch.eye(cols), upper=True)
    inp = Inputs()
    canon = None
    wsz = int(lib.vlmc_sparsegpt_select_workspace_bytes())
    for pitch, offs in [((0,) * 4, (0,) * 4), ((4,) * 4, (0,) * 4), ((1,) * 4, (0,) * 4), ((4,) * 4, (1, 1, 1, 1)), ((1,) * 4, (1, 1, 1, 3))]:
        wv, wb = LV.placed(W.to(DEV), cols + pitch[0], offs[0])
        uv = inp.place(U.to(DEV), cols + pitch[1], offs[1])
        (ev, eb), (mo, mob) = _out((rows, bs), F32, bs + pitch[2], offs[2]), _out((rows, cols), torch.bool, cols + pitch[3], offs[3])
        sel = torch.zeros(wsz // 4, dtype=torch.int32, device=DEV)
        scope_rows = (ctypes.c_int64 * 1)(rows)
        scope_sp = (ctypes.c_double * 1)(0.5)
        _ok(lib.vlmc_sparsegpt_prune_blocks(wv.data_ptr(), rows, cols, cols + pitch[0], uv.data_ptr(), cols + pitch[1], bs, n, m, 0 if n else 1,
                                            None if n else scope_rows, None if n else scope_sp, ev.data_ptr(), bs + pitch[2], mo.data_ptr(),
                                            cols + pitch[3], None if n else sel.data_ptr(), ops._stream()))
        torch.cuda.synchronize()
        assert LV.untouched(wb, wv) and LV.untouched(mob, mo), (pitch, offs)
        assert not bool(sel.any()), "the select workspace was not returned zero"
        # err is scratch: the last block writes 64 of its 128 columns, the earlier blocks all of them -- its surroundings stay untouched
        assert LV.untouched(eb, ev), (pitch, offs)
        if canon is None:
            canon = (wv.clone(), mo.clone())
            Wr = W.clone()
            mref = torch.zeros(rows, cols, dtype=torch.bool)
            for i1 in range(0, cols, bs):
                i2 = min(i1 + bs, cols)
                U1 = U[i1:i2, i1:i2]
                W1 = Wr[:, i1:i2].clone()
                mask1 = OS.block_mask_unstructured(W1, torch.diag(U1), 0.5) if n == 0 else torch.zeros_like(W1) == 1
                Qb, Eb, mb = OS.sweep_block(W1, U1, mask1, n, m)
                Wr[:, i1:i2], mref[:, i1:i2] = Qb, mb
                Wr[:, i2:] -= (Eb.double() @ U[i1:i2, i2:].double()).float()
            agree = (canon[1].cpu() == mref)
            assert agree.float().mean().item() >= 0.999
            clean = agree.all(dim=1)
            assert clean.float().mean().item() > 0.8
            got = canon[0].cpu()
            assert float((got[clean] - Wr[clean]).norm() / Wr[clean].norm()) < 1e-3
        assert _same(wv, canon[0]) and _same(mo, canon[1]), (pitch, offs)
    assert inp.unchanged()


# =====================================================================================================================================
# DSnoT: vlmc_dsnot_apply (csrc/dsnot.hip:453 `vec`), vlmc_dsnot_refine / _refine_kind with a pitched W
# =====================================================================================================================================
def _dsnot_setup(dtype, in_f, nm):
    from oracle import dsnot as OD
    from vlmc import dsnot
    out_f = 9
    g = torch.Generator().manual_seed(in_f + out_f)
    W = (torch.randn(out_f, in_f, generator=g) * 0.02).to(dtype)
    xs = [((torch.randn(1, 9, in_f, generator=g) * 0.5) + 0.2).to(dtype) for _ in range(4)]
    ost = OD.DSnoTStat(in_f)
    st = dsnot.DsnotInputStat(in_f, DEV)
    for x in xs:
        ost.add_batch(x)
        st.add_call(x.to(DEV))
    st.finalize()
    ost.scaler_row, ost.sum_metric_row, ost.var = st.scaler_row.cpu(), st.sum_row.cpu(), st.var_row.cpu().reshape(-1, 1)
    mc = min(60, in_f - 4)
    n, m = nm
    want = OD.prune_nm(W, ost, n, m, max_cycle_time=mc, update_threshold=0.05) if n else \
        OD.prune_unstructured(W, ost, 0.5, max_cycle_time=mc, update_threshold=0.05)
    return W, st, mc, ~want


@pytest.mark.parametrize("nm", [(0, 0), (2, 4)], ids=["unstructured", "2of4"])
@pytest.mark.parametrize("in_f", [24, 72, 1000])
@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=["fp16", "bf16", "fp32"])
def test_dsnot_apply_on_pitched_and_misaligned_weights(dtype, in_f, nm):
    _lib, lib, ops = _abi()
    out_f = 9
    n, m = nm
    W, st, mc, want_keep = _dsnot_setup(dtype, in_f, nm)
    Wd = W.to(DEV)
    inp = Inputs()
    Wc = inp.place(Wd)
    keep0, _ = ops.wanda_select(Wc, st.sqrt_row, "nm" if n else "row", k=round(in_f * 0.5), n=n, m=m, apply_zero=False)
    k0 = inp.place(keep0)
    sq, su, va = inp.place(st.sqrt_row), inp.place(st.sum_row), inp.place(st.var_row)

    def refine(wv, ldw, kind):
        (ev, eb), (sv, sb) = _out((out_f, mc), torch.int32), _out((out_f,), torch.int32)
        if kind:
            _ok(lib.vlmc_dsnot_refine_kind(wv.data_ptr(), _code(dtype), out_f, in_f, ldw, k0.data_ptr(), sq.data_ptr(), su.data_ptr(), va.data_ptr(),
                                           _lib.DSNOT_INIT_WANDA, None, n, m, mc, 0.05, 1.0, 1, ev.data_ptr(), sv.data_ptr(), ops._stream()))
        else:
            _ok(lib.vlmc_dsnot_refine(wv.data_ptr(), _code(dtype), out_f, in_f, ldw, k0.data_ptr(), sq.data_ptr(), su.data_ptr(), va.data_ptr(), 1,
                                      n, m, mc, 0.05, 1.0, 1, ev.data_ptr(), sv.data_ptr(), ops._stream()))
        assert LV.untouched(eb, ev) and LV.untouched(sb, sv)
        return ev, sv
    events, stop = refine(Wc, in_f, False)
    Wp = inp.place(Wd, in_f + 8)                                 # refine demands 16-byte aligned rows: pitched, still aligned
    for kind in (False, True):
        e2, s2 = refine(Wp, in_f + 8, kind)
        assert _same(e2, events) and _same(s2, stop), kind
    ncyc = inp.place(stop.max().clamp(max=mc).to(torch.int32).reshape(1))
    evs = inp.place(events)
    for apply_zero in (0, 1):
        canon = None
        for dldw, woff, koff in [(0, 0, 0), (8, 0, 0), (1, 0, 0), (8, 1, 0), (0, 0, 1), (1, 1, 1)]:
            if apply_zero:
                wv, wb = LV.placed(Wd, in_f + dldw, woff)
            else:
                wv = inp.place(Wd, in_f + dldw, woff)
            kv, kb = LV.placed(keep0, None, koff)                 # in / out, row-contiguous by contract
            _ok(lib.vlmc_dsnot_apply(wv.data_ptr(), _code(dtype), out_f, in_f, in_f + dldw, kv.data_ptr(), evs.data_ptr(), ncyc.data_ptr(), mc,
                                     int(n != 0), apply_zero, ops._stream()))
            assert LV.untouched(kb, kv), (apply_zero, dldw, woff, koff)
            if apply_zero:
                assert LV.untouched(wb, wv), (apply_zero, dldw, woff, koff)
            if canon is None:
                canon = (kv.clone(), wv.clone())
                assert torch.equal(kv.cpu(), want_keep), "the canonical mask is not the oracle's replay"
                if apply_zero:
                    assert _same(wv.cpu(), torch.where(want_keep, W, torch.zeros_like(W)))
            assert _same(kv, canon[0]) and _same(wv, canon[1]), (apply_zero, dldw, woff, koff)
    assert inp.unchanged()


# =====================================================================================================================================
# Wanda select: vlmc_wanda_select in its three modes and _batch (csrc/wanda_select.hip: `job_aligned`, the grouping by it at :1835)
# =====================================================================================================================================
WANDA_MODES = {"row": 0, "matrix": 1, "nm": 2}


def _wanda_case(out_f, in_f, dtype, seed):
    """tests/test_wanda_gpu.py::_rand_case"""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(out_f, in_f, generator=g) * 0.02).to(dtype)
    s = (torch.rand(in_f, generator=g) * 4 + 0.01).numpy().astype(np.float32)
    return W, s


def _wanda_args(mode, W):
    if mode == "row":
        return dict(k=int(W.shape[1] * 0.5), n=0, m=0)
    if mode == "matrix":
        return dict(k=int(W.numel() * 0.5), n=0, m=0)
    return dict(k=0, n=2, m=4)


class _WandaCall:
    """the operands of one vlmc_wanda_select job on one layout: W in / out, mask and partial sums out, a SEL_MATRIX workspace"""

    def __init__(self, lib, inp, mode, W, sq, dld, woff, sqoff, moff, ws=None):
        out_f, in_f = W.shape
        self.ldw = in_f + dld
        self.W, self.Wb = LV.placed(W, self.ldw, woff)
        self.sq = inp.place(sq, None, sqoff)
        self.mask, self.maskb = _out((out_f, in_f), torch.bool, None, moff)
        code = WANDA_MODES[mode]
        self.nparts = int(lib.vlmc_wanda_select_partials(code, out_f, in_f))
        self.parts = torch.zeros(max(self.nparts, 1), dtype=torch.float64, device=DEV)
        self.ws_bytes = int(lib.vlmc_wanda_select_workspace(code, out_f, in_f))
        # zero-filled when it is first handed over, then REUSED as the last call left it (include/vlmc.h): `ws` is an earlier call's
        self.ws = torch.zeros(max(self.ws_bytes, 256), dtype=torch.uint8, device=DEV) if ws is None else ws
        assert self.ws.data_ptr() % 256 == 0

    def check_surroundings(self):
        assert LV.untouched(self.Wb, self.W) and LV.untouched(self.maskb, self.mask)
        # the histogram and control words come back zero; the key slots / candidate lists behind them are scratch (include/vlmc.h)
        assert not bool(self.ws[:8320].any()), "the SEL_MATRIX workspace's counters were not returned zero"


WANDA_LAYOUTS = [(0, 0, 0, 0), (8, 0, 0, 0), (1, 0, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (8, 1, 0, 0), (1, 1, 1, 1)]     # (ldw - in, W, sqrt_scaler, mask offsets)


@pytest.mark.parametrize("shape", [(11, 104), (9, 2056)], ids=["11x104", "9x2056"])
@pytest.mark.parametrize("mode", ["row", "matrix", "nm"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_wanda_select_on_pitched_and_misaligned_operands(dtype, mode, shape):
    from oracle import wanda as OW
    _lib, lib, ops = _abi()
    W, s = _wanda_case(*shape, dtype, shape[0] * 7 + shape[1])
    kw = _wanda_args(mode, W)
    sq = ops.sqrt_scaler(torch.from_numpy(s).to(DEV))
    Wd = W.to(DEV)
    inp = Inputs()
    ws = None                                                   # ONE workspace for every call of the test, aligned and unaligned kernels in turn
    for apply_zero in (1, 0):
        canon = None
        for lay in WANDA_LAYOUTS:
            c = _WandaCall(lib, inp, mode, Wd, sq, *lay, ws=ws)
            ws = c.ws
            _ok(lib.vlmc_wanda_select(c.W.data_ptr(), _code(dtype), shape[0], shape[1], c.ldw, c.sq.data_ptr(), WANDA_MODES[mode], kw["k"], kw["n"],
                                      kw["m"], apply_zero, c.mask.data_ptr(), c.parts.data_ptr(), c.ws.data_ptr() if c.ws_bytes else None,
                                      c.ws_bytes, ops._stream()))
            c.check_surroundings()
            imp = float(c.parts[:c.nparts].sum().item()) / W.numel()
            if canon is None:
                canon = (c.W.clone(), c.mask.clone())
                want = OW.prune_linear(W, s, mode, ratio=0.5, n=kw["n"], m=kw["m"], apply_zero=bool(apply_zero))     # tests/test_wanda_gpu.py
                assert np.array_equal(c.mask.cpu().numpy(), want["mask"])
                assert torch.equal(c.W.cpu().view(torch.uint8), want["weight"].view(torch.uint8))
            # the partial sums are cut by the kernel that ran; their total is the reference's sum (rel 1e-5, tests/test_wanda_gpu.py)
            assert imp == pytest.approx(want["importance_score"], rel=1e-5), lay
            assert _same(c.W, canon[0]) and _same(c.mask, canon[1]), (apply_zero, lay)
    assert inp.unchanged()


@pytest.mark.parametrize("mode", ["row", "matrix", "nm"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_wanda_select_batch_mixing_aligned_and_misaligned_jobs(dtype, mode):
    """Six jobs of one (in_features, k), alternately aligned and not: SEL_ROW groups them by alignment (wanda_select.hip:1835), SEL_MATRIX and
    SEL_NM launch a group on the unaligned kernel as soon as one member is.  Every job has the bits of its own single call."""
    _lib, lib, ops = _abi()
    out_f, in_f = 11, 104
    inp = Inputs()
    cases = [_wanda_case(out_f, in_f, dtype, 100 + j) for j in range(6)]
    kw = _wanda_args(mode, cases[0][0])
    sqs = [ops.sqrt_scaler(torch.from_numpy(s).to(DEV)) for _, s in cases]
    singles = []
    for (W, _), sq in zip(cases, sqs):
        c = _WandaCall(lib, inp, mode, W.to(DEV), sq, 0, 0, 0, 0)
        _ok(lib.vlmc_wanda_select(c.W.data_ptr(), _code(dtype), out_f, in_f, c.ldw, c.sq.data_ptr(), WANDA_MODES[mode], kw["k"], kw["n"], kw["m"], 1,
                                  c.mask.data_ptr(), c.parts.data_ptr(), c.ws.data_ptr() if c.ws_bytes else None, c.ws_bytes, ops._stream()))
        c.check_surroundings()
        singles.append(c)
    lays = [(0, 0, 0, 0), (1, 0, 0, 0), (8, 0, 0, 0), (8, 1, 0, 0), (0, 0, 0, 0), (0, 0, 1, 1)]
    # SEL_MATRIX workspaces: distinct per job, each used by its job's single call before and handed on as that call left it
    calls = [_WandaCall(lib, inp, mode, W.to(DEV), sq, *lay, ws=one.ws) for (W, _), sq, lay, one in zip(cases, sqs, lays, singles)]
    assert len({c.ws.data_ptr() for c in calls}) == 6
    jobs = (_lib.SelectJob * 6)()
    for j, c in enumerate(calls):
        jobs[j] = _lib.SelectJob(c.W.data_ptr(), out_f, in_f, c.ldw, c.sq.data_ptr(), kw["k"], c.mask.data_ptr(), c.parts.data_ptr(),
                                 c.ws.data_ptr() if c.ws_bytes else None, c.ws_bytes)
    _ok(lib.vlmc_wanda_select_batch(jobs, 6, _code(dtype), WANDA_MODES[mode], kw["n"], kw["m"], 1, ops._stream()))
    for j, (c, one) in enumerate(zip(calls, singles)):
        c.check_surroundings()
        assert _same(c.W, one.W) and _same(c.mask, one.mask), j
        assert float(c.parts[:c.nparts].sum()) == pytest.approx(float(one.parts[:one.nparts].sum()), rel=1e-5), j
    assert inp.unchanged()


# =====================================================================================================================================
# Global select: vlmc_score_select (csrc/score_select.hip:458 `vec_ok`, false only for misaligned pointers)
# =====================================================================================================================================
SCORE_NUMEL = [1000, 1001, 4096, 77]
SCORE_SCOPES = [0, 0, 1, 1]
SCORE_DTYPES = [BF16, F16, F32, BF16]
# which operands of which jobs sit one element past alignment: (W, S, prev_keep, keep) per job
_ALL, _NONE = (1, 1, 1, 1), (0, 0, 0, 0)
SCORE_LAYOUTS = {"canonical": [_NONE] * 4, "W": [(1, 0, 0, 0)] * 4, "S": [(0, 1, 0, 0)] * 4, "prev_keep": [(0, 0, 1, 0)] * 4, "keep": [(0, 0, 0, 1)] * 4,
                 "all": [_ALL] * 4, "mixed_jobs": [_NONE, _ALL, _NONE, _ALL]}


@pytest.mark.parametrize("mode", ["weight", "score", "absw_score"])
def test_score_select_with_misaligned_operands(mode):
    import oracle_ops
    _lib, lib, ops = _abi()
    g = torch.Generator().manual_seed(len(mode))
    ws = [(torch.randn(n, generator=g) * 0.05).to(dt) for n, dt in zip(SCORE_NUMEL, SCORE_DTYPES)]
    ws[2][torch.rand(4096, generator=g) < 0.2] = 0
    S = None if mode == "weight" else [torch.randn(n, generator=g) if mode == "score" else torch.rand(n, generator=g) for n in SCORE_NUMEL]
    prev = [torch.rand(n, generator=g) > 0.3 for n in SCORE_NUMEL]
    ks = [int(0.4 * (1000 + 1001)), int(0.6 * (4096 + 77))]
    use_w = True                                                 # VLMC_SCORE_S may leave W out; given, it is multiplied by the mask like the others
    want_w = [w.clone() for w in ws]
    want = oracle_ops.score_select(want_w, mode, scopes=SCORE_SCOPES, scope_ks=ks, scores=S, prev_keeps=prev, protect_ks=None)   # tests/test_global_gpu.py
    inp = Inputs()
    canon = None
    for name, lay in SCORE_LAYOUTS.items():
        wv, wb, keeps, kb = [], [], [], []
        for w, (ow, _, _, ok_) in zip(ws, lay):
            a, b = LV.placed(w.to(DEV), None, ow)
            wv.append(a), wb.append(b)
            a, b = _out((w.numel(),), torch.bool, None, ok_)
            keeps.append(a), kb.append(b)
        Sd = None if S is None else [inp.place(s.to(DEV), None, o[1]) for s, o in zip(S, lay)]
        pd = [inp.place(p.to(DEV), None, o[2]) for p, o in zip(prev, lay)]
        got = ops.score_select(wv if use_w else None, mode, scopes=SCORE_SCOPES, scope_ks=ks, scores=Sd, prev_keeps=pd, keeps=keeps)
        for i in range(4):
            assert LV.untouched(kb[i], keeps[i]) and LV.untouched(wb[i], wv[i]), (name, i)
        if canon is None:
            canon = ([k.clone() for k in got], [w.clone() for w in wv])
            for i in range(4):
                assert torch.equal(got[i].cpu(), want[i]), i
                if use_w:
                    assert torch.equal(wv[i].cpu().view(torch.uint8), want_w[i].view(torch.uint8)), i
        for i in range(4):
            assert _same(got[i], canon[0][i]) and _same(wv[i], canon[1][i]), (name, i)
    assert inp.unchanged()


# =====================================================================================================================================
# Refusals: layouts that include/vlmc.h excludes next to the entry point (found while writing this file; nothing is launched)
# =====================================================================================================================================
def test_dsnot_refine_refuses_narrow_or_misaligned_rows():
    """vlmc_dsnot_refine / _refine_kind read the rows in 16-byte chunks only (the replay hands them whole nn.Linear weights)."""
    _lib, lib, ops = _abi()
    out_f, in_f, mc = 9, 72, 20
    W = torch.zeros(out_f, in_f, dtype=F16, device=DEV)
    keep = torch.ones(out_f, in_f, dtype=torch.bool, device=DEV)
    sq, su, va = (torch.ones(in_f, device=DEV) for _ in range(3))
    events = torch.zeros(out_f, mc, dtype=torch.int32, device=DEV)
    stop = torch.zeros(out_f, dtype=torch.int32, device=DEV)
    for dld, woff, koff in [(1, 0, 0), (8, 1, 0), (0, 0, 1)]:
        wv, _ = LV.placed(W, in_f + dld, woff)
        kv, _ = LV.placed(keep, None, koff)
        for kind in (False, True):
            if kind:
                rc = lib.vlmc_dsnot_refine_kind(wv.data_ptr(), 1, out_f, in_f, in_f + dld, kv.data_ptr(), sq.data_ptr(), su.data_ptr(), va.data_ptr(),
                                                _lib.DSNOT_INIT_WANDA, None, 0, 0, mc, 0.05, 1.0, 1, events.data_ptr(), stop.data_ptr(), ops._stream())
            else:
                rc = lib.vlmc_dsnot_refine(wv.data_ptr(), 1, out_f, in_f, in_f + dld, kv.data_ptr(), sq.data_ptr(), su.data_ptr(), va.data_ptr(), 1, 0, 0,
                                           mc, 0.05, 1.0, 1, events.data_ptr(), stop.data_ptr(), ops._stream())
            assert rc == _lib.VLMC_EINVAL, (dld, woff, koff, kind)
            assert "needs in_features % 8 == 0 and 16-byte aligned rows" in lib.vlmc_last_error().decode()
    assert not bool(events.any()) and not bool(stop.any())


def test_chol_inverse_refuses_odd_pitches_and_misaligned_matrices():
    _lib, lib, ops = _abi()
    n = 128
    need = int(lib.vlmc_chol_inverse_workspace(n))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    eye = torch.eye(n, device=DEV)
    for dld, off, msg in [(1, 0, "row strides must be >= n and multiples of 4"), (4, 1, "matrices must be 16-byte aligned")]:
        for which in range(3):
            ops_ = [LV.placed(eye, n + (dld if i == which else 0), off if i == which else 0) for i in range(3)]
            (a, _), (m, mb), (x, xb) = ops_
            rc = lib.vlmc_chol_inverse(a.data_ptr(), n, a.stride(0), m.data_ptr(), m.stride(0), x.data_ptr(), x.stride(0), info.data_ptr(), ws.data_ptr(),
                                       need, 0, ops._stream())
            assert rc == _lib.VLMC_EINVAL and msg in lib.vlmc_last_error().decode(), (dld, off, which)
            assert torch.equal(m, eye) and torch.equal(x, eye) and LV.untouched(mb, m) and LV.untouched(xb, x)
