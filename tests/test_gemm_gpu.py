"""GPU parity of the MFMA GEMM engine (csrc/gemm_nt.hip) through the C ABI:

* vlmc_linear_fwd -- the dense calibration forward of a block's linears -- against an fp64 reference within the
  stated floating-point tolerance, exactly on integer data, and BATCH-INVARIANT bit for bit (the property the grouped
  calibration replay relies on: wanda_pruner.py:308-311 runs one sample per forward, here up to 128 share a launch);
* vlmc_hessian_accum -- SparseGPT.add_batch (sparsegpt_pruner.py:68-79) -- against the oracle's fp64 / the reference's
  fp32 recurrence at rel < 1e-5, at config-3 sizes (in = 5120 / 6144, 8192 / 32 896 rows)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# tolerance of the floating-point kernel (BASELINE.json north_star: "within 1e-3 rel on updated fp32 weights"; here the
# output dtype's own rounding dominates): one rounding of the 16-bit output = 2^-9 (bf16) / 2^-11 (fp16) relative,
# plus fp32 accumulation over K terms
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}


def _ref64(x, w, b):
    y = x.double().reshape(-1, x.shape[-1]) @ w.double().t()
    if b is not None:
        y = y + b.double()
    return y.reshape(*x.shape[:-1], w.shape[0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K,bias", [(1, 8, 8, False), (5, 24, 40, True), (64, 2048, 2048, False), (257, 4224, 1408, True),
                                        (128, 1408, 6144, True), (16, 5120, 2048, False), (300, 2048, 5120, False),
                                        (130, 136, 72, True), (127, 129, 64, True)])
def test_linear_fwd_matches_fp64_reference(dtype, M, N, K, bias):
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N * 3 + K)
    x = (torch.randn(M, K, generator=g, device=DEV) * 0.5 + 0.1).to(dtype)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(dtype)
    b = (torch.randn(N, generator=g, device=DEV) * 0.1).to(dtype) if bias else None
    y = ops.linear_fwd(x, w, b)
    assert y.shape == (M, N) and y.dtype == dtype
    ref = _ref64(x, w, b)
    scale = (x.double().abs() @ w.double().abs().t() + (b.double().abs() if b is not None else 0))   # sum |terms|
    err = (y.double() - ref).abs()
    bound = ULP[dtype] * ref.abs() + 4e-7 * math.sqrt(K) * scale + 1e-30
    assert bool((err <= bound).all()), float((err / bound).max())
    # and it is what rounding the fp32-accumulated product gives, up to the last bit of a few elements
    same = (y == ref.to(dtype)).float().mean().item()
    assert same > 0.98, same


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_linear_fwd_exact_on_integer_data_with_asymmetric_operands(dtype):
    """Small integers: every product and partial sum is exact in fp32, so any layout mistake (row <-> column, k order,
    a swapped fragment) shows as a wrong integer.  W and X are unrelated (asymmetric), bias included."""
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(5)
    M, N, K = 200, 264, 320
    x = torch.randint(-3, 4, (M, K), generator=g, device=DEV).to(dtype)
    w = torch.randint(-2, 3, (N, K), generator=g, device=DEV).to(dtype)
    b = torch.randint(-8, 9, (N,), generator=g, device=DEV).to(dtype)
    want = (x.float() @ w.float().t() + b.float()).to(dtype)             # exact integers, then one rounding
    assert torch.equal(ops.linear_fwd(x, w, b), want)
    assert torch.equal(ops.linear_fwd(x, w), (x.float() @ w.float().t()).to(dtype))
    eye = torch.eye(K, device=DEV).to(dtype)[:N]                         # W = I: y = x[:, :N]
    assert torch.equal(ops.linear_fwd(x, eye), x[:, :N])


@pytest.mark.parametrize("dtype,tokens,N,K", [(torch.bfloat16, 64, 2048, 2048), (torch.bfloat16, 16, 5120, 2048),
                                              (torch.float16, 257, 4224, 1408), (torch.float16, 257, 1408, 6144),
                                              (torch.bfloat16, 7, 40, 72)])
def test_linear_fwd_is_batch_invariant(dtype, tokens, N, K):
    """Rows do not depend on what else is in the launch: 24 samples forwarded one by one, in groups of 5, and all at
    once give identical bits; so does a strided (non-contiguous batch) input."""
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(tokens + N)
    S = 24
    x = (torch.randn(S, tokens, K, generator=g, device=DEV) + 0.2).to(dtype)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.03).to(dtype)
    b = (torch.randn(N, generator=g, device=DEV) * 0.1).to(dtype)
    whole = ops.linear_fwd(x, w, b)
    assert whole.shape == (S, tokens, N)
    one = torch.stack([ops.linear_fwd(x[j], w, b) for j in range(S)])
    five = torch.cat([ops.linear_fwd(x[j:j + 5], w, b) for j in range(0, S, 5)])
    assert torch.equal(whole, one) and torch.equal(whole, five)
    odd = ops.linear_fwd(x[::2], w, b)                                     # every other sample: a strided view
    assert torch.equal(odd, whole[::2])


@pytest.mark.parametrize("dtype,M,Ns,K", [
    (torch.bfloat16, 2048, (2048, 2048, 2048), 2048),        # T5 decoder q / k / v: 192 tiles of 256 x 256 in one launch
    (torch.bfloat16, 8192, (5120, 5120), 2048),              # T5 encoder wi_0 / wi_1: 1280 tiles, 5 whole rounds of the chip
    (torch.float16, 257 * 9, (1408, 4224, 136, 1408), 1408), # half panels in three of four groups, half block of rows
    (torch.bfloat16, 70, (40, 264, 8), 72),                  # register-staged kernel (K % 32 != 0), small tiles
    (torch.float16, 300, (520,), 64),                        # one group through the group entry point
])
def test_linear_fwd_group_gives_every_job_the_bits_of_its_own_launch(dtype, M, Ns, K):
    """vlmc_linear_fwd_group: up to 4 weights fed the same activations share ONE launch (q / k / v, wi_0 / wi_1).  What
    a job computes must not depend on its neighbours: bit-identical to vlmc_linear_fwd per weight, with and without bias,
    with a strided X."""
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(M + K + len(Ns))
    xw = (torch.randn(M, K + 8, generator=g, device=DEV) * 0.5 + 0.1).to(dtype)
    x = xw[:, :K]                                                          # row stride K + 8
    ws = [(torch.randn(n, K, generator=g, device=DEV) * 0.05).to(dtype) for n in Ns]
    bs = [(torch.randn(n, generator=g, device=DEV) * 0.1).to(dtype) if i % 2 == 0 else None for i, n in enumerate(Ns)]
    got = ops.linear_fwd_group(x, ws, bs)
    assert len(got) == len(Ns)
    for y, w, b in zip(got, ws, bs):
        assert y.shape == (M, w.shape[0]) and torch.equal(y, ops.linear_fwd(x, w, b))
    ref = _ref64(x, ws[-1], bs[-1])
    err = (got[-1].double() - ref).abs()
    scale = x.double().abs() @ ws[-1].double().abs().t() + (bs[-1].double().abs() if bs[-1] is not None else 0)
    assert bool((err <= ULP[dtype] * ref.abs() + 4e-7 * math.sqrt(K) * scale + 1e-30).all())
    with pytest.raises(ValueError):
        ops.linear_fwd_group(x, ws[:1] * 5)


@pytest.mark.parametrize("dtype,M,N,K", [(torch.float16, 128 * 257, 6144, 1408),      # ViT-g fc1 of 128 samples: 3096 tiles
                                         (torch.float16, 128 * 257, 1408, 6144),      # fc2: 5.5 panels x 128.5 blocks
                                         (torch.bfloat16, 8192, 2048, 5120)])         # T5 wo: 256 tiles, K = 5120
def test_persistent_256x256_kernel_against_fp64_at_prune_size(dtype, M, N, K):
    """The kernel that carries a prune's GPU time -- gemm_nt_wide_kernel (all three shapes have K % 64 == 0) on 256 x 256 tiles,
    persistent workgroups, half panels / half blocks handed out last -- held DIRECTLY against float64 at the calibration replay's own sizes
    (128 samples per launch): 16 384 sampled entries plus the whole last rows / columns (the edge tiles), the stated
    tolerance of test_linear_fwd_matches_fp64_reference."""
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(N + K)
    x = (torch.randn(M, K, generator=g, device=DEV) * 0.5 + 0.1).to(dtype)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(dtype)
    b = (torch.randn(N, generator=g, device=DEV) * 0.1).to(dtype)
    y = ops.linear_fwd(x, w, b)
    assert y.shape == (M, N) and bool(torch.isfinite(y).all())

    def check(rows, cols):
        xr, wc = x[rows].double(), w[cols].double()
        ref = (xr * wc).sum(-1) + b[cols].double()
        scale = (xr.abs() * wc.abs()).sum(-1) + b[cols].double().abs()
        err = (y[rows, cols].double() - ref).abs()
        bound = ULP[dtype] * ref.abs() + 4e-7 * math.sqrt(K) * scale + 1e-30
        assert bool((err <= bound).all()), float((err / bound).max())
    check(torch.randint(0, M, (16384,), generator=g, device=DEV), torch.randint(0, N, (16384,), generator=g, device=DEV))
    # the last block of rows and the last panel of columns, every element (edge tiles, masked waves)
    rows = torch.arange(M - 40, M, device=DEV).repeat_interleave(N)
    check(rows, torch.arange(N, device=DEV).repeat(40))
    cols = torch.arange(N - 24, N, device=DEV).repeat(2048)
    check(torch.randint(0, M, (2048,), generator=g, device=DEV).repeat_interleave(24), cols)
    # a row of the big launch has the bits of its own sample's launch (batch invariance at full size)
    for j in (0, 77, 127):
        rows_j = slice(j * (M // 128), (j + 1) * (M // 128))
        assert torch.equal(ops.linear_fwd(x[rows_j], w, b), y[rows_j])


def test_linear_fwd_refuses_what_it_cannot_do():
    from vlmc import ops
    x = torch.randn(4, 16, device=DEV)
    w = torch.randn(8, 16, device=DEV)
    assert not ops.linear_fwd_supported(x, w) and ops.linear_f32_supported(x, w)   # fp32: its own kernel since round 6 (not the 16-bit family)
    assert ops.linear_fwd(x, w).dtype == torch.float32
    with pytest.raises(TypeError):
        ops.linear_fwd(x.double(), w.double())                            # fp64: nobody's
    assert not ops.linear_fwd_supported(x.half(), w.bfloat16())
    assert not ops.linear_fwd_supported(torch.randn(4, 12, device=DEV).half(), torch.randn(8, 12, device=DEV).half())  # K % 8
    with pytest.raises(RuntimeError):
        ops.linear_fwd(x.half().cpu(), w.half().cpu())                     # no CPU fallback


# ---- Hessian (K8) -------------------------------------------------------------------------------------------------------
def _hessian_ref(xs, dtype64=True):
    """The reference's recurrence (sparsegpt_pruner.py:76-79), one update per call, in float64."""
    n = 0
    H = torch.zeros(xs[0].shape[-1], xs[0].shape[-1], dtype=torch.float64, device=xs[0].device)
    for x in xs:
        x = x.reshape(-1, x.shape[-1]).double()
        H *= n / (n + 1)
        n += 1
        H += (2.0 / n) * (x.t() @ x)
    return H


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("rows,cols", [(5, 8), (64, 128), (257, 200), (1000, 384), (300, 1408)])
def test_hessian_accum_matches_fp64(dtype, rows, cols):
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(rows + cols)
    xs = [(torch.randn(rows, cols, generator=g, device=DEV) * 0.7 + 0.3).to(dtype) for _ in range(3)]
    H = torch.zeros(cols, cols, device=DEV)
    n = 0
    for x in xs:
        ops.hessian_accum(H, x, n / (n + 1), 2.0 / (n + 1))
        n += 1
    ops.symmetrize_lower(H)
    ref = _hessian_ref(xs)
    rel = float((H.double() - ref).norm() / ref.norm())
    assert rel < 1e-6, rel
    assert float((H.double() - ref).abs().max() / ref.abs().max()) < 1e-5
    assert torch.equal(H, H.t())                                           # exactly symmetric


@pytest.mark.parametrize("dtype,rows,cols", [(torch.bfloat16, 8192, 5120), (torch.float16, 32896, 6144),
                                             (torch.bfloat16, 2048, 2048)])
def test_hessian_accum_config3_sizes(dtype, rows, cols):
    """in = 5120 / 6144 with the tokens of 128 calibration samples in ONE update (what the grouped replay feeds), against
    fp64 on a random subset of entries and against the fp32 library GEMM on the whole matrix."""
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(cols)
    x = (torch.randn(rows, cols, generator=g, device=DEV) * 0.5 + 0.1).to(dtype)
    H = torch.full((cols, cols), float("nan"), device=DEV)                # alpha = 0 must not read H
    ops.hessian_accum(H, x, 0.0, 2.0 / 128)
    ops.symmetrize_lower(H)
    assert bool(torch.isfinite(H).all()) and torch.equal(H, H.t())
    idx = torch.randint(0, cols, (4096, 2), generator=g, device=DEV)
    xd = x.double()
    want = (2.0 / 128) * (xd[:, idx[:, 0]] * xd[:, idx[:, 1]]).sum(0)
    got = H[idx[:, 0], idx[:, 1]].double()
    assert float((got - want).abs().max() / want.abs().max()) < 1e-5
    lib = torch.zeros(cols, cols, device=DEV).addmm_(x.float().t(), x.float(), beta=0.0, alpha=2.0 / 128)
    assert float((H - lib).norm() / lib.norm()) < 1e-5


def test_sparsegpt_class_uses_the_syrk_kernel_and_matches_the_library_route(monkeypatch):
    import torch.nn as nn
    from vlmc import ops, sparsegpt as SG
    calls = {"n": 0}
    real = ops.hessian_accum

    def counting(H, x, a, b):
        calls["n"] += 1
        return real(H, x, a, b)
    monkeypatch.setattr(ops, "hessian_accum", counting)
    lin = nn.Linear(384, 64, bias=False).to(DEV).to(torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(0)
    xs = [(torch.randn(1, 33, 384, generator=g, device=DEV) + 0.1).bfloat16() for _ in range(6)]
    a = SG.SparseGPT(lin)
    for x in xs:
        a.add_batch(x)
    Ha = a.H.clone()
    assert calls["n"] >= 1 and a.nsamples == 6
    monkeypatch.setattr(SG, "_SYRK", False)
    b = SG.SparseGPT(lin)
    for x in xs:
        b.add_batch(x)
    assert float((Ha - b.H).norm() / b.H.norm()) < 1e-6
    ref = _hessian_ref(xs)
    assert float((Ha.double() - ref).norm() / ref.norm()) < 1e-6


def test_hessian_of_the_reference_golden_inputs_through_the_syrk_kernel():
    """tests/golden/sparsegpt.npz holds the reference's own H after `SparseGPT.add_batch` over its calls
    (sparsegpt_pruner.py:68-79).  The fp32 cases store inputs that are exactly representable in fp16, so the fp16 MFMA
    path sees the very numbers the reference saw: H within rel 1e-5 of the reference's."""
    import golden_io
    from vlmc import ops
    G = golden_io.load("sparsegpt")
    n_checked = 0
    for name in sorted({k.split("/")[0] for k in G}):
        if f"{name}/H" not in G:
            continue
        xs, Href = G[f"{name}/xs"], G[f"{name}/H"]
        x16 = xs.to(torch.float16)
        if not torch.equal(x16.float(), xs.float()):
            x16 = xs.to(torch.bfloat16)
            if not torch.equal(x16.float(), xs.float()):
                continue
        H = torch.zeros(Href.shape, device=DEV)
        n = 0
        for x in x16:
            ops.hessian_accum(H, x[None].to(DEV), n / (n + 1), 2.0 / (n + 1))
            n += 1
        ops.symmetrize_lower(H)
        rel = float((H.cpu() - Href).norm() / Href.norm())
        assert rel < 1e-5, (name, rel)
        n_checked += 1
    assert n_checked >= 2


def test_ring_and_register_staged_kernels_give_the_same_bits(tmp_path):
    """Three kernels compute the product (operands streamed into an LDS ring by global_load_lds, K % 32 == 0, with the two waves
    of a SIMD in lockstep or half a step apart; or staged through registers, any K % 8 == 0) in five tile shapes (256 x 256,
    128 x 128, and for few rows of X 64 x 64, 32 x 64 and 32 x 32): an output element sees the same MFMAs in the same order in all
    of them.  `VLMC_GEMM_RING` / `VLMC_GEMM_BIG_TILES` /
    `VLMC_GEMM_PINGPONG` are read once per process, hence the child processes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"""
import sys, torch
sys.path.insert(0, {os.path.join(root, 'vlm-compression_amd')!r})
from vlmc import ops
g = torch.Generator(device='cuda:0').manual_seed(11)
outs = []
for dt, M, N, K in [(torch.bfloat16, 700, 1024, 2048), (torch.float16, 3000, 1408, 1408), (torch.bfloat16, 64, 5120, 2048),
                    (torch.float16, 9000, 4224, 352), (torch.float16, 20 * 257, 6144, 96), (torch.bfloat16, 301, 2048, 5120),
                    (torch.float16, 40, 1000, 1408), (torch.bfloat16, 16, 2048, 2048), (torch.bfloat16, 100, 520, 200)]:
    x = (torch.randn(M, K, generator=g, device='cuda:0') * 0.5 + 0.1).to(dt)
    w = (torch.randn(N, K, generator=g, device='cuda:0') * 0.05).to(dt)
    b = (torch.randn(N, generator=g, device='cuda:0') * 0.1).to(dt)
    outs.append(ops.linear_fwd(x, w, b).cpu())
    H = torch.zeros(K, K, device='cuda:0')
    ops.hessian_accum(H, x, 0.0, 0.01)
    outs.append(ops.symmetrize_lower(H).cpu())
torch.save(outs, sys.argv[1])
"""
    results = []
    # (ring, tiles needed for the 256 x 256 shape, the two waves of a SIMD half a step apart, persistent workgroups,
    #  half panels / blocks handed out last; edge "w": K-steps of 32 with half-line requests also where K % 64 == 0 -- the default
    #  there is the whole-line kernel)
    combos = [("1", "200", "1", "1", "1"), ("0", "200", "1", "1", "1"), ("1", "1", "1", "1", "1"), ("1", "1", "1", "0", "1"),
              ("1", "1", "0", "1", "1"), ("0", "0", "1", "1", "1"), ("1", "0", "1", "1", "1"), ("1", "1", "1", "1", "0"),
              ("1", "1", "1", "1", "w"), ("1", "0", "1", "1", "w")]
    envs = [dict(VLMC_GEMM_RING=ring, VLMC_GEMM_BIG_TILES=big, VLMC_GEMM_PINGPONG=pp, VLMC_GEMM_PERSIST=persist,
                 VLMC_GEMM_EDGE="1" if edge == "w" else edge, VLMC_GEMM_WIDE="0" if edge == "w" else "1")
            for ring, big, pp, persist, edge in combos]
    # the tile shapes for few rows of X (round 4): the default picks among them by the number of workgroups; here 128 x 128
    # everywhere, and every shape forced on every launch below the 256 x 256 threshold, ring and register-staged
    envs.append(dict(VLMC_GEMM_SMALL_TILES="0"))
    # (ring kernel of whole lines with three double steps in flight -- the default for the small shapes --, with one, the
    #  four-slot ring of half lines, the register-staged kernel)
    envs += [dict(VLMC_GEMM_SHAPE=sh, VLMC_GEMM_RING=ring, VLMC_GEMM_WIDE=wide, VLMC_GEMM_WIDE_SLOTS=slots)
             for sh in ("128", "64", "p32", "32") for ring, wide, slots in (("1", "1", "0"), ("1", "1", "2"), ("1", "0", "0"), ("0", "1", "0"))]
    for i, extra in enumerate(envs):
        out = tmp_path / f"variant{i}.pt"
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        results.append(torch.load(out))
    for extra, other in zip(envs[1:], results[1:]):
        for a, b in zip(results[0], other):
            assert torch.equal(a, b), extra


def test_256x256_kernels_agree_on_the_shortest_k_loops(tmp_path):
    """The prologue, tail and tile hand-off of the 256 x 256 kernels at the K extents where they are all there is: K = 32 (a
    one-step ring), 64 (one double step), 96 (NSLOT - 1 steps, no steady state), 128 and 192 (two and three double steps), 160
    (steady state and tail on the half-line kernel).  M = 600, N = 1100 is 2 full + 1 half block of rows and 4 full + 1 half
    panel -- 15 tiles, more than the 8 below which half panels are scheduled like full ones, so edge tiles are dealt; the
    Hessians of x [40, 1100] and [100, 1100] are SYRKs on 15 triangle tiles with one and two double steps.  Every variant --
    whole-line persistent (the default), half-line persistent, lockstep, one workgroup per tile, edges scheduled like full
    tiles -- has the bits of the register-staged kernel, and the default is within the fp64 bound of
    test_linear_fwd_matches_fp64_reference.  The switches are read once per process, hence the child processes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"""
import sys, torch
sys.path.insert(0, {os.path.join(root, 'vlm-compression_amd')!r})
from vlmc import ops
g = torch.Generator(device='cuda:0').manual_seed(23)
out = []
for dt in (torch.bfloat16, torch.float16):
    for K in (32, 64, 96, 128, 160, 192):
        x = (torch.randn(600, K, generator=g, device='cuda:0') * 0.5 + 0.1).to(dt)
        w = (torch.randn(1100, K, generator=g, device='cuda:0') * 0.05).to(dt)
        b = (torch.randn(1100, generator=g, device='cuda:0') * 0.1).to(dt)
        out.append(dict(kind='linear', x=x.cpu(), w=w.cpu(), b=b.cpu(), y=ops.linear_fwd(x, w, b).cpu()))
    for T in (40, 100):
        x = (torch.randn(T, 1100, generator=g, device='cuda:0') * 0.5 + 0.1).to(dt)
        H = torch.zeros(1100, 1100, device='cuda:0')
        ops.hessian_accum(H, x, 0.0, 0.01)
        out.append(dict(kind='hessian', x=x.cpu(), y=ops.symmetrize_lower(H).cpu()))
torch.save(out, sys.argv[1])
"""
    variants = [dict(), dict(VLMC_GEMM_WIDE="0"), dict(VLMC_GEMM_PINGPONG="0"), dict(VLMC_GEMM_PERSIST="0"), dict(VLMC_GEMM_EDGE="0"),
                dict(VLMC_GEMM_RING="0")]                                 # the last: the register-staged kernel, the reference
    results = []
    for i, extra in enumerate(variants):
        out = tmp_path / f"variant{i}.pt"
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=dict(os.environ, VLMC_GEMM_BIG_TILES="1", **extra),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (extra, r.stderr[-2000:])
        results.append(torch.load(out))
    ref = results[-1]
    for extra, res in zip(variants[:-1], results[:-1]):
        for i, (a, b) in enumerate(zip(res, ref)):
            assert torch.equal(a["x"], b["x"])                            # (same inputs in every child)
            assert torch.equal(a["y"], b["y"]), (extra, i, a["kind"], tuple(a["x"].shape), a["x"].dtype)
    for case in results[0]:
        x, y = case["x"].double(), case["y"].double()
        if case["kind"] == "linear":
            w, b, dtype, K = case["w"].double(), case["b"].double(), case["x"].dtype, x.shape[1]
            want = x @ w.t() + b
            scale = x.abs() @ w.abs().t() + b.abs()
            bound = ULP[dtype] * want.abs() + 4e-7 * math.sqrt(K) * scale + 1e-30
        else:
            # products of two 16-bit values are exact in fp32; what rounds, by at most 2^-24 relative each, are the T additions,
            # beta as an fp32 number and the multiplication by it
            T = x.shape[0]
            want = 0.01 * (x.t() @ x)
            bound = (T + 2) * 2.0 ** -24 * 0.01 * (x.abs().t() @ x.abs()) + 1e-30
        err = (y - want).abs()
        assert bool((err <= bound).all()), (case["kind"], tuple(x.shape), float((err / bound).max()))


# ---- vlmc_linear_fwd_rows: the dense calibration forward of a PADDED group of ragged samples (round 6) ------------------------------
def _ragged_case(dtype, lengths, tpad, K, seed, garbage=True):
    """x [samples, tpad, K]: a sample's own rows are data, the rows behind them hold NaN / Inf garbage (nothing may read them);
    rowmap = real rows first (sample order, token order), padding rows after."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = len(lengths)
    x = (torch.randn(B, tpad, K, generator=g, device=DEV) * 0.5 + 0.1).to(dtype)
    real, pad = [], []
    for b, t in enumerate(lengths):
        real += [b * tpad + i for i in range(t)]
        pad += [b * tpad + i for i in range(t, tpad)]
        if garbage and t < tpad:
            x[b, t:] = float("nan")
            x[b, t::2] = float("inf")
    rowmap = torch.tensor(real + pad, dtype=torch.int32, device=DEV)
    return x, rowmap, len(real)


RAGGED_SHAPES = [  # (lengths, tpad, K, [N..]): the tile families -- persistent 256 x 256, 128 x 128, 64 / 32 -- and edge rows
    ([40, 48, 56, 64, 64, 80, 96, 160] * 16, 160, 2048, [2048, 2048, 2048]),       # a T5 encoder block's q / k / v at 128 ragged samples
    ([40, 48, 56, 64, 64, 80, 96, 160] * 16, 160, 2048, [5120, 5120]),             # wi_0 / wi_1
    ([4, 8, 16, 16] * 32, 16, 2048, [2048]),                                          # the decoder's self-attention projections
    ([3, 1, 7], 9, 72, [40]),
    ([1], 5, 64, [24, 8]),
    ([17, 257, 100, 31], 257, 1408, [4224]),
    ([5, 5, 5], 5, 128, [136]),                                                       # nothing is padding
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", range(len(RAGGED_SHAPES)))
def test_linear_fwd_rows_has_the_bits_of_each_samples_own_forward(dtype, case):
    """Row-mapped launch == `linear_fwd` of every sample ALONE on its own rows (what the reference's one-sample-per-forward loop
    computes, wanda_pruner.py:308-311), bit for bit; padding rows of the outputs are +0; NaN / Inf in the padding rows of x reach nothing."""
    from vlmc import ops
    lengths, tpad, K, Ns = RAGGED_SHAPES[case]
    x, rowmap, n_real = _ragged_case(dtype, lengths, tpad, K, seed=case * 13 + 1)
    g = torch.Generator(device=DEV).manual_seed(case + 100)
    ws = [(torch.randn(N, K, generator=g, device=DEV) * 0.05).to(dtype) for N in Ns]
    bs = [(torch.randn(N, generator=g, device=DEV) * 0.1).to(dtype) if i % 2 == 0 else None for i, N in enumerate(Ns)]
    outs = ops.linear_fwd_rows(x, ws, bs, rowmap, n_real)
    assert len(outs) == len(ws)
    for y, w, b in zip(outs, ws, bs):
        assert y.shape == (len(lengths), tpad, w.shape[0]) and y.dtype == dtype
        for s_ in sorted(set(range(0, len(lengths), max(1, len(lengths) // 9))) | {len(lengths) - 1}):
            t = lengths[s_]
            alone = ops.linear_fwd(x[s_:s_ + 1, :t].contiguous(), w, b)
            assert torch.equal(y[s_, :t].view(torch.int16), alone[0].view(torch.int16)), (case, s_)
            assert bool((y[s_, t:].view(torch.int16) == 0).all()), "a padding row of Y is not +0"
        assert bool(torch.isfinite(y.float()).all())
    # against fp64 on the real rows (the same bound as vlmc_linear_fwd's)
    y, w, b = outs[0], ws[0], bs[0]
    rows = rowmap[:n_real].long()
    xr = x.reshape(-1, K)[rows]
    ref = _ref64(xr, w, b)
    scale = xr.double().abs() @ w.double().abs().t() + (b.double().abs() if b is not None else 0)
    err = (y.reshape(-1, w.shape[0])[rows].double() - ref).abs()
    assert bool((err <= ULP[dtype] * ref.abs() + 4e-7 * math.sqrt(K) * scale + 1e-30).all())


def test_linear_fwd_rows_any_row_order_and_strided_input():
    """The map is a permutation: real rows listed in another order give the same Y; x may be a row-strided view."""
    from vlmc import ops
    dtype, lengths, tpad, K, N = torch.bfloat16, [9, 3, 12, 1, 7], 12, 256, 320
    x, rowmap, n_real = _ragged_case(dtype, lengths, tpad, K, seed=3)
    w = (torch.randn(N, K, device=DEV) * 0.05).to(dtype)
    y0 = ops.linear_fwd_rows(x, [w], None, rowmap, n_real)[0]
    perm = torch.randperm(n_real, device=DEV)
    shuffled = torch.cat([rowmap[:n_real][perm], rowmap[n_real:].flip(0)]).contiguous()
    y1 = ops.linear_fwd_rows(x, [w], None, shuffled, n_real)[0]
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    wide = torch.full((len(lengths), tpad, K + 64), float("nan"), dtype=dtype, device=DEV)
    wide[..., :K] = x
    y2 = ops.linear_fwd_rows(wide[..., :K], [w], None, rowmap, n_real)[0]
    assert torch.equal(y0.view(torch.int16), y2.view(torch.int16))


def test_linear_fwd_rows_refuses_bad_maps():
    from vlmc import _lib, ops
    x = torch.zeros(2, 4, 64, dtype=torch.float16, device=DEV)
    w = torch.zeros(8, 64, dtype=torch.float16, device=DEV)
    rm = torch.arange(8, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.linear_fwd_rows(x, [w], None, rm[:7].contiguous(), 4)
    with pytest.raises(ValueError):
        ops.linear_fwd_rows(x, [w], None, rm, 0)
    with pytest.raises(ValueError):
        ops.linear_fwd_rows(x, [w], None, rm.long(), 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.linear_fwd_rows(x.cpu(), [w.cpu()], None, rm.cpu(), 4)
    lib = _lib.load()
    job = (_lib.LinearJob * 1)(_lib.LinearJob(w.data_ptr(), None, x.data_ptr(), 8, 64, 8))
    assert lib.vlmc_linear_fwd_rows(x.data_ptr(), job, 1, _lib.F16, 8, 64, 64, None, 4, None) == _lib.VLMC_EINVAL
    assert lib.vlmc_linear_fwd_rows(x.data_ptr(), job, 1, _lib.F16, 8, 64, 64, rm.data_ptr(), 9, None) == _lib.VLMC_EINVAL


# ---- fp32 on fp32 matrix cores (round 6): the reference's Q-Former stays in fp32 (blip2_t5_instruct.py:76-95, :143-175) -------------
@pytest.mark.parametrize("M,N,K,bias", [(1, 8, 8, False), (5, 24, 40, True), (300, 768, 768, True), (257 * 3, 768, 1408, True),
                                        (130, 3072, 768, True), (64, 768, 3072, False), (127, 129, 65, True), (33, 2048, 768, True)])
def test_linear_fwd_fp32_matches_fp64_and_is_batch_invariant(M, N, K, bias):
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g, device=DEV) * 0.5 + 0.1
    w = torch.randn(N, K, generator=g, device=DEV) * 0.05
    b = torch.randn(N, generator=g, device=DEV) * 0.1 if bias else None
    y = ops.linear_fwd(x, w, b)
    assert y.shape == (M, N) and y.dtype == torch.float32
    ref = _ref64(x, w, b)
    scale = x.double().abs() @ w.double().abs().t() + (b.double().abs() if b is not None else 0)
    assert bool(((y.double() - ref).abs() <= 1e-6 * scale + 1e-30).all())
    # rows do not depend on what else is in the launch; a 3-D strided input is read through its strides
    for r in sorted({0, M // 2, M - 1}):
        assert torch.equal(ops.linear_fwd(x[r:r + 1], w, b)[0], y[r]), r
    if M >= 6:
        x3 = torch.cat([x, x], dim=1)[:, :K].reshape(2, M // 2, K) if M % 2 == 0 else None
        if x3 is not None:
            assert torch.equal(ops.linear_fwd(x3, w, b).reshape(M, N), y)


@pytest.mark.parametrize("lengths,tpad,K,N", [([5, 1, 9, 3], 9, 64, 48), ([40, 104, 7, 160, 33, 99, 128, 61], 160, 768, 768),
                                               ([100] * 3 + [17] * 40 + [160], 161, 768, 3072), ([3, 2], 4, 3072, 768)])
def test_linear_fwd_rows_fp32_has_the_bits_of_each_samples_own_forward(lengths, tpad, K, N):
    """The fp32 row-mapped launch (the Q-Former's padded stack, blip2_t5_instruct.py:143-175) == `linear_fwd` of every sample alone
    on its own rows, bit for bit; padding rows of Y are +0 whatever the padding rows of x hold."""
    from vlmc import ops
    x, rowmap, n_real = _ragged_case(torch.float32, lengths, tpad, K, seed=len(lengths) + K)
    g = torch.Generator(device=DEV).manual_seed(N)
    w = torch.randn(N, K, generator=g, device=DEV) * 0.05
    b = torch.randn(N, generator=g, device=DEV) * 0.1
    for bias in (b, None):
        y = ops.linear_fwd_rows(x, [w], [bias], rowmap, n_real)[0]
        assert y.shape == (len(lengths), tpad, N) and y.dtype == torch.float32
        for s_ in sorted(set(range(0, len(lengths), max(1, len(lengths) // 7))) | {len(lengths) - 1}):
            t = lengths[s_]
            alone = ops.linear_fwd(x[s_:s_ + 1, :t].contiguous(), w, bias)
            assert torch.equal(y[s_, :t].view(torch.int32), alone[0].view(torch.int32)), s_
            assert bool((y[s_, t:].view(torch.int32) == 0).all()), "a padding row of Y is not +0"
    two = ops.linear_fwd_rows(x, [w, w[: N // 2]], [b, None], rowmap, n_real)
    assert torch.equal(two[0], ops.linear_fwd_rows(x, [w], [b], rowmap, n_real)[0]) and two[1].shape[-1] == N // 2


@pytest.mark.parametrize("lengths,P,a,L,K,N", [([40, 104, 39, 160, 33, 99, 128, 61], 160, 32, 128, 768, 3072), ([40, 104, 39, 160, 33], 160, 0, 32, 768, 768),
                                                ([5, 1, 9, 3], 9, 2, 7, 64, 48), ([2, 2, 2], 8, 4, 3, 40, 24)])
def test_linear_fwd_gather_reads_a_token_slice_in_place(lengths, P, a, L, K, N):
    """`attention_output[:, a:a + L]` of a padded stack (a BERT layer's text / query halves, Qformer.py:434-466) through
    vlmc_linear_fwd_gather: every sample's real rows of the slice have the bits of `linear_fwd` on them alone, the compact output's other
    rows are +0, NaN in the stack's padding rows reaches nothing; an empty slice (no real row at all) is all zeros."""
    import numpy as np
    from vlmc import ops
    n = len(lengths)
    g = torch.Generator(device=DEV).manual_seed(P + a + L)
    base = torch.randn(n, P, K, generator=g, device=DEV) * 0.5 + 0.1
    for j, t in enumerate(lengths):
        base[j, t:] = float("nan")
    w = torch.randn(N, K, generator=g, device=DEV) * 0.05
    b = torch.randn(N, generator=g, device=DEV) * 0.1
    x = base[:, a:a + L]
    ln = np.clip(np.asarray(lengths) - a, 0, L)
    tok = np.arange(L)[None, :]
    real = tok < ln[:, None]
    xi, yi = np.arange(n)[:, None] * P + tok, np.arange(n)[:, None] * L + tok
    x_rows = torch.from_numpy(xi[real].astype(np.int32)).to(DEV)
    y_rows = torch.from_numpy(np.concatenate([yi[real], yi[~real]]).astype(np.int32)).to(DEV)
    y = ops.linear_fwd_gather(x, w, b, x_rows, y_rows, int(real.sum()), n * L, K).view(n, L, N)
    for j in range(n):
        t = int(ln[j])
        if t:
            alone = ops.linear_fwd(base[j:j + 1, a:a + t].contiguous(), w, b)
            assert torch.equal(y[j, :t].view(torch.int32), alone[0].view(torch.int32)), j
        assert bool((y[j, t:].view(torch.int32) == 0).all())
    assert bool(torch.isfinite(y).all())


def test_linear_fwd_gather_refuses_what_it_does_not_compute():
    from vlmc import _lib, ops
    x = torch.zeros(2, 4, 64, device=DEV)
    w = torch.zeros(8, 64, device=DEV)
    xr = torch.arange(4, dtype=torch.int32, device=DEV)
    yr = torch.arange(8, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError):
        ops.linear_fwd_gather(x.half(), w.half(), None, xr, yr, 4, 8, 64)            # fp32 only
    with pytest.raises(ValueError):
        ops.linear_fwd_gather(x, w, None, xr, yr[:7].contiguous(), 4, 8, 64)         # y_rows must name every output row
    with pytest.raises(ValueError):
        ops.linear_fwd_gather(x, w, None, xr.long(), yr, 4, 8, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.linear_fwd_gather(x.cpu(), w.cpu(), None, xr.cpu(), yr.cpu(), 4, 8, 64)
    lib = _lib.load()
    y = torch.empty(8, 8, device=DEV)
    args = (x.data_ptr(), w.data_ptr(), None)
    assert lib.vlmc_linear_fwd_gather(*args, _lib.F16, 8, 64, 64, 64, y.data_ptr(), 8, xr.data_ptr(), yr.data_ptr(), 4, 4, None) == _lib.VLMC_EINVAL
    assert b"VLMC_F32" in lib.vlmc_last_error()
    assert lib.vlmc_linear_fwd_gather(*args, _lib.F32, 8, 64, 32, 64, y.data_ptr(), 8, xr.data_ptr(), yr.data_ptr(), 4, 4, None) == _lib.VLMC_EINVAL   # ldx < K
    assert lib.vlmc_linear_fwd_gather(*args, _lib.F32, 8, 64, 64, 64, y.data_ptr(), 8, None, yr.data_ptr(), 4, 4, None) == _lib.VLMC_EINVAL          # rows without x_rows
    assert lib.vlmc_linear_fwd_gather(*args, _lib.F32, 8, 64, 64, 64, y.data_ptr(), 8, None, yr.data_ptr(), 0, 8, None) == _lib.VLMC_OK              # nothing real: y cleared
    torch.cuda.synchronize()
    assert bool((y == 0).all())


def test_fp32_linears_of_a_padded_stack_take_their_real_rows_only():
    """vlmc/forward.py inside `padded_rows`: the contiguous stack by its leading shape, a token slice by what it is a view of, the
    slice's output and its GELU by the map they carry -- each equal to the full computation on the real rows, zero on the others."""
    import torch.nn.functional as F
    from vlmc import forward
    lengths, P, q = [40, 104, 39, 160, 33, 99, 128, 61], 160, 32
    n, d, h = len(lengths), 768, 3072
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(n, P, d, generator=g, device=DEV) * 0.5
    for j, t in enumerate(lengths):
        x[j, t:] = 0
    lin = [torch.nn.Linear(d, d).to(DEV), torch.nn.Linear(d, h).to(DEV), torch.nn.Linear(h, d).to(DEV)]
    import numpy as np
    ln = np.asarray(lengths)
    tok = np.arange(P)[None, :]
    real = tok < ln[:, None]
    flat = np.arange(n)[:, None] * P + tok
    rowmap = torch.from_numpy(np.concatenate([flat[real], flat[~real]]).astype(np.int32)).to(DEV)

    def block(x):
        a = lin[0](x)                                     # the whole stack
        text = lin[2](F.gelu(lin[1](a[:, q:, :])))        # intermediate / output of the text half
        query = lin[2](F.gelu(lin[1](a[:, :q, :])))       # .. of the query half (no padding)
        return a, text, query
    before = dict(forward.stats)
    with torch.no_grad(), forward.invariant_linears(lin):
        full = block(x)
        with forward.padded_rows({(n, P): (rowmap, int(real.sum()))}, None, {(n, P): tuple(lengths)}):
            part = block(x)
    assert forward.stats["kernel_slices"] - before["kernel_slices"] == 2
    assert forward.stats["kernel_rows"] - before["kernel_rows"] == 4        # the stack, two slices, the text half's tagged output (the query half's: all rows)
    for j, t in enumerate(lengths):
        assert torch.equal(part[0][j, :t], full[0][j, :t]) and bool((part[0][j, t:] == 0).all())
        tt = max(0, min(t - q, P - q))
        assert torch.equal(part[1][j, :tt], full[1][j, :tt]) and bool((part[1][j, tt:] == 0).all())
    assert torch.equal(part[2], full[2])


@pytest.mark.parametrize("B,H,Tq,Tk,d", [(3, 12, 45, 45, 64), (2, 12, 32, 257, 64), (1, 4, 7, 5, 16), (5, 12, 160, 160, 64)])
def test_attn_matmul_fp32_both_products_match_fp64_and_are_batch_invariant(B, H, Tq, Tk, d):
    """`torch.matmul(q, k.transpose(-1, -2))` and `torch.matmul(probs, v)` of the fp32 Q-Former (Qformer.py:201,246) through permuted views."""
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(B + Tq + Tk)
    q = torch.randn(B, Tq, H, d, generator=g, device=DEV).permute(0, 2, 1, 3)            # `transpose_for_scores`: a permuted view
    k = torch.randn(B, Tk, H, d, generator=g, device=DEV).permute(0, 2, 1, 3)
    v = torch.randn(B, Tk, H, d, generator=g, device=DEV).permute(0, 2, 1, 3)
    s = ops.attn_matmul(q, k.transpose(-1, -2))
    assert s.shape == (B, H, Tq, Tk) and s.dtype == torch.float32
    ref = q.double() @ k.double().transpose(-1, -2)
    assert bool(((s.double() - ref).abs() <= 1e-6 * (q.double().abs() @ k.double().abs().transpose(-1, -2)) + 1e-30).all())
    p = torch.softmax(s / 8.0, dim=-1)
    o = ops.attn_matmul(p, v)
    assert bool(((o.double() - p.double() @ v.double()).abs() <= 1e-6 * (p.double().abs() @ v.double().abs()) + 1e-30).all())
    for bi in (0, B - 1):                                                                 # one sample alone: the same bits
        assert torch.equal(ops.attn_matmul(q[bi:bi + 1], k[bi:bi + 1].transpose(-1, -2))[0], s[bi])
        assert torch.equal(ops.attn_matmul(p[bi:bi + 1], v[bi:bi + 1])[0], o[bi])


def test_gelu_fp32_is_torchs_body_arithmetic_everywhere():
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(4097 * 3 + 5, generator=g, device=DEV) * 3
    y = ops.gelu(x)
    ref = torch.nn.functional.gelu(x[:4096 * 3].double()).float()
    assert torch.allclose(y[:4096 * 3], ref, rtol=2e-6, atol=1e-7)
    assert torch.equal(ops.gelu(x[100:]), y[100:])                                          # position in the tensor does not matter
    assert torch.allclose(ops.gelu(x, "tanh"), torch.nn.functional.gelu(x, approximate="tanh"), rtol=1e-5, atol=1e-6)


# ---- the fp32 GEMM's tile sizes (csrc/gemm_f32.hip: launch_f32 picks 128 / 64 / 32 by the launch's size; VLMC_F32_TILE forces one) --
# Every tile must give an output element the same bits: a calibration sample runs alone on the 32 tile while a stack of samples
# runs on the 64 or 128 tile, and the stacked capture and the row-mapped linears rely on both being the sample's own forward.
F32_EDGES = [1, 31, 33, 64, 65, 127, 129, 257]                              # M and N across every tile's edge
F32_KS = [1, 3, 4, 5, 31, 32, 33, 63, 65, 127, 128, 129, 768, 1408, 3072]   # K across every chunk's (128 / 64 / 32) edge
F32_RAGGED = [([40, 104, 7, 160, 33, 99, 128, 61], 160, 768, 768),         # 648 padding rows: several zero blocks for every tile
              ([40, 104, 7, 160, 33, 99, 128, 61] * 6, 160, 768, 3072),    # the size rule's 128 tile
              ([5, 1, 9, 3, 70, 2] * 30, 70, 65, 129)]                     # odd K and N, 6336 padding rows
F32_GATHER = [([40, 104, 39, 160, 33, 99, 128, 61] * 4, 160, 32, 128, 768, 3072), ([5, 1, 9, 3] * 40, 9, 2, 7, 33, 65)]
F32_ATTN = [(3, 12, 45, 45, 64), (2, 4, 129, 65, 33), (1, 3, 257, 33, 127), (2, 12, 257, 257, 64), (16, 12, 160, 160, 64)]
F32_PRUNE = [(4096, 3072, 768), (20480, 768, 768)]                          # the rule's 128 and 64 tiles on a 256-CU device


def _f32_cases():
    """(M, N, K, bias, layout of X): every M and N edge meets every K; the layouts take both load branches of `fetch`."""
    cases = []
    for i, K in enumerate(F32_KS):
        for j, M in enumerate(F32_EDGES):
            cases.append((M, F32_EDGES[(i + j + 3) % len(F32_EDGES)], K, (i + j) % 2 == 0, ("dense", "stride", "offset")[(i + 2 * j) % 3]))
    return cases


def _f32_linear_inputs(M, N, K, bias, layout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 0.5 + 0.1
    w = torch.randn(N, K, generator=g) * 0.05
    b = torch.randn(N, generator=g) * 0.1 if bias else None
    if layout == "stride":                                  # rows of X (and W) at a pitch that is no multiple of 4 floats
        pad = 1 if (K + 1) % 4 else 2
        x = torch.cat([x, torch.full((M, pad), float("nan"))], 1).to(DEV)[:, :K]
        w = torch.cat([w, torch.full((N, pad), float("nan"))], 1).to(DEV)[:, :K]
    elif layout == "offset":                                # X starts 4 bytes into its buffer: no 16-byte loads
        x = torch.cat([torch.full((1,), float("nan")), x.reshape(-1)]).to(DEV)[1:].view(M, K)
    x, w = x.to(DEV), w.to(DEV)
    return x, w, b.to(DEV) if b is not None else None


def _f32_ragged_inputs(lengths, tpad, K, N):
    x, rowmap, n_real = _ragged_case(torch.float32, lengths, tpad, K, seed=len(lengths) * 7 + K)
    g = torch.Generator(device=DEV).manual_seed(N + K)
    return x, rowmap, n_real, torch.randn(N, K, generator=g, device=DEV) * 0.05, torch.randn(N, generator=g, device=DEV) * 0.1


def _f32_gather_inputs(lengths, P, a, L, K, N):
    import numpy as np
    n = len(lengths)
    g = torch.Generator(device=DEV).manual_seed(P + a + L + K)
    base = torch.randn(n, P, K, generator=g, device=DEV) * 0.5 + 0.1
    for j, t in enumerate(lengths):
        base[j, t:] = float("nan")
    w = torch.randn(N, K, generator=g, device=DEV) * 0.05
    b = torch.randn(N, generator=g, device=DEV) * 0.1
    ln = np.clip(np.asarray(lengths) - a, 0, L)
    tok = np.arange(L)[None, :]
    real = tok < ln[:, None]
    xi, yi = np.arange(n)[:, None] * P + tok, np.arange(n)[:, None] * L + tok
    x_rows = torch.from_numpy(xi[real].astype(np.int32)).to(DEV)
    y_rows = torch.from_numpy(np.concatenate([yi[real], yi[~real]]).astype(np.int32)).to(DEV)
    return base, w, b, x_rows, y_rows, int(real.sum()), ln


def _f32_attn_inputs(B, H, Tq, Tk, d):
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + Tq + Tk + d)
    q = torch.randn(B, Tq, H, d, generator=g, device=DEV).permute(0, 2, 1, 3)
    k = torch.randn(B, Tk, H, d, generator=g, device=DEV).permute(0, 2, 1, 3)
    v = torch.randn(B, Tk, H, d, generator=g, device=DEV).permute(0, 2, 1, 3)
    p = torch.softmax(torch.randn(B, H, Tq, Tk, generator=g, device=DEV), -1)          # (like softmax(q k^T / 8) of the Q-Former)
    return q, k, v, p


def _f32_prune_inputs(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    return (torch.randn(M, K, generator=g, device=DEV) * 0.5 + 0.1, torch.randn(N, K, generator=g, device=DEV) * 0.05,
            torch.randn(N, generator=g, device=DEV) * 0.1)


def f32_tile_outputs():
    """Every fp32 entry point at the tile-edge shapes (run once per VLMC_F32_TILE value, in a child process: tests/variant_runs.py)."""
    from vlmc import ops
    out = {"linear": [], "rows": [], "gather": [], "qk": [], "pv": [], "prune": []}
    for i, case in enumerate(_f32_cases()):
        x, w, b = _f32_linear_inputs(*case, seed=i)
        out["linear"].append(ops.linear_fwd(x, w, b).cpu())
    for lengths, tpad, K, N in F32_RAGGED:
        x, rowmap, n_real, w, b = _f32_ragged_inputs(lengths, tpad, K, N)
        y = ops.linear_fwd_rows(x, [w, w], [b, None], rowmap, n_real)
        out["rows"].append([t.cpu() for t in y])
    for lengths, P, a, L, K, N in F32_GATHER:
        base, w, b, x_rows, y_rows, n_real, _ = _f32_gather_inputs(lengths, P, a, L, K, N)
        out["gather"].append(ops.linear_fwd_gather(base[:, a:a + L], w, b, x_rows, y_rows, n_real, len(lengths) * L, K).cpu())
    for shape in F32_ATTN:
        q, k, v, p = _f32_attn_inputs(*shape)
        out["qk"].append(ops.attn_matmul(q, k.transpose(-1, -2)).cpu())        # B k-contiguous
        out["pv"].append(ops.attn_matmul(p, v).cpu())                          # B n-contiguous
    for shape in F32_PRUNE:
        out["prune"].append(ops.linear_fwd(*_f32_prune_inputs(*shape)).cpu())
    return out


@pytest.fixture(scope="module")
def f32_tiles(tmp_path_factory):
    import variant_runs
    return variant_runs.run_variants(tmp_path_factory.mktemp("f32_tiles"), "test_gemm_gpu", "f32_tile_outputs",
                                     {"default": {}, "128": {"VLMC_F32_TILE": "128"}, "64": {"VLMC_F32_TILE": "64"},
                                      "32": {"VLMC_F32_TILE": "32"}})


def test_f32_tiles_give_the_same_bits(f32_tiles):
    """VLMC_F32_TILE = 128 / 64 / 32 and the size rule: linear_fwd, linear_fwd_rows, linear_fwd_gather and both attn_matmul layouts
    at every tile and K-chunk edge, strided and misaligned X, with and without bias, and the prune-size shapes."""
    import variant_runs
    variant_runs.assert_variants_agree(f32_tiles)


def _f32_close(y, ref, scale):
    """the bound of test_linear_fwd_fp32_matches_fp64_and_is_batch_invariant"""
    return bool(((y.double() - ref).abs() <= 1e-6 * scale + 1e-30).all())


@pytest.mark.parametrize("tile", ["default", "128", "64", "32"])
def test_f32_tiles_against_fp64(f32_tiles, tile):
    out = f32_tiles[tile]
    for i, case in enumerate(_f32_cases()):
        x, w, b = _f32_linear_inputs(*case, seed=i)
        ref = _ref64(x, w, b).cpu()
        scale = (x.double().abs() @ w.double().abs().t() + (b.double().abs() if b is not None else 0)).cpu()
        assert _f32_close(out["linear"][i], ref, scale), case
    for (lengths, tpad, K, N), ys in zip(F32_RAGGED, out["rows"]):
        x, rowmap, n_real, w, b = _f32_ragged_inputs(lengths, tpad, K, N)
        rows = rowmap[:n_real].long()
        xr = x.reshape(-1, K)[rows]
        for y, bias in zip(ys, (b, None)):
            assert y.shape == (len(lengths), tpad, N)
            flat = y.reshape(-1, N)
            scale = xr.double().abs() @ w.double().abs().t() + (bias.double().abs() if bias is not None else 0)
            assert _f32_close(flat[rows.cpu()], _ref64(xr, w, bias).cpu(), scale.cpu()), (lengths[:4], tpad, K, N)
            pad = rowmap[n_real:].long().cpu()
            assert bool((flat[pad].view(torch.int32) == 0).all()), "a padding row of Y is not +0"
    for (lengths, P, a, L, K, N), y in zip(F32_GATHER, out["gather"]):
        base, w, b, x_rows, y_rows, n_real, ln = _f32_gather_inputs(lengths, P, a, L, K, N)
        xr = base.reshape(-1, K)[x_rows.long() + a]                  # (x_rows count from the slice's first token)
        scale = xr.double().abs() @ w.double().abs().t() + b.double().abs()
        assert _f32_close(y[y_rows[:n_real].long().cpu()], _ref64(xr, w, b).cpu(), scale.cpu())
        assert bool((y[y_rows[n_real:].long().cpu()].view(torch.int32) == 0).all()), "an output row outside the slice is not +0"
    for shape, s, o in zip(F32_ATTN, out["qk"], out["pv"]):
        q, k, v, p = (t.double() for t in _f32_attn_inputs(*shape))
        kt = k.transpose(-1, -2)
        assert s.shape == shape[:2] + (shape[2], shape[3]) and _f32_close(s, (q @ kt).cpu(), (q.abs() @ kt.abs()).cpu()), shape
        assert _f32_close(o, (p @ v).cpu(), (p.abs() @ v.abs()).cpu()), shape
    # prune size: 16 384 sampled entries and the whole last rows / columns (the edge tiles), as the 16-bit kernel's test does
    for (M, N, K), y in zip(F32_PRUNE, out["prune"]):
        x, w, b = _f32_prune_inputs(M, N, K)
        y = y.to(DEV)
        g = torch.Generator(device=DEV).manual_seed(M)

        def check(rows, cols):
            xr, wc = x[rows].double(), w[cols].double()
            ref = (xr * wc).sum(-1) + b[cols].double()
            scale = (xr.abs() * wc.abs()).sum(-1) + b[cols].double().abs()
            assert _f32_close(y[rows, cols], ref, scale), (M, N, K)
        check(torch.randint(0, M, (16384,), generator=g, device=DEV), torch.randint(0, N, (16384,), generator=g, device=DEV))
        check(torch.arange(M - 40, M, device=DEV).repeat_interleave(N), torch.arange(N, device=DEV).repeat(40))
        check(torch.randint(0, M, (2048,), generator=g, device=DEV).repeat_interleave(24), torch.arange(N - 24, N, device=DEV).repeat(2048))
