"""GPU: `vlmc_rope` (csrc/rope.hip) against the tensor-op sequence of the reference's `apply_rotary_pos_emb`
(modeling_llama.py:126-140, restated in vlmc/synthetic_llama.py) -- bit for bit: fp16 and bf16, head_dim 64 and 128, q / k as strided
views of a stacked q / k / v tensor, `position_ids` [B, T] and [1, T], positions that are not monotonic, `q_len` (live rows equal, the
rows behind them zero).  Error paths through the status code and the error string; nothing here provokes a fault."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _inputs(dtype, d, B=3, H=32, T=45, P=200, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = (torch.randn(B, T, 3, H, d, generator=g, device=DEV) * scale).to(dtype)           # a grouped q / k / v launch's output
    q, k = qkv[:, :, 0].transpose(1, 2), qkv[:, :, 1].transpose(1, 2)                      # [B, H, T, d] views, token stride 3 H d
    from vlmc.synthetic_llama import LlamaRotaryEmbeddingOps
    rot = LlamaRotaryEmbeddingOps(d, max_position_embeddings=P).to(DEV)
    cos, sin = rot(q, seq_len=P - 7)                                                       # [1, 1, P - 7, d] in the dtype
    return g, q, k, cos, sin, P - 7


@pytest.mark.parametrize("batched_positions", [True, False], ids=["pos[B,T]", "pos[1,T]"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_rope_has_the_bits_of_the_op_sequence(dtype, d, batched_positions):
    from vlmc import ops
    from vlmc.synthetic_llama import apply_rotary_pos_emb
    g, q, k, cos, sin, P = _inputs(dtype, d, seed=d + batched_positions)
    B, H, T, _ = q.shape
    assert not q.is_contiguous() and q.stride(2) == 3 * H * d
    pos = torch.randint(0, P, (B if batched_positions else 1, T), generator=g, device=DEV)  # not monotonic, with repeats
    pos[0, 0], pos[-1, -1] = P - 1, 0                                                       # the table's last and first row
    want_q, want_k = apply_rotary_pos_emb(q, k, cos, sin, pos)
    got_q, got_k = ops.rope(q, k, cos, sin, pos)
    assert got_q.shape == want_q.shape == (B, H, T, d) and got_q.transpose(1, 2).is_contiguous()
    nq, nk = int((_bits(got_q) != _bits(want_q)).sum()), int((_bits(got_k) != _bits(want_k)).sum())
    print(f"rope {dtype} d={d} pos{tuple(pos.shape)}: {nq} + {nk} of 2 x {got_q.numel()} entries differ")
    assert nq == 0 and nk == 0
    assert not torch.equal(_bits(got_q), _bits(q))                                          # (it did rotate)
    # k as a contiguous tensor, q as it is: every operand through its own strides
    got_q2, got_k2 = ops.rope(q, k.contiguous(), cos, sin, pos)
    assert torch.equal(_bits(got_q2), _bits(want_q)) and torch.equal(_bits(got_k2), _bits(want_k))
    ops.rope_check(DEV)                                                                     # every position was inside the table


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_rope_on_large_and_tiny_values_and_a_small_head(dtype):
    """values whose products overflow / underflow the dtype round where the tensor ops round; head_dim 8 and 24 (d / 2 not a multiple
    of 8: a chunk's partners straddle two)"""
    from vlmc import ops
    from vlmc.synthetic_llama import apply_rotary_pos_emb
    for d, scale in ((64, 3e4 if dtype == torch.float16 else 1e38), (64, 1e-6), (8, 1.0), (24, 1.0)):
        g, q, k, cos, sin, P = _inputs(dtype, d, B=2, H=4, T=19, P=50, seed=d, scale=scale)
        pos = torch.randint(0, P, (2, 19), generator=g, device=DEV)
        want = apply_rotary_pos_emb(q, k, cos, sin, pos)
        got = ops.rope(q, k, cos, sin, pos)
        for w, o in zip(want, got):
            finite = torch.isfinite(w.float())                                              # (inf - inf = NaN: sign / payload not compared)
            assert torch.equal(_bits(o)[finite], _bits(w)[finite]) and torch.equal(torch.isnan(o.float()), torch.isnan(w.float())), (d, scale)


def test_rope_lengths_keep_the_live_rows_and_zero_the_rest():
    from vlmc import ops
    dtype, d = torch.float16, 128
    g, q, k, cos, sin, P = _inputs(dtype, d, B=4, H=32, T=60, seed=5)
    lens = [60, 13, 1, 44]
    pos = torch.randint(0, P, (4, 60), generator=g, device=DEV)
    for i, n in enumerate(lens):
        pos[i, n:] = 10 ** 9                                                                # rows behind a length are not read: nor are their positions
    ql = torch.tensor(lens, dtype=torch.int32, device=DEV)
    safe = pos.clamp(max=P - 1)
    full_q, full_k = ops.rope(q, k, cos, sin, safe)
    cut_q, cut_k = ops.rope(q, k, cos, sin, pos, q_len=ql)
    for i, n in enumerate(lens):
        assert torch.equal(_bits(cut_q[i, :, :n]), _bits(full_q[i, :, :n])) and torch.equal(_bits(cut_k[i, :, :n]), _bits(full_k[i, :, :n]))
        assert bool((_bits(cut_q[i, :, n:]) == 0).all()) and bool((_bits(cut_k[i, :, n:]) == 0).all()), "a padding row is not +0"
    ops.rope_check(DEV)
    with pytest.raises(TypeError):
        ops.rope(q, k, cos, sin, safe, q_len=ql.long())


def test_rope_refusals_are_status_codes_not_reads():
    """a position outside the table: the row is written as zeros, nothing is read, and `vlmc_rope_status` returns VLMC_EINVAL with an
    error string; head_dim not a multiple of 8 and a null pointer are refused by the entry point"""
    import ctypes
    from vlmc import _lib, ops
    g, q, k, cos, sin, P = _inputs(torch.bfloat16, 64, B=2, H=4, T=9, P=40, seed=9)
    pos = torch.randint(0, P, (2, 9), generator=g, device=DEV)
    ops.rope_check(DEV)
    good_q, _ = ops.rope(q, k, cos, sin, pos)
    bad = pos.clone()
    bad[1, 3], bad[0, 8] = P, -1                                                            # one past the cut table, and a negative one
    out_q, out_k = ops.rope(q, k, cos, sin, bad)
    with pytest.raises(_lib.VlmcError, match="outside the cos / sin table") as e:
        ops.rope_check(DEV)
    assert e.value.code == _lib.VLMC_EINVAL
    ops.rope_check(DEV)                                                                     # reported once, then clear
    assert bool((_bits(out_q[1, :, 3]) == 0).all()) and bool((_bits(out_k[0, :, 8]) == 0).all())
    keep = torch.ones(2, 9, dtype=torch.bool, device=DEV)
    keep[1, 3] = keep[0, 8] = False
    assert torch.equal(_bits(out_q.transpose(1, 2)[keep]), _bits(good_q.transpose(1, 2)[keep]))
    lib = _lib.load()
    I3 = ctypes.c_int64 * 3
    st = I3(1, 1, 1)
    qo, ko = torch.empty_like(q.contiguous()), torch.empty_like(q.contiguous())
    args = lambda d, qp: (qp, k.data_ptr(), qo.data_ptr(), ko.data_ptr(), _lib.BF16, 2, 4, 9, d, st, st, st, cos.data_ptr(), sin.data_ptr(), P, 64,
                          pos.data_ptr(), 9, 1, None, None, None)
    assert lib.vlmc_rope(*args(60, q.data_ptr())) == _lib.VLMC_EINVAL and b"multiple of 8" in lib.vlmc_last_error()
    assert lib.vlmc_rope(*args(136, q.data_ptr())) == _lib.VLMC_EINVAL and b"at most 128" in lib.vlmc_last_error()
    assert lib.vlmc_rope(*args(64, None)) == _lib.VLMC_EINVAL and b"null pointer" in lib.vlmc_last_error()
    assert lib.vlmc_rope_status(None, None) == _lib.VLMC_EINVAL and b"null pointer" in lib.vlmc_last_error()
    with pytest.raises(TypeError):
        ops.rope(q, k, cos.float(), sin.float(), pos)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.rope(q.cpu(), k.cpu(), cos.cpu(), sin.cpu(), pos.cpu())
