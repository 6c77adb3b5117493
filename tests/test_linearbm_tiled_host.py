"""CPU-only: the tiled bitmap-packed linear's entry points (include/vlmc.h: vlmc_linear_fwd_bm_tiled and the row limit
vlmc_linear_fwd_bm_tiled_max_rows) are declared, exported and bound, validate their arguments without touching a device and name
themselves in every refusal; the `tiled` keyword of `ops.linear_fwd_bm` refuses `unpack=True` and CPU tensors."""
import ctypes

import pytest
import torch

from vlmc import _lib

N, K = 32, 64
FN = "vlmc_linear_fwd_bm_tiled"
ORDER = ("X", "values", "meta", "offs", "rowptr", "nnz", "bias", "dtype", "M", "N", "K", "ldx", "Y", "ldy", "stream")


def _bufs():
    """Host buffers of the right sizes: every call below must fail before anything is dereferenced."""
    raw = dict(X=ctypes.create_string_buffer(16 * K * 2 + 32), values=ctypes.create_string_buffer(N * K * 2 + 64),
               meta=ctypes.create_string_buffer(N * K // 8 + 16), offs=ctypes.create_string_buffer(N * 2 * 2), rowptr=ctypes.create_string_buffer(8 * (N + 1)),
               Y=ctypes.create_string_buffer(128 * N * 2))
    align = lambda b: (ctypes.addressof(b) + 15) // 16 * 16
    a = dict(X=align(raw["X"]), values=align(raw["values"]), meta=align(raw["meta"]), offs=ctypes.addressof(raw["offs"]),
             rowptr=ctypes.addressof(raw["rowptr"]), nnz=N * K // 2, bias=None, dtype=_lib.F16, M=1, N=N, K=K, ldx=K, Y=ctypes.addressof(raw["Y"]), ldy=N,
             stream=None)
    return raw, a


def test_the_new_exports_are_declared_bound_and_the_abi_moved_on():
    new = [FN, "vlmc_linear_fwd_bm_tiled_max_rows"]
    assert set(new) <= set(_lib.header_functions()) and set(new) <= set(_lib.SIGNATURES)
    assert _lib.header_abi_version() >= 29                                             # the parent's is 28
    lib = _lib.load()
    for fn in new:
        assert callable(getattr(lib, fn))
    # vlmc_linear_fwd_bm's arguments without the workspace and its size
    old = _lib.SIGNATURES["vlmc_linear_fwd_bm"]
    assert len(old[1]) == len(ORDER) + 2
    assert _lib.SIGNATURES[FN] == (old[0], old[1][:14] + old[1][16:])
    assert _lib.SIGNATURES["vlmc_linear_fwd_bm_tiled_max_rows"] == _lib.SIGNATURES["vlmc_linear_fwd_bm_max_rows"]


def test_the_row_limit_is_zero_or_above_the_packed_kernels():
    from vlmc import ops
    lib = _lib.load()
    limit = lib.vlmc_linear_fwd_bm_tiled_max_rows()
    assert limit == 0 or limit >= lib.vlmc_linear_fwd_bm_max_rows()
    assert ops.linear_fwd_bm_tiled_max_rows() == limit


# the n:m tiled entry points' table (the format asks 4-byte alignment of values, so that row moves values by 2 bytes, not 4), then what
# the bitmap format adds
CHANGES = [dict(dtype=_lib.F32), dict(K=12, ldx=16), dict(ldx=K + 4), dict(ldx=K - 8), dict(ldy=N - 1), dict(M=0), dict(X=None), dict(values=None),
           dict(meta=None), dict(Y=None), dict(X="+2"), dict(values="+2"),
           dict(offs=None), dict(rowptr=None), dict(nnz=-1), dict(meta="+2"), dict(nnz=N * K + 1), dict(K=65536 + 8, ldx=65536 + 8)]
IDS = ["f32", "K_12", "ldx_not_8", "ldx_below_K", "ldy_below_N", "M_0", "null_X", "null_values", "null_meta", "null_Y", "X_misaligned_2",
       "values_misaligned_2", "null_offs", "null_rowptr", "nnz_negative", "meta_misaligned_2", "nnz_above_NK", "K_above_65536"]


@pytest.mark.parametrize("change", CHANGES, ids=IDS)
def test_bad_arguments_are_refused_before_any_launch(change):
    lib = _lib.load()
    keep, a = _bufs()
    for k, v in change.items():
        a[k] = a[k] + int(v) if isinstance(v, str) else v
    assert getattr(lib, FN)(*(a[k] for k in ORDER)) == _lib.VLMC_EINVAL
    assert FN.encode() in lib.vlmc_last_error()
    del keep


def test_rows_above_the_packed_kernels_limit_are_not_refused_for_their_number():
    """any M >= 1: with M far above every row limit the first complaint is still the bad argument, never the rows or a workspace"""
    lib = _lib.load()
    keep, a = _bufs()
    a.update(M=100000, nnz=-1)
    assert getattr(lib, FN)(*(a[k] for k in ORDER)) == _lib.VLMC_EINVAL
    assert b"nnz" in lib.vlmc_last_error() and b"workspace" not in lib.vlmc_last_error()
    del keep


def _packed_cpu(out_f=4, in_f=16, dtype=torch.float16):
    """an all-kept weight's four tensors and one row of x (CPU)"""
    values = torch.zeros(out_f * in_f + 16, dtype=dtype)
    meta = torch.full((out_f, in_f // 8), 255, dtype=torch.uint8)
    offs = torch.zeros((out_f, (in_f + 31) // 32), dtype=torch.uint16)
    rowptr = torch.arange(out_f + 1, dtype=torch.int64) * in_f
    return torch.zeros(1, in_f, dtype=dtype), values, meta, offs, rowptr


def test_unpack_and_tiled_together_raise():
    from vlmc import ops
    with pytest.raises(ValueError, match="tiled"):
        ops.linear_fwd_bm(*_packed_cpu(), unpack=True, tiled=True)


@pytest.mark.parametrize("tiled", [True, False, None])
def test_ops_refuse_cpu_tensors_on_the_tiled_keyword(tiled):
    from vlmc import ops
    packed = _packed_cpu()
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.linear_fwd_bm(*packed, tiled=tiled)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.linear_fwd_bm(*packed, torch.zeros(4, dtype=torch.float16), tiled=tiled)
    assert callable(ops.linear_fwd_bm_tiled_max_rows)
