"""CPU-only: the tiled packed linears' entry points (include/vlmc.h: vlmc_linear_fwd_24_tiled, vlmc_linear_fwd_48_tiled and the row
limit vlmc_linear_fwd_24_tiled_max_rows) are declared and exported, validate their arguments without touching a device and name
themselves in every refusal; the `tiled` keyword of `ops.linear_fwd_24` / `ops.linear_fwd_48` refuses `unpack=True` and CPU tensors."""
import ctypes

import pytest
import torch

from vlmc import _lib

N, K = 32, 64
EXPORTS = ["vlmc_linear_fwd_24_tiled", "vlmc_linear_fwd_48_tiled"]


def _bufs():
    """Host buffers of the right sizes: every call below must fail before anything is dereferenced."""
    x = ctypes.create_string_buffer(16 * K * 2 + 32)
    values = ctypes.create_string_buffer(N * K + 32)
    meta = ctypes.create_string_buffer(N * K // 8)
    y = ctypes.create_string_buffer(128 * N * 2)
    align = lambda b: (ctypes.addressof(b) + 15) // 16 * 16
    return (x, values, meta, y), dict(X=align(x), values=align(values), meta=ctypes.addressof(meta), bias=None, dtype=_lib.F16, M=1, N=N, K=K,
                                      ldx=K, Y=ctypes.addressof(y), ldy=N, stream=None)


def _call(lib, fn, a):
    return getattr(lib, fn)(a["X"], a["values"], a["meta"], a["bias"], a["dtype"], a["M"], a["N"], a["K"], a["ldx"], a["Y"], a["ldy"], a["stream"])


def test_the_new_exports_are_declared_and_the_abi_moved_on():
    declared = set(_lib.header_functions())
    assert set(EXPORTS) | {"vlmc_linear_fwd_24_tiled_max_rows"} <= declared
    assert _lib.header_abi_version() >= 27                                             # the parent's is 26
    lib = _lib.load()
    for fn in EXPORTS + ["vlmc_linear_fwd_24_tiled_max_rows"]:
        assert callable(getattr(lib, fn))
    assert _lib.SIGNATURES["vlmc_linear_fwd_48_tiled"] == _lib.SIGNATURES["vlmc_linear_fwd_24_tiled"]
    # vlmc_linear_fwd_24's arguments without the workspace and its size
    old = _lib.SIGNATURES["vlmc_linear_fwd_24"]
    assert _lib.SIGNATURES["vlmc_linear_fwd_24_tiled"] == (old[0], old[1][:11] + old[1][13:])


def test_the_row_limit_is_zero_or_above_the_packed_kernels():
    from vlmc import ops
    lib = _lib.load()
    limit = lib.vlmc_linear_fwd_24_tiled_max_rows()
    assert limit == 0 or limit >= lib.vlmc_linear_fwd_24_max_rows()
    assert ops.linear_fwd_24_tiled_max_rows() == limit


CHANGES = [dict(dtype=_lib.F32), dict(K=12, ldx=16), dict(ldx=K + 4), dict(ldx=K - 8), dict(ldy=N - 1), dict(M=0), dict(X=None), dict(values=None),
           dict(meta=None), dict(Y=None), "X+2", "values+4"]
IDS = ["f32", "K_12", "ldx_not_8", "ldx_below_K", "ldy_below_N", "M_0", "null_X", "null_values", "null_meta", "null_Y", "X_misaligned_2",
       "values_misaligned_4"]


@pytest.mark.parametrize("fn", EXPORTS)
@pytest.mark.parametrize("change", CHANGES, ids=IDS)
def test_bad_arguments_are_refused_before_any_launch(change, fn):
    lib = _lib.load()
    keep, a = _bufs()
    if change == "X+2":
        a["X"] += 2
    elif change == "values+4":
        a["values"] += 4
    else:
        a.update(change)
    assert _call(lib, fn, a) == _lib.VLMC_EINVAL
    assert fn.encode() in lib.vlmc_last_error()
    del keep


def _packed_cpu():
    return torch.zeros(1, 16, dtype=torch.float16), torch.zeros(4, 8, dtype=torch.float16), torch.zeros(4, 2, dtype=torch.uint8)


@pytest.mark.parametrize("name", ["linear_fwd_24", "linear_fwd_48"])
def test_unpack_and_tiled_together_raise(name):
    from vlmc import ops
    x, values, meta = _packed_cpu()
    with pytest.raises(ValueError, match="tiled"):
        getattr(ops, name)(x, values, meta, unpack=True, tiled=True)


@pytest.mark.parametrize("name", ["linear_fwd_24", "linear_fwd_48"])
@pytest.mark.parametrize("tiled", [True, False, None])
def test_ops_refuse_cpu_tensors_on_the_tiled_keyword(name, tiled):
    from vlmc import ops
    x, values, meta = _packed_cpu()
    with pytest.raises(RuntimeError, match="GPU only"):
        getattr(ops, name)(x, values, meta, tiled=tiled)
    with pytest.raises(RuntimeError, match="GPU only"):
        getattr(ops, name)(x, values, meta, torch.zeros(4, dtype=torch.float16), tiled=tiled)
    assert callable(ops.linear_fwd_24_tiled_max_rows)
