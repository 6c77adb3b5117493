"""CPU-only: the packed 4:8 linear's entry point (include/vlmc.h: vlmc_linear_fwd_48) validates its arguments without touching a
device and names itself in every refusal, the row limit and the workspace it is held to are the ones vlmc_linear_fwd_24's queries
report, and a `Linear48` carries exactly the packed state-dict keys and refuses what a `Linear24` refuses."""
import ctypes

import pytest
import torch

from vlmc import _lib

N, K = 32, 64


def _bufs():
    """Host buffers of the right sizes: every call below must fail before anything is dereferenced."""
    x = ctypes.create_string_buffer(16 * K * 2 + 16)
    values = ctypes.create_string_buffer(N * K)
    meta = ctypes.create_string_buffer(N * K // 8)
    y = ctypes.create_string_buffer(128 * N * 2)
    align = lambda b: (ctypes.addressof(b) + 15) // 16 * 16
    return (x, values, meta, y), dict(X=align(x), values=align(values), meta=ctypes.addressof(meta), bias=None, dtype=_lib.F16, M=1, N=N, K=K,
                                      ldx=K, Y=ctypes.addressof(y), ldy=N, workspace=None, workspace_bytes=0, stream=None)


def _call(lib, a):
    return lib.vlmc_linear_fwd_48(a["X"], a["values"], a["meta"], a["bias"], a["dtype"], a["M"], a["N"], a["K"], a["ldx"], a["Y"], a["ldy"],
                                  a["workspace"], a["workspace_bytes"], a["stream"])


def test_the_new_exports_are_declared_and_the_abi_moved_on():
    declared = _lib.header_functions()
    assert {"vlmc_pack_48", "vlmc_unpack_48", "vlmc_linear_fwd_48"} <= set(declared) and _lib.header_abi_version() >= 25
    assert _lib.SIGNATURES["vlmc_linear_fwd_48"] == _lib.SIGNATURES["vlmc_linear_fwd_24"]
    assert _lib.SIGNATURES["vlmc_pack_48"] == _lib.SIGNATURES["vlmc_pack_24"] and _lib.SIGNATURES["vlmc_unpack_48"] == _lib.SIGNATURES["vlmc_unpack_24"]


@pytest.mark.parametrize("change", [dict(X=None), dict(values=None), dict(meta=None), dict(Y=None), dict(dtype=_lib.F32), dict(K=12, ldx=16),
                                    dict(ldx=K - 8), dict(M=0)],
                         ids=["null_X", "null_values", "null_meta", "null_Y", "f32", "K_12", "ldx_below_K", "M_0"])
def test_bad_arguments_are_refused_before_any_launch(change):
    lib = _lib.load()
    keep, a = _bufs()
    a.update(change)
    assert _call(lib, a) == _lib.VLMC_EINVAL
    assert b"vlmc_linear_fwd_48" in lib.vlmc_last_error()
    del keep


def test_rows_above_max_rows_need_the_workspace():
    lib = _lib.load()
    keep, a = _bufs()
    mr = lib.vlmc_linear_fwd_24_max_rows()                                             # one limit, one workspace rule for both formats
    need = lib.vlmc_linear_fwd_24_workspace(mr + 1, N, K)
    assert need >= N * K * 2
    ws = ctypes.create_string_buffer(need + 16)
    a.update(M=mr + 1)
    assert _call(lib, a) == _lib.VLMC_EINVAL and b"vlmc_linear_fwd_48" in lib.vlmc_last_error()      # NULL workspace
    a.update(workspace=(ctypes.addressof(ws) + 15) // 16 * 16, workspace_bytes=need - 1)
    assert _call(lib, a) == _lib.VLMC_EINVAL and b"workspace" in lib.vlmc_last_error()  # short by one byte
    assert b"vlmc_linear_fwd_48" in lib.vlmc_last_error()
    del keep


@pytest.mark.parametrize("fn", ["vlmc_pack_48", "vlmc_unpack_48"])
def test_pack_and_unpack_refuse_like_their_2_4_siblings(fn):
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    args = dict(vlmc_pack_48=lambda dtype=_lib.F16, in_f=16, ld=16, w=p: (w, dtype, 4, in_f, ld, p, ld, p, p, p, None),
                vlmc_unpack_48=lambda dtype=_lib.F16, in_f=16, ld=16, w=p: (p, p, dtype, 4, in_f, w, ld, p, ld, p, None))[fn]
    for bad in (dict(dtype=_lib.F32), dict(in_f=12), dict(ld=8), dict(w=None)):
        assert getattr(lib, fn)(*args(**bad)) == _lib.VLMC_EINVAL and fn.encode() in lib.vlmc_last_error(), bad


def test_linear48_state_dict_and_refusals():
    from vlmc import formats
    from vlmc.packed48 import Linear48
    values = torch.zeros(8, 16, dtype=torch.bfloat16)
    meta = torch.full((8, 4), 105, dtype=torch.uint8)
    lin = Linear48(values, meta, torch.zeros(8, dtype=torch.bfloat16))
    assert (lin.in_features, lin.out_features) == (32, 8)
    assert list(lin.state_dict()) == [formats.PACKED_VALUES_48, formats.PACKED_META_48, "bias"] == ["weight_packed48", "weight_meta48", "bias"]
    assert list(Linear48(values, meta).state_dict()) == ["weight_packed48", "weight_meta48"]
    assert not list(lin.parameters())
    x = torch.zeros(3, 32, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        lin(x)
    with pytest.raises(RuntimeError, match="Linear48: dense"):
        lin(x, dense=True)
    with pytest.raises(TypeError, match="dtype"):
        lin(x.half())
    with pytest.raises(RuntimeError, match="Linear48 is inference only"):
        lin(x.clone().requires_grad_())
    with pytest.raises(TypeError, match="Linear48"):
        Linear48(values.float(), meta)
    with pytest.raises(TypeError):
        Linear48(values, meta[:, :3])
    with pytest.raises(TypeError):
        Linear48(values, meta, torch.zeros(7, dtype=torch.bfloat16))
    with pytest.raises(TypeError):
        Linear48(values, meta, torch.zeros(8, dtype=torch.float16))


def test_ops_refuse_cpu_tensors_and_name_the_4_8_functions():
    from vlmc import ops
    w, m = torch.zeros(4, 16, dtype=torch.float16), torch.ones(4, 16, dtype=torch.bool)
    for call in (lambda: ops.pack_48(w, m), lambda: ops.unpack_48(torch.zeros(4, 8, dtype=torch.float16), torch.zeros(4, 2, dtype=torch.uint8)),
                 lambda: ops.linear_fwd_48(torch.zeros(1, 16, dtype=torch.float16), torch.zeros(4, 8, dtype=torch.float16),
                                           torch.zeros(4, 2, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    assert not ops.linear_fwd_48_supported(torch.zeros(1, 16, dtype=torch.float16), torch.zeros(4, 8, dtype=torch.float16),
                                           torch.zeros(4, 2, dtype=torch.uint8))
