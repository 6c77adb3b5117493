"""CPU-only: the bitmap-packed linear's exports (include/vlmc.h: vlmc_pack_bm_rows, vlmc_pack_bm, vlmc_unpack_bm, vlmc_linear_fwd_bm and
its two queries) are declared and bound, validate their arguments without touching a device and name themselves in every refusal; the
format has a row limit of its own; a `LinearBM` carries exactly the four packed state-dict keys plus `bias` and refuses what a
`Linear24` refuses; the ops refuse CPU tensors by name."""
import ctypes

import pytest
import torch

from vlmc import _lib

N, K = 32, 64
NEW = ["vlmc_pack_bm_rows", "vlmc_pack_bm", "vlmc_unpack_bm", "vlmc_linear_fwd_bm_max_rows", "vlmc_linear_fwd_bm_workspace", "vlmc_linear_fwd_bm"]
ORDER = ("X", "values", "meta", "offs", "rowptr", "nnz", "bias", "dtype", "M", "N", "K", "ldx", "Y", "ldy", "workspace", "workspace_bytes", "stream")


def _bufs():
    """Host buffers of the right sizes: every call below must fail before anything is dereferenced."""
    raw = dict(X=ctypes.create_string_buffer(16 * K * 2 + 32), values=ctypes.create_string_buffer(N * K * 2 + 64),
               meta=ctypes.create_string_buffer(N * K // 8 + 16), offs=ctypes.create_string_buffer(N * 2 * 2), rowptr=ctypes.create_string_buffer(8 * (N + 1)),
               Y=ctypes.create_string_buffer(128 * N * 2))
    align = lambda b: (ctypes.addressof(b) + 15) // 16 * 16
    a = dict(X=align(raw["X"]), values=align(raw["values"]), meta=align(raw["meta"]), offs=ctypes.addressof(raw["offs"]),
             rowptr=ctypes.addressof(raw["rowptr"]), nnz=N * K // 2, bias=None, dtype=_lib.F16, M=1, N=N, K=K, ldx=K, Y=ctypes.addressof(raw["Y"]), ldy=N,
             workspace=None, workspace_bytes=0, stream=None)
    return raw, a


def _call(lib, a):
    return lib.vlmc_linear_fwd_bm(*(a[k] for k in ORDER))


def test_the_new_exports_are_declared_bound_and_the_abi_moved_on():
    declared = _lib.header_functions()
    assert set(NEW) <= set(declared) and set(NEW) <= set(_lib.SIGNATURES)
    assert _lib.header_abi_version() >= 26                                     # the parent's is 25
    lib = _lib.load()
    assert all(hasattr(lib, f) for f in NEW)
    assert len(_lib.SIGNATURES["vlmc_linear_fwd_bm"][1]) == len(ORDER) == len(_lib.SIGNATURES["vlmc_linear_fwd_24"][1]) + 3
    mr = lib.vlmc_linear_fwd_bm_max_rows()
    assert mr % 16 == 0 and 16 <= mr <= 64
    assert lib.vlmc_linear_fwd_bm_workspace(mr, N, K) == 0
    assert lib.vlmc_linear_fwd_bm_workspace(mr + 1, N, K) == lib.vlmc_linear_fwd_24_workspace(10 ** 6, N, K) >= N * K * 2


@pytest.mark.parametrize("change", [dict(X=None), dict(values=None), dict(meta=None), dict(offs=None), dict(rowptr=None), dict(Y=None),
                                    dict(dtype=_lib.F32), dict(K=12, ldx=16), dict(K=65536 + 8, ldx=65536 + 8), dict(ldx=K - 8), dict(ldx=K + 4),
                                    dict(M=0), dict(nnz=-1), dict(nnz=N * K + 1), dict(X="+2"), dict(values="+2"), dict(meta="+1")],
                         ids=["null_X", "null_values", "null_meta", "null_offs", "null_rowptr", "null_Y", "f32", "K_12", "K_above_65536", "ldx_below_K",
                              "ldx_not_8", "M_0", "nnz_negative", "nnz_above_NK", "X_misaligned", "values_misaligned", "meta_misaligned"])
def test_bad_arguments_are_refused_before_any_launch(change):
    lib = _lib.load()
    keep, a = _bufs()
    for k, v in change.items():
        a[k] = a[k] + int(v) if isinstance(v, str) else v
    assert _call(lib, a) == _lib.VLMC_EINVAL
    assert b"vlmc_linear_fwd_bm" in lib.vlmc_last_error()
    del keep


def test_rows_above_the_formats_own_limit_need_the_workspace():
    lib = _lib.load()
    keep, a = _bufs()
    mr = lib.vlmc_linear_fwd_bm_max_rows()
    need = lib.vlmc_linear_fwd_bm_workspace(mr + 1, N, K)
    assert need >= N * K * 2
    ws = ctypes.create_string_buffer(need + 16)
    a.update(M=mr + 1)
    assert _call(lib, a) == _lib.VLMC_EINVAL and b"vlmc_linear_fwd_bm" in lib.vlmc_last_error()      # NULL workspace
    a.update(workspace=(ctypes.addressof(ws) + 15) // 16 * 16, workspace_bytes=need - 1)
    assert _call(lib, a) == _lib.VLMC_EINVAL and b"workspace" in lib.vlmc_last_error()                # short by one byte
    assert b"vlmc_linear_fwd_bm" in lib.vlmc_last_error()
    del keep


@pytest.mark.parametrize("fn", ["vlmc_pack_bm_rows", "vlmc_pack_bm", "vlmc_unpack_bm"])
def test_pack_and_unpack_refuse_bad_arguments_by_name(fn):
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    args = dict(vlmc_pack_bm_rows=lambda dtype=_lib.F16, in_f=16, ld=16, w=p, nnz=8: (w, ld, 4, in_f, p, None),
                vlmc_pack_bm=lambda dtype=_lib.F16, in_f=16, ld=16, w=p, nnz=8: (w, dtype, 4, in_f, ld, p, ld, p, nnz, p, p, p, None),
                vlmc_unpack_bm=lambda dtype=_lib.F16, in_f=16, ld=16, w=p, nnz=8: (p, p, p, p, nnz, dtype, 4, in_f, w, ld, p, ld, p, None))[fn]
    bads = [dict(in_f=12), dict(ld=8), dict(w=None), dict(in_f=65536 + 8, ld=65536 + 8)]
    if fn != "vlmc_pack_bm_rows":
        bads += [dict(dtype=_lib.F32), dict(nnz=-1), dict(nnz=4 * 16 + 1)]
    for bad in bads:
        assert getattr(lib, fn)(*args(**bad)) == _lib.VLMC_EINVAL and fn.encode() in lib.vlmc_last_error(), bad


def _packed(out_f=8, in_f=32, dtype=torch.bfloat16):
    """an all-kept weight's four tensors (CPU)"""
    values = torch.zeros(out_f * in_f + 16, dtype=dtype)
    meta = torch.full((out_f, in_f // 8), 255, dtype=torch.uint8)
    offs = torch.zeros((out_f, (in_f + 31) // 32), dtype=torch.uint16)
    rowptr = torch.arange(out_f + 1, dtype=torch.int64) * in_f
    return values, meta, offs, rowptr


def test_linearbm_state_dict_and_refusals():
    from vlmc import formats
    from vlmc.packedbm import LinearBM
    values, meta, offs, rowptr = _packed()
    lin = LinearBM(values, meta, offs, rowptr, torch.zeros(8, dtype=torch.bfloat16))
    assert (lin.in_features, lin.out_features) == (32, 8)
    keys = [formats.PACKED_VALUES_BM, formats.PACKED_META_BM, formats.PACKED_OFFS_BM, formats.PACKED_ROWPTR_BM]
    assert keys == ["weight_packedbm", "weight_metabm", "weight_offsbm", "weight_rowptrbm"]
    assert list(lin.state_dict()) == keys + ["bias"]
    assert list(LinearBM(values, meta, offs, rowptr).state_dict()) == keys
    assert list(LinearBM(values, meta, offs, rowptr, bias=torch.zeros(8, dtype=torch.bfloat16)).state_dict()) == keys + ["bias"]
    assert not list(lin.parameters())
    x = torch.zeros(3, 32, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        lin(x)
    with pytest.raises(RuntimeError, match="LinearBM: dense"):
        lin(x, dense=True)
    with pytest.raises(TypeError, match="dtype"):
        lin(x.half())
    with pytest.raises(RuntimeError, match="LinearBM is inference only"):
        lin(x.clone().requires_grad_())
    with pytest.raises(TypeError, match="LinearBM"):
        LinearBM(values.float(), meta, offs, rowptr)
    for bad in ((values, meta[:4], offs, rowptr), (values, meta.to(torch.int8), offs, rowptr), (values, meta, offs.view(torch.int16), rowptr), (values, meta, offs, rowptr[:-1]),
                (values, meta, offs, rowptr.int()), (values[:8], meta, offs, rowptr), (values, meta, offs), (values.reshape(-1, 16), meta, offs, rowptr)):
        with pytest.raises(TypeError):
            LinearBM(*bad)
    with pytest.raises(TypeError):
        LinearBM(values, meta, offs, rowptr, torch.zeros(7, dtype=torch.bfloat16))
    with pytest.raises(TypeError):
        LinearBM(values, meta, offs, rowptr, torch.zeros(8, dtype=torch.float16))


def test_the_n_m_modules_kept_their_constructors():
    """`_PackedLinear` was generalised for the four-buffer format: the two-buffer modules keep their (values, meta, bias=None) signature"""
    from vlmc.packed24 import Linear24
    from vlmc.packed48 import Linear48
    values, meta, bias = torch.zeros(8, 16, dtype=torch.float16), torch.full((8, 4), 0x4e, dtype=torch.uint8), torch.zeros(8, dtype=torch.float16)
    for cls, names in ((Linear24, ["weight_packed24", "weight_meta24"]), (Linear48, ["weight_packed48", "weight_meta48"])):
        assert list(cls(values, meta).state_dict()) == names
        assert list(cls(values, meta, bias).state_dict()) == list(cls(values, meta, bias=bias).state_dict()) == names + ["bias"]
        assert list(cls(values, meta, None).state_dict()) == names
        with pytest.raises(TypeError):
            cls(values, meta, bias, bias)                                      # an explicit signature: two buffers and a bias, no more


def test_ops_refuse_cpu_tensors_and_name_the_bm_functions():
    from vlmc import ops
    values, meta, offs, rowptr = _packed(4, 16, torch.float16)
    w, m = torch.zeros(4, 16, dtype=torch.float16), torch.ones(4, 16, dtype=torch.bool)
    x = torch.zeros(1, 16, dtype=torch.float16)
    for call in (lambda: ops.pack_bm(w, m), lambda: ops.unpack_bm(values, meta, offs, rowptr), lambda: ops.linear_fwd_bm(x, values, meta, offs, rowptr)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    assert not ops.linear_fwd_bm_supported(x, values, meta, offs, rowptr)
    for name in ("pack_bm", "unpack_bm", "linear_fwd_bm", "linear_fwd_bm_supported", "linear_fwd_bm_max_rows"):
        assert callable(getattr(ops, name))
    assert ops.linear_fwd_bm_max_rows() == _lib.load().vlmc_linear_fwd_bm_max_rows()
