"""CPU-only: the packed-linear entry points (include/vlmc.h: vlmc_linear_fwd_24 and its two queries) validate their arguments
without touching a device, `mask_24_from_zeros` rebuilds 2:4 masks from kept zeros, and a `Linear24` carries exactly the packed
state-dict keys."""
import ctypes

import pytest
import torch

import golden_io
from vlmc import _lib

N, K = 32, 64


def _bufs():
    """Host buffers of the right sizes: every call below must fail (or be a pure query) before anything is dereferenced."""
    x = ctypes.create_string_buffer(16 * K * 2 + 16)
    values = ctypes.create_string_buffer(N * K)
    meta = ctypes.create_string_buffer(N * K // 8)
    y = ctypes.create_string_buffer(128 * N * 2)
    align = lambda b: (ctypes.addressof(b) + 15) // 16 * 16
    return (x, values, meta, y), dict(X=align(x), values=align(values), meta=ctypes.addressof(meta), bias=None, dtype=_lib.F16, M=1, N=N, K=K,
                                      ldx=K, Y=ctypes.addressof(y), ldy=N, workspace=None, workspace_bytes=0, stream=None)


def _call(lib, a):
    return lib.vlmc_linear_fwd_24(a["X"], a["values"], a["meta"], a["bias"], a["dtype"], a["M"], a["N"], a["K"], a["ldx"], a["Y"], a["ldy"],
                                  a["workspace"], a["workspace_bytes"], a["stream"])


def test_max_rows_and_workspace_queries():
    lib = _lib.load()
    mr = lib.vlmc_linear_fwd_24_max_rows()
    assert mr >= 16 and mr % 16 == 0
    assert lib.vlmc_linear_fwd_24_workspace(1, 4096, 4096) == 0
    assert lib.vlmc_linear_fwd_24_workspace(mr, 4096, 4096) == 0
    assert lib.vlmc_linear_fwd_24_workspace(mr + 1, 4096, 4096) >= 4096 * 4096 * 2
    assert lib.vlmc_linear_fwd_24_workspace(mr + 1, 11008, 4096) >= 11008 * 4096 * 2


@pytest.mark.parametrize("change", [dict(X=None), dict(values=None), dict(meta=None), dict(Y=None), dict(dtype=_lib.F32), dict(K=12, ldx=16),
                                    dict(ldx=K - 8), dict(M=0)],
                         ids=["null_X", "null_values", "null_meta", "null_Y", "f32", "K_12", "ldx_below_K", "M_0"])
def test_bad_arguments_are_refused_before_any_launch(change):
    lib = _lib.load()
    keep, a = _bufs()
    a.update(change)
    assert _call(lib, a) == _lib.VLMC_EINVAL
    assert b"vlmc_linear_fwd_24" in lib.vlmc_last_error()
    del keep


def test_rows_above_max_rows_need_the_workspace():
    lib = _lib.load()
    keep, a = _bufs()
    mr = lib.vlmc_linear_fwd_24_max_rows()
    need = lib.vlmc_linear_fwd_24_workspace(mr + 1, N, K)
    ws = ctypes.create_string_buffer(need + 16)
    a.update(M=mr + 1)
    assert _call(lib, a) == _lib.VLMC_EINVAL                                           # NULL workspace
    a.update(workspace=(ctypes.addressof(ws) + 15) // 16 * 16, workspace_bytes=need - 1)
    assert _call(lib, a) == _lib.VLMC_EINVAL and b"workspace" in lib.vlmc_last_error()  # short by one byte
    del keep


def _groups(rows):
    return torch.tensor(rows, dtype=torch.float32)


def test_mask_from_zeros_fills_up_with_the_lowest_zero_columns():
    from vlmc.packed24 import mask_24_from_zeros
    w = _groups([[0, 0, 0, 0,   0, 0, 5, 0,   7, 0, 0, 0,   0, 3, 0, 4,   1, 2, 0, 0,   0, 0, 0, 9]])
    want = [[1, 1, 0, 0,   1, 0, 1, 0,   1, 1, 0, 0,   0, 1, 0, 1,   1, 1, 0, 0,   1, 0, 0, 1]]
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        m = mask_24_from_zeros(w.to(dt))
        assert m.dtype == torch.bool and m.tolist() == [[bool(v) for v in want[0]]]
        assert bool((m.reshape(1, -1, 4).sum(-1) == 2).all()) and bool(m[w != 0].all())
    assert mask_24_from_zeros(_groups([[0, -0.0, 0, 1]])).tolist() == [[True, False, False, True]]      # -0.0 is a zero


def test_mask_from_zeros_counts_the_groups_that_are_not_2_4():
    from vlmc.packed24 import mask_24_from_zeros
    w = _groups([[1, 2, 3, 0,   0, 0, 1, 1], [1, 1, 1, 1,   0, 2, 2, 2]])
    with pytest.raises(ValueError, match="3 groups"):
        mask_24_from_zeros(w)
    with pytest.raises(ValueError):
        mask_24_from_zeros(torch.zeros(2, 6))


def test_mask_from_zeros_reproduces_the_references_2_4_masks():
    from vlmc.packed24 import mask_24_from_zeros
    g = golden_io.load("wanda_unit")
    seen = 0
    for name in sorted({k.rsplit("/", 1)[0] for k in g if k.endswith("/mask")}):
        keep = g[f"{name}/mask"].bool()
        if keep.dim() != 2 or keep.shape[1] % 8 or not bool((keep.reshape(keep.shape[0], -1, 4).sum(-1) == 2).all()):
            continue
        wn = g[f"{name}/Wn"]                                                   # the reference's pruned weight: zeros where it pruned
        got = mask_24_from_zeros(wn)
        two = ((wn != 0).reshape(wn.shape[0], -1, 4).sum(-1, keepdim=True) == 2).expand(-1, -1, 4).reshape(wn.shape)
        assert bool(two.any()) and torch.equal(got[two], keep[two]), name
        assert bool((got.reshape(wn.shape[0], -1, 4).sum(-1) == 2).all()) and bool(got[wn != 0].all())
        seen += 1
    assert seen >= 1


def test_linear24_state_dict_and_cpu_refusal():
    from vlmc import formats
    from vlmc.packed24 import Linear24
    values = torch.zeros(8, 16, dtype=torch.bfloat16)
    meta = torch.full((8, 4), 4 | 4 << 4, dtype=torch.uint8)
    lin = Linear24(values, meta, torch.zeros(8, dtype=torch.bfloat16))
    assert (lin.in_features, lin.out_features) == (32, 8)
    assert list(lin.state_dict()) == [formats.PACKED_VALUES, formats.PACKED_META, "bias"] == ["weight_packed24", "weight_meta24", "bias"]
    assert list(Linear24(values, meta).state_dict()) == ["weight_packed24", "weight_meta24"]
    assert not list(lin.parameters())
    x = torch.zeros(3, 32, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        lin(x)
    with pytest.raises(RuntimeError, match="dense"):
        lin(x, dense=True)
    with pytest.raises(TypeError, match="dtype"):
        lin(x.half())
    with pytest.raises(RuntimeError, match="inference only"):
        lin(x.clone().requires_grad_())
    with pytest.raises(TypeError):
        Linear24(values.float(), meta)
    with pytest.raises(TypeError):
        Linear24(values, meta[:, :3])
