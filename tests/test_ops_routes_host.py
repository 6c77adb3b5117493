"""CPU-only: the pieces the two host routes of vlmc/ops.py share -- the rows view both flavours of which every launch goes through, and
the signatures that make the ctypes back end and the compiled one (csrc/fastpath/fast_bind.cpp) interchangeable."""
import inspect
import os
import re

import pytest
import torch

from vlmc import ops

FAST_BIND = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vlm-compression_amd", "csrc", "fastpath", "fast_bind.cpp")


def _view(x, n, aligned):
    """(copied, rows, ld) of `ops._rows`, after checking that what comes back holds x's values as unit-stride rows ld apart."""
    x2, rows, ld = ops._rows(x, n, aligned)
    assert x2.shape == (rows, n) and torch.equal(x2, x.reshape(-1, n)) and (x2.stride(1) == 1 or n == 1)
    assert ld >= n and (rows <= 1 or ld == x2.stride(0))
    return x2.data_ptr() != x.data_ptr(), rows, ld


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_rows_view_copies_only_what_a_kernel_cannot_read(dtype):
    """The loose flavour wants unit stride along n and rows that do not overlap, and says ld = n for a single row; the aligned one
    (the 16-bit GEMMs) also wants the rows a multiple of 8 elements apart and a 16-byte-aligned pointer, and reports the stride."""
    per16 = 16 // torch.empty(0, dtype=dtype).element_size()                # elements in 16 bytes
    base = torch.arange(6 * 48, dtype=torch.float32).to(dtype)
    assert base.data_ptr() % 16 == 0
    x = base.reshape(3, 2, 48)
    assert _view(x, 48, False) == (False, 6, 48) and _view(x, 48, True) == (False, 6, 48)                    # contiguous
    cols = base.reshape(6, 48)[:, 16:32]                                                                     # a column slice
    assert _view(cols, 16, False) == (False, 6, 48) and _view(cols, 16, True) == (False, 6, 48)
    odd = base[:6 * 44].reshape(6, 44)[:, :16]                                                               # rows 44 apart: not 8 | ld
    assert _view(odd, 16, False) == (False, 6, 44) and _view(odd, 16, True) == (True, 6, 16)
    inner = base.reshape(6, 48)[:, ::2]                                                                      # no unit stride
    assert _view(inner, 24, False) == (True, 6, 24) and _view(inner, 24, True) == (True, 6, 24)
    row = base[:16].reshape(1, 16).expand(5, 16)                                                             # stride(0) == 0 < n
    assert _view(row, 16, False) == (True, 5, 16) and _view(row, 16, True) == (True, 5, 16)
    off = base.reshape(6, 48)[:, per16 // 2:per16 // 2 + 16]                                                 # 8 bytes into a 16-byte line
    assert off.data_ptr() % 16 == 8
    assert _view(off, 16, False) == (False, 6, 48) and _view(off, 16, True) == (True, 6, 16)
    packed = base[per16 // 2:per16 // 2 + 6 * 16].reshape(6, 16)              # the same offset, contiguous: `.contiguous()` has nothing to
    assert packed.data_ptr() % 16 == 8                                       # copy, the view comes back as it is (the entry point refuses it)
    assert _view(packed, 16, False) == (False, 6, 16) and _view(packed, 16, True) == (False, 6, 16)
    for wide in (48, 44):                                                                                    # M = 1, a column slice:
        one = base[:wide].reshape(1, wide)[:, 8:24]                                                          # read in place, ld = n
        assert one.stride(0) == wide and _view(one, 16, False) == (False, 1, 16) and _view(one, 16, True) == (False, 1, 16)
    assert _view(base[:16], 16, False) == (False, 1, 16) and _view(base[:16], 16, True) == (False, 1, 16)    # 1-D


def test_ctypes_back_end_mirrors_the_compiled_signatures():
    """Every entry point of the compiled module has a ctypes counterpart with the same parameter names in the same order, and both
    lists are `_FAST_ENTRY_POINTS`: the public ops call `(_fast or _ctypes_route).op(...)` positionally."""
    src = open(FAST_BIND).read()
    defs = {name: re.findall(r'py::arg\("(\w+)"\)', args)
            for name, args in re.findall(r'm\.def\(\s*"(\w+)"\s*,\s*&\w+((?:\s*,\s*py::arg\("\w+"\))*)\s*\)', src)}
    assert sorted(defs) == sorted(ops._FAST_ENTRY_POINTS), "fast_bind.cpp registers other entry points than ops._FAST_ENTRY_POINTS names"
    for name in ops._FAST_ENTRY_POINTS:
        params = list(inspect.signature(getattr(ops._ctypes_route, name)).parameters)
        assert params == defs[name] and params[-1] == "stream", (name, params, defs[name])
    if ops._fast is not None:
        for name in ops._FAST_ENTRY_POINTS:
            assert callable(getattr(ops._fast, name))
    public = [n for n in dir(ops._ctypes_route) if not n.startswith("_")]
    assert sorted(public) == sorted(ops._FAST_ENTRY_POINTS)


def test_back_ends_answer_none_for_cpu_tensors_and_the_fronts_raise():
    """No host pointer reaches a launch: each back end checks the device of every tensor itself and answers None (the fronts test the
    first tensor only, and only to keep from asking for a stream without a GPU); the fronts raise RuntimeError, or answer None
    under `_try`."""
    x, w = torch.randn(4, 64), torch.randn(8, 64)
    xh, wh = x.half(), w.half()
    rowmap = torch.arange(4, dtype=torch.int32)
    q = torch.randn(1, 2, 5, 16).half()
    calls = {"linear_fwd": [(xh, wh, None), (x, w, None)], "linear_fwd_group": [(xh, [wh], [None])], "linear_fwd_rows": [(xh, [wh], [None], rowmap, 4)],
             "attn_matmul": [(xh[None], wh.t()[None])], "row_mean": [(x, False)], "rms_norm": [(xh, torch.ones(64).half(), 1e-6, 0)],
             "sdpa": [(q, q, q, 0.25, False)]}
    assert sorted(calls) == sorted(ops._FAST_ENTRY_POINTS)
    for back_end in filter(None, (ops._fast, ops._ctypes_route)):
        for name, argss in calls.items():
            for args in argss:
                assert getattr(back_end, name)(*args, 0) is None, (back_end, name)
    for name, argss in calls.items():
        for args in argss:
            with pytest.raises(RuntimeError, match="GPU only"):
                getattr(ops, name)(*args)
    assert ops.linear_fwd(xh, wh, _try=True) is None and ops.attn_matmul(xh[None], wh.t()[None], _try=True) is None
    assert ops.sdpa(q, q, q, _try=True) is None
