"""Operands at a chosen pitch and pointer offset inside one larger torch allocation, for the tests of the kernel paths that are picked by
operand LAYOUT (tests/test_layout_paths_gpu.py, profiles/layout_paths.md).

`placed(t, ld, offset_elems)` copies the values of `t` (1-D, or 2-D with rows `ld` elements apart) into a fresh backing tensor whose
every other element holds a sentinel bit pattern -- a NaN with a payload for the float types, 0xA5 in every byte otherwise -- with the
first element `offset_elems` elements past a 256-byte boundary.  `untouched(backing, view)` then says whether everything around the view
still holds the sentinel: a store one element past a row, into the pitch gap or in front of the operand shows.  The view lies wholly inside
the backing allocation; nothing here looks at memory it does not own."""
import torch

ALIGN = 256                       # bytes
_TAIL = 64                        # sentinel elements behind the last row (the last row's pitch gap and a little more)

# dtype -> (integer dtype of the same width, sentinel bits)
_BITS = {
    torch.float32: (torch.int32, 0x7FC0A5A5),                 # quiet NaN, payload 0xA5A5
    torch.float16: (torch.int16, 0x7EA5),                     # quiet NaN, payload 0xA5
    torch.bfloat16: (torch.int16, 0x7FE5),                    # quiet NaN, payload 0x25
    torch.uint8: (torch.uint8, 0xA5),
    torch.bool: (torch.uint8, 0xA5),
    torch.int32: (torch.int32, 0xA5A5A5A5 - (1 << 32)),
    torch.int64: (torch.int64, 0xA5A5A5A5A5A5A5A5 - (1 << 64)),
    torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5),
}


def sentinel(dtype):
    return _BITS[dtype][1]


def bits(t):
    """The raw integer bits of `t` (same shape and strides)."""
    idt = _BITS[t.dtype][0]
    return t.view(idt) if t.dtype != idt else t


def placed(t, ld=None, offset_elems=0):
    """(view, backing): `view` has t's shape, dtype and values, unit stride along the last dimension, rows `ld` elements apart (2-D; default
    the width) and view.data_ptr() == a 256-byte boundary + offset_elems * itemsize.  `backing` is the flat integer tensor that holds it."""
    assert t.dim() in (1, 2) and offset_elems >= 0
    idt, sent = _BITS[t.dtype]
    item = t.element_size()
    rows, width = (1, t.shape[0]) if t.dim() == 1 else t.shape
    ld = width if ld is None else int(ld)
    assert ld >= width
    per = ALIGN // item
    backing = torch.full((2 * per + offset_elems + rows * ld + _TAIL,), sent, dtype=idt, device=t.device)
    lead = (-backing.data_ptr() % ALIGN) // item + per                    # a whole sentinel block in front of the operand as well
    start = lead + offset_elems
    shape, strides = ((width,), (1,)) if t.dim() == 1 else ((rows, width), (ld, 1))
    raw = backing.as_strided(shape, strides, start)
    raw.copy_(bits(t.contiguous()))
    view = raw if t.dtype == idt else raw.view(t.dtype)
    assert view.data_ptr() % ALIGN == (offset_elems * item) % ALIGN and view.shape == t.shape
    return view, backing


def _inside(backing, view):
    item = backing.element_size()
    off = view.data_ptr() - backing.data_ptr()
    assert off % item == 0 and view.element_size() == item
    inside = torch.zeros(backing.numel(), dtype=torch.bool, device=backing.device)
    inside.as_strided(tuple(view.shape), tuple(view.stride()), off // item).fill_(True)
    return inside


def untouched(backing, view):
    """Every element of `backing` that is not an element of `view` still holds the sentinel, compared as raw integer bits."""
    outside = backing[~_inside(backing, view)]
    return bool((outside == sentinel(view.dtype)).all())

