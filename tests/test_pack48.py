"""CPU-only: the packed 4:8 layout (include/vlmc.h: vlmc_pack_48 / vlmc_unpack_48).  The reference has no such format, so the pins
are the numpy restatement (tests/pack48_restatement.py) on a hand-written example and on the masks the REFERENCE's n:m rule
produced at 4:8 (tests/golden/wanda_unit.npz), and `mask_48_from_zeros` against those masks.  The kernels against the restatement:
tests/test_linear48_gpu.py.  Integer views, no tolerance."""
import numpy as np
import pytest
import torch

import golden_io
import pack48_restatement as pack48


def test_layout_on_a_hand_written_example():
    w = np.arange(1, 17, dtype=np.uint16).reshape(1, 16)
    keep = np.array([[1, 0, 0, 1, 0, 1, 1, 0,   0, 0, 1, 1, 1, 1, 0, 0]], dtype=bool)
    values, meta, bad = pack48.pack(w, keep)
    assert bad == 0
    assert values.tolist() == [[1, 4, 6, 7, 11, 12, 13, 14]]
    assert meta.tolist() == [[105, 60]]                                    # bit j = column 8c + j kept: 1 + 8 + 32 + 64, 4 + 8 + 16 + 32
    w2, k2, bad2 = pack48.unpack(values, meta)
    assert bad2 == 0 and np.array_equal(k2, keep) and np.array_equal(w2, np.where(keep, w, 0))
    assert pack48.pack(w, np.ones_like(keep))[2] == 2                     # not a 4:8 mask: every group of eight counted
    assert pack48.unpack(values, np.array([[255, 7]], dtype=np.uint8))[2] == 2


def _reference_48_prunes():
    """(name, keep, the reference's pruned weight as bit patterns of its own dtype, that weight) of every 2-D n:m case of the golden
    file whose mask keeps four of every eight"""
    g = golden_io.load("wanda_unit")
    for name in sorted({k.rsplit("/", 1)[0] for k in g if k.endswith("/mask")}):
        keep = g[f"{name}/mask"].bool()
        if keep.dim() != 2 or keep.shape[1] % 8 or not bool((keep.reshape(keep.shape[0], -1, 8).sum(-1) == 4).all()):
            continue
        wn = g[f"{name}/Wn"]
        dt = torch.float16 if "fp16" in name else torch.bfloat16
        yield name, keep, wn.to(dt).view(torch.int16).numpy().view(np.uint16), wn


def test_the_references_4_8_prunes_pack_and_round_trip():
    seen = []
    for name, keep, bits, _wn in _reference_48_prunes():
        k = keep.numpy()
        values, meta, bad = pack48.pack(bits, k)
        w2, k2, bad2 = pack48.unpack(values, meta)
        assert bad == 0 and bad2 == 0 and np.array_equal(k2, k), name
        assert np.array_equal(w2, np.where(k, bits, 0)) and np.array_equal(w2, bits), name
        assert values.size * 2 + meta.size == bits.size * 2 * 9 // 16
        seen.append(name)
    assert {"g4/bf16_4_8_t5", "g4/fp16_4_8_vit"} <= set(seen), seen
    assert len(seen) >= 2


def test_mask_from_zeros_reproduces_the_references_4_8_masks():
    from vlmc.packed48 import is_mask_48, mask_48_from_zeros
    seen = 0
    for name, keep, _bits, wn in _reference_48_prunes():
        got = mask_48_from_zeros(wn)
        four = ((wn != 0).reshape(wn.shape[0], -1, 8).sum(-1, keepdim=True) == 4).expand(-1, -1, 8).reshape(wn.shape)
        assert bool(four.any()) and torch.equal(got[four], keep[four]), name
        assert is_mask_48(got, wn.shape) and bool(got[wn != 0].all()), name
        assert is_mask_48(keep, wn.shape)
        seen += 1
    assert seen >= 2


def _groups(rows):
    return torch.tensor(rows, dtype=torch.float32)


def test_mask_from_zeros_fills_up_with_the_lowest_zero_columns():
    from vlmc.packed48 import mask_48_from_zeros
    w = _groups([[0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 5, 0, 7, 0, 0, 0,   0, 3, 0, 4, 1, 2, 0, 0,   9, 0, 0, 0, 0, 0, 8, 7]])
    want = [[1, 1, 1, 1, 0, 0, 0, 0,   1, 1, 1, 0, 1, 0, 0, 0,   0, 1, 0, 1, 1, 1, 0, 0,   1, 1, 0, 0, 0, 0, 1, 1]]
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        m = mask_48_from_zeros(w.to(dt))
        assert m.dtype == torch.bool and m.tolist() == [[bool(v) for v in want[0]]]
        assert bool((m.reshape(1, -1, 8).sum(-1) == 4).all()) and bool(m[w != 0].all())
    # -0.0 is a zero: the three lowest zero columns (0, 1 = -0.0, 2) fill up the one non-zero
    assert mask_48_from_zeros(_groups([[0, -0.0, 0, 0, 0, 0, 0, 1]])).tolist() == [[True, True, True, False, False, False, False, True]]


def test_mask_from_zeros_counts_the_groups_that_are_not_4_8():
    from vlmc.packed48 import mask_48_from_zeros
    w = _groups([[1, 2, 3, 0, 4, 5, 0, 0,   0, 0, 1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1, 1, 1,   0, 2, 2, 2, 0, 0, 2, 2]])
    with pytest.raises(ValueError, match="3 groups of eight"):
        mask_48_from_zeros(w)
    with pytest.raises(ValueError):
        mask_48_from_zeros(torch.zeros(2, 12))


def test_every_2_4_mask_is_a_4_8_mask_and_validity_of_metadata():
    from vlmc.packed24 import is_mask_24
    from vlmc.packed48 import is_mask_48, meta_48_is_valid
    m24 = torch.tensor([True, False, False, True, False, True, True, False]).repeat(3, 2)
    assert is_mask_24(m24, m24.shape) and is_mask_48(m24, m24.shape)
    m48 = torch.tensor([True, True, True, True, False, False, False, False]).repeat(3, 2)
    assert is_mask_48(m48, m48.shape) and not is_mask_24(m48, m48.shape)
    assert not is_mask_48(m48[:, :12], (3, 12)) and not is_mask_48(m48.to(torch.uint8), m48.shape)
    every = torch.arange(256, dtype=torch.uint8)
    valid = [b for b in range(256) if meta_48_is_valid(every[b:b + 1])]
    assert len(valid) == 70 and all(bin(b).count("1") == 4 for b in valid)
    assert meta_48_is_valid(torch.tensor([[105, 60]], dtype=torch.uint8)) and not meta_48_is_valid(torch.tensor([[105, 0]], dtype=torch.uint8))
