"""CPU-only: the packed bitmap ("bm") layout (include/vlmc.h: vlmc_pack_bm / vlmc_unpack_bm).  The reference has no such format, so the
pins are the numpy restatement (tests/packbm_restatement.py) on a hand-written example worked out below, its round trips, the lane-local
address formula of the forward kernel against the sequential unpack, the unstructured masks the REFERENCE's rule produced
(tests/golden/wanda_unit.npz), and `packedbm.meta_bm_is_valid`.  The kernels against the restatement: tests/test_linearbm_gpu.py.
Integer views, no tolerance."""
import numpy as np
import pytest
import torch

import golden_io
import packbm_restatement as packbm


def _cols(in_f, *kept):
    row = np.zeros(in_f, dtype=bool)
    row[list(kept)] = True
    return row


def test_layout_on_a_hand_written_example():
    """K = 40: five chunks, two steps, the second partial (one chunk).  w[r][c] = 40 r + c + 1.
    row 0  nothing kept
    row 1  chunk 0 full, chunk 1 empty, columns 16 19 | 31 | 32 39: 8 + 0 + 2 + 1 = 11 before step 1, 13 in all
    row 2  everything kept: starts at the ODD index 13
    row 3  columns 1 and 33: starts at 13 + 40 = 53, nnz = 55"""
    w = np.arange(1, 161, dtype=np.uint16).reshape(4, 40)
    keep = np.stack([_cols(40), _cols(40, 0, 1, 2, 3, 4, 5, 6, 7, 16, 19, 31, 32, 39), np.ones(40, dtype=bool), _cols(40, 1, 33)])
    values, meta, offs, rowptr = packbm.pack(w, keep)
    assert rowptr.tolist() == [0, 0, 13, 53, 55] and rowptr.dtype == np.int64
    assert values.tolist() == [41, 42, 43, 44, 45, 46, 47, 48, 57, 60, 72, 73, 80] + list(range(81, 121)) + [122, 154] + [0] * 16
    assert meta.tolist() == [[0, 0, 0, 0, 0], [255, 0, 9, 128, 129], [255] * 5, [2, 0, 0, 0, 2]]
    assert offs.tolist() == [[0, 0], [0, 11], [0, 32], [0, 1]] and offs.dtype == np.uint16
    assert values.size * 2 + meta.size + offs.size * 2 + rowptr.size * 8 == packbm.packed_bytes(4, 40, 55) == 71 * 2 + 20 + 16 + 40
    w2, k2, bad = packbm.unpack(values, meta, offs, rowptr)
    assert bad == 0 and np.array_equal(k2, keep) and np.array_equal(w2, np.where(keep, w, 0))
    assert np.array_equal(packbm.unpack_lane_local(values, meta, offs, rowptr), w2)
    # the first value of chunk 3 of row 1 (s = 0, q = 3): rowptr 0 + offs 0 + popcount(255, 0, 9) = 10 -> 72
    assert values[0 + 0 + 8 + 0 + 2] == 72
    # the first value of chunk 4 of row 3 (s = 1, q = 0): 53 + 1 + 0 -> 154
    assert values[53 + 1] == 154


def _random_case(out_f, in_f, seed, density=0.5, per_row=False):
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 65536, size=(out_f, in_f), dtype=np.uint16)
    if per_row:                                                              # exactly density * in_f kept in every row
        keep = np.zeros((out_f, in_f), dtype=bool)
        for r in range(out_f):
            keep[r, rng.permutation(in_f)[:int(in_f * density)]] = True
    else:
        keep = rng.random((out_f, in_f)) < density
    return w, keep


@pytest.mark.parametrize("out_f,in_f", [(5, 8), (33, 40), (17, 64), (33, 1408)])
def test_round_trips_and_the_lane_local_formula(out_f, in_f):
    w, keep = _random_case(out_f, in_f, seed=out_f * in_f, per_row=in_f == 1408)
    keep[0] = False                                                          # a row with nothing kept
    keep[out_f - 1] = True                                                   # a row with everything kept
    w[1, :8] = 0                                                             # kept zeros stay kept: positions come from the mask
    values, meta, offs, rowptr = packbm.pack(w, keep)
    nnz = int(keep.sum())
    assert values.size == nnz + 16 and rowptr[-1] == nnz and not values[nnz:].any()
    assert meta.shape == (out_f, in_f // 8) and offs.shape == (out_f, (in_f + 31) // 32)
    w2, k2, bad = packbm.unpack(values, meta, offs, rowptr)
    assert bad == 0 and np.array_equal(k2, keep) and np.array_equal(w2, np.where(keep, w, 0))
    assert np.array_equal(packbm.unpack_lane_local(values, meta, offs, rowptr), w2)
    if in_f == 1408:
        assert len(np.unique(meta[1:-1])) == 256                             # every metadata byte occurs


def _reference_unstructured_prunes():
    """(name, keep, the reference's pruned weight as bit patterns of its own dtype) of every 16-bit 2-D case of the golden file"""
    g = golden_io.load("wanda_unit")
    for name in sorted({k.rsplit("/", 1)[0] for k in g if k.endswith("/mask")}):
        keep, wn = g[f"{name}/mask"].bool(), g[f"{name}/Wn"]
        if keep.dim() != 2 or keep.shape[1] % 8 or wn.dtype not in (torch.float16, torch.bfloat16):
            continue
        yield name, keep.numpy(), wn.view(torch.int16).numpy().view(np.uint16)


def test_the_references_masks_pack_and_round_trip():
    seen = []
    for name, keep, bits in _reference_unstructured_prunes():
        values, meta, offs, rowptr = packbm.pack(bits, keep)
        w2, k2, bad = packbm.unpack(values, meta, offs, rowptr)
        assert bad == 0 and np.array_equal(k2, keep), name
        assert np.array_equal(w2, np.where(keep, bits, 0)) and np.array_equal(w2, bits), name     # the reference zeroed what it pruned
        assert np.array_equal(packbm.unpack_lane_local(values, meta, offs, rowptr), w2), name
        seen.append(name)
    # unstructured row-wise prunes at three ratios, and the n:m ones, which are masks like any other
    assert {"g2/bf16_r30", "g2/bf16_r50", "g2/fp16_r50", "g3/bf16_r25", "g3/fp16_r50", "g4/bf16_2_4_t5", "g4/fp16_4_8_vit"} <= set(seen), seen


def _torch_case(out_f=9, in_f=72, seed=3):
    w, keep = _random_case(out_f, in_f, seed)
    values, meta, offs, rowptr = packbm.pack(w, keep)
    return torch.from_numpy(meta), torch.from_numpy(offs), torch.from_numpy(rowptr), int(keep.sum())


def test_meta_bm_is_valid_accepts_what_pack_writes():
    from vlmc.packedbm import meta_bm_is_valid
    assert meta_bm_is_valid(*_torch_case())
    assert meta_bm_is_valid(*_torch_case(5, 8, 1)) and meta_bm_is_valid(*_torch_case(33, 40, 2))
    w = np.arange(1, 161, dtype=np.uint16).reshape(4, 40)
    _v, meta, offs, rowptr = packbm.pack(w, np.zeros((4, 40), dtype=bool))                       # nothing kept anywhere
    assert meta_bm_is_valid(torch.from_numpy(meta), torch.from_numpy(offs), torch.from_numpy(rowptr), 0)


def test_meta_bm_is_valid_rejects_wrong_offs_rowptr_and_nnz():
    from vlmc.packedbm import meta_bm_is_valid
    meta, offs, rowptr, nnz = _torch_case()
    bad = offs.clone()
    bad[4, 2] = int(bad[4, 2]) + 1                                             # a wrong offs entry
    assert not meta_bm_is_valid(meta, bad, rowptr, nnz)
    bad = rowptr.clone()
    bad[5] += 1                                                                # a wrong rowptr entry
    assert not meta_bm_is_valid(meta, offs, bad, nnz)
    assert not meta_bm_is_valid(meta, offs, rowptr, nnz + 1)                   # rowptr[N] != nnz
    bad = meta.clone()
    bad[0, 0] ^= 1                                                             # a bit more or less: every count after it moves
    assert not meta_bm_is_valid(bad, offs, rowptr, nnz)
    assert not meta_bm_is_valid(meta, offs[:, :2], rowptr, nnz) and not meta_bm_is_valid(meta, offs, rowptr[:-1], nnz)
    assert not meta_bm_is_valid(meta, offs.view(torch.int16), rowptr, nnz)


def test_mask_from_zeros_and_break_even():
    from vlmc.packedbm import is_mask_bm, mask_bm_from_zeros, packed_bm_bytes
    w = torch.tensor([[0.0, -0.0, 1.0, 0.0, -2.0, 0.0, 0.0, 3.0]])
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert mask_bm_from_zeros(w.to(dt)).tolist() == [[False, False, True, False, True, False, False, True]]
    with pytest.raises(ValueError):
        mask_bm_from_zeros(torch.zeros(8))
    assert packed_bm_bytes(4, 40, 55) == packbm.packed_bytes(4, 40, 55)
    out_f, in_f = 64, 256
    half = torch.zeros(out_f, in_f, dtype=torch.bool)
    half[:, ::2] = True
    assert is_mask_bm(half, half.shape) and packed_bm_bytes(out_f, in_f, int(half.sum())) < 2 * out_f * in_f
    dense = torch.ones(out_f, in_f, dtype=torch.bool)
    dense[:, ::16] = False                                                    # 15 / 16 kept: above break-even
    assert not is_mask_bm(dense, dense.shape)
    assert not is_mask_bm(half[:, :12], (out_f, 12)) and not is_mask_bm(half.to(torch.uint8), half.shape)
    assert not is_mask_bm(half, (out_f, in_f + 8))
