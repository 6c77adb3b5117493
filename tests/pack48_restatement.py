"""TEST INFRASTRUCTURE: the packed 4:8 layout of include/vlmc.h (vlmc_pack_48 / vlmc_unpack_48), restated in numpy.

The reference has no packed format, so there is no reference output to pin this against: the layout is this build's own, defined
in include/vlmc.h, and what the tests hold the kernels to is (a) this restatement, (b) the round trip unpack(pack(W, mask)) ==
W * mask with the mask recovered, (c) the masks the reference's n:m rule produced at 4:8 (tests/golden/wanda_unit.npz) being
packable."""
import numpy as np


def pack(w_bits: np.ndarray, keep: np.ndarray):
    """w_bits [out, in] uint16 (the weights' bit patterns), keep [out, in] bool -> (values [out, in/2] uint16, meta [out, in/8] uint8,
    number of groups of eight that do not keep exactly four)"""
    out_f, in_f = w_bits.shape
    assert in_f % 8 == 0
    g = keep.reshape(out_f, in_f // 8, 8)
    bad = int((g.sum(-1) != 4).sum())
    values = np.zeros((out_f, in_f // 2), dtype=np.uint16)
    meta = np.zeros((out_f, in_f // 8), dtype=np.uint8)
    wg = w_bits.reshape(out_f, in_f // 8, 8)
    for r in range(out_f):
        for c in range(in_f // 8):
            idx = [j for j in range(8) if g[r, c, j]]
            meta[r, c] = sum(1 << j for j in idx)
            for s, j in enumerate(idx[:4]):
                values[r, 4 * c + s] = wg[r, c, j]
    return values, meta, bad


def unpack(values: np.ndarray, meta: np.ndarray):
    """-> (w_bits [out, in] uint16, keep [out, in] bool, number of metadata bytes whose popcount is not 4)"""
    out_f, half = values.shape
    in_f = half * 2
    w = np.zeros((out_f, in_f), dtype=np.uint16)
    keep = np.zeros((out_f, in_f), dtype=bool)
    bad = 0
    for r in range(out_f):
        for c in range(in_f // 8):
            idx = [j for j in range(8) if (int(meta[r, c]) >> j) & 1]
            bad += len(idx) != 4
            for s, j in enumerate(idx):
                keep[r, 8 * c + j] = True
                if s < 4:
                    w[r, 8 * c + j] = values[r, 4 * c + s]
    return w, keep, bad
