"""TEST INFRASTRUCTURE: the packed bitmap ("bm") layout of include/vlmc.h (vlmc_pack_bm_rows / vlmc_pack_bm / vlmc_unpack_bm), restated
in numpy.

The reference has no packed format, so there is no reference output to pin this against: the layout is this build's own, defined
in include/vlmc.h, and what the tests hold the kernels to is (a) this restatement, (b) the round trip unpack(pack(W, mask)) ==
W * mask with the mask recovered, (c) the unstructured masks the reference's rule produced (tests/golden/wanda_unit.npz) being
packable, (d) the lane-local address formula of the forward kernel (`unpack_lane_local`) reproducing the sequential unpack."""
import numpy as np

TAIL = 16


def pack(w_bits: np.ndarray, keep: np.ndarray):
    """w_bits [out, in] uint16 (the weights' bit patterns), keep [out, in] bool ->
    (values [nnz + 16] uint16, meta [out, in / 8] uint8, offs [out, ceil(in / 32)] uint16, rowptr [out + 1] int64)"""
    out_f, in_f = w_bits.shape
    assert in_f % 8 == 0 and in_f <= 65536
    steps = (in_f + 31) // 32
    values, meta = [], np.zeros((out_f, in_f // 8), dtype=np.uint8)
    offs, rowptr = np.zeros((out_f, steps), dtype=np.uint16), np.zeros(out_f + 1, dtype=np.int64)
    for r in range(out_f):
        rowptr[r] = len(values)
        for col in range(in_f):
            if col % 32 == 0:
                offs[r, col // 32] = len(values) - rowptr[r]
            if keep[r, col]:
                meta[r, col // 8] |= 1 << (col % 8)
                values.append(w_bits[r, col])
    rowptr[out_f] = len(values)
    return np.array(values + [0] * TAIL, dtype=np.uint16), meta, offs, rowptr


def unpack(values: np.ndarray, meta: np.ndarray, offs: np.ndarray, rowptr: np.ndarray):
    """Sequential: the values are taken in order as the bitmap is walked.  -> (w_bits [out, in] uint16, keep [out, in] bool, the number
    of steps whose offs and of rows whose rowptr disagree with the running popcount, rowptr[0] != 0 and rowptr[out] != nnz included)"""
    out_f, chunks = meta.shape
    in_f, nnz = 8 * chunks, values.size - TAIL
    w, keep = np.zeros((out_f, in_f), dtype=np.uint16), np.zeros((out_f, in_f), dtype=bool)
    nxt, bad = 0, int(rowptr[0] != 0) + int(rowptr[out_f] != nnz)
    for r in range(out_f):
        start = nxt
        for col in range(in_f):
            if col % 32 == 0:
                bad += int(offs[r, col // 32]) != nxt - start
            if (int(meta[r, col // 8]) >> (col % 8)) & 1:
                keep[r, col] = True
                if nxt < values.size:
                    w[r, col] = values[nxt]
                nxt += 1
        bad += int(rowptr[r + 1]) - int(rowptr[r]) != nxt - start
    return w, keep, bad


def unpack_lane_local(values: np.ndarray, meta: np.ndarray, offs: np.ndarray, rowptr: np.ndarray):
    """Chunk by chunk, each on its own, as a lane of the forward kernel does it: the chunk's first value is at
    min(rowptr[n] + offs[n][s] + popcount(meta[n][4s .. 4s+q-1]), nnz), nothing else is looked at.  -> w_bits [out, in] uint16"""
    out_f, chunks = meta.shape
    nnz = values.size - TAIL
    w = np.zeros((out_f, 8 * chunks), dtype=np.uint16)
    for r in range(out_f):
        for c in range(chunks):
            s, q = divmod(c, 4)
            before = sum(bin(int(meta[r, 4 * s + p])).count("1") for p in range(q))
            i = max(min(int(rowptr[r]) + int(offs[r, s]) + before, nnz), 0)
            for j in range(8):
                if (int(meta[r, c]) >> j) & 1:
                    w[r, 8 * c + j] = values[i]
                    i += 1
    return w


def packed_bytes(out_f: int, in_f: int, nnz: int) -> int:
    return (nnz + TAIL) * 2 + out_f * in_f // 8 + 2 * out_f * ((in_f + 31) // 32) + 8 * (out_f + 1)
