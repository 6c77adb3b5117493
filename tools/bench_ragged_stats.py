"""`vlmc_act_moments_lens` and `vlmc_hessian_accum_rows` against their unpadded siblings on the compacted input (GPU only): microseconds
per launch, HIP-event medians after two warm-up launches.  Prints a markdown table (profiles/ragged_dsnot_sparsegpt.md).

    python tools/bench_ragged_stats.py [--reps 20]

Shapes: the padded group of the ragged InstructBLIP-Vicuna-7B calibration set (128 samples, 32 query tokens + 8..128 prompt + 4..16 answer
tokens padded to 176, 4096 and 11008 wide, fp16) and those of tests/test_ragged_stats_gpu.py.  The sibling of the moments kernel is
`vlmc_act_moments` once PER LENGTH GROUP of the compacted samples (what the walk of equal shapes launches); the sibling of the Hessian is
`vlmc_hessian_accum` on the rows gathered into a contiguous matrix beforehand (the gather's own `index_select` is timed apart)."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vlm-compression_amd"))
import torch

from vlmc import _lib, ops, synthetic
from vlmc.ops import _dtype_code, _stream
from lavis.compression.pruners import replay_padding as rp

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
dev = "cuda:0"
lib = _lib.load()


def timeit(fn, reps=args.reps, warm=2):
    ts = []
    for i in range(reps + warm):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def vicuna_lengths(n=128):
    return [32 + synthetic.RAGGED_TEXT[j % len(synthetic.RAGGED_TEXT)] + synthetic.RAGGED_OUT[(j // 3) % len(synthetic.RAGGED_OUT)] for j in range(n)]


CASES = [("Vicuna set", vicuna_lengths(), 4096, torch.float16), ("Vicuna set", vicuna_lengths(), 11008, torch.float16),
         ("test 6", [44, 176, 60, 97, 176, 52], 1408, torch.float16), ("test 6", [300] * 7 + [173], 5120, torch.bfloat16),
         ("test 6", [300] * 7 + [173], 2048, torch.float32), ("test 5", [1, 53, 17, 32, 16, 33], 4096, torch.bfloat16)]

print("| kernel | case | shape | us per launch | sibling on the compacted input, us | note |")
print("|---|---|---|---|---|---|")
for tag, lens, in_f, dtype in CASES:
    tp, n = max(lens), len(lens)
    g = torch.Generator(device=dev).manual_seed(in_f)
    x = (torch.randn(n, tp, in_f, generator=g, device=dev) * 0.5).to(dtype)
    ct = torch.tensor(lens, dtype=torch.int32, device=dev)
    row_map, n_rows = rp.row_map(lens, tp, dev)
    compact = x.reshape(-1, in_f).index_select(0, row_map[:n_rows])
    shape = f"[{n}, {tp}, {in_f}] {str(dtype)[6:]}, {n_rows} real rows of {n * tp}"
    # ---- moments
    out = torch.empty((3, n, in_f), device=dev)
    us = timeit(lambda: _lib.check(lib.vlmc_act_moments_lens(x.data_ptr(), _dtype_code(x), n, tp, in_f, in_f, tp * in_f, ct.data_ptr(),
                                                             out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _stream())))
    groups, off = {}, 0
    for t in lens:                                                          # the compacted samples of one length, stacked: one launch each
        groups.setdefault(t, []).append(compact[off:off + t])
        off += t
    stacks = [torch.stack(v) for v in groups.values()]
    outs = [torch.empty((3, s.shape[0], in_f), device=dev) for s in stacks]

    def per_length():
        for s, o in zip(stacks, outs):
            _lib.check(lib.vlmc_act_moments(s.data_ptr(), _dtype_code(s), s.shape[0], s.shape[1], in_f, in_f, s.shape[1] * in_f, o[0].data_ptr(),
                                            o[1].data_ptr(), o[2].data_ptr(), _stream()))
    us_sib = timeit(per_length)
    nbytes = n_rows * in_f * x.element_size()
    print(f"| `vlmc_act_moments_lens` | {tag} | {shape} | {us:.1f} | {us_sib:.1f} ({len(stacks)} launches of `vlmc_act_moments`, one per length) | "
          f"{nbytes / us / 1e3:.0f} GB/s of the real rows' bytes |", flush=True)
    # ---- Hessian
    H = torch.zeros(in_f, in_f, device=dev)
    code = _dtype_code(x)
    need = lib.vlmc_hessian_workspace(code, n_rows, in_f)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    one, zero = ctypes.c_float(2.0 / n), ctypes.c_float(0.0)
    us = timeit(lambda: _lib.check(lib.vlmc_hessian_accum_rows(x.data_ptr(), code, n * tp, in_f, in_f, row_map.data_ptr(), n_rows, H.data_ptr(), in_f,
                                                               zero, one, ws.data_ptr(), need, _stream())))
    us_sib = timeit(lambda: _lib.check(lib.vlmc_hessian_accum(compact.data_ptr(), code, n_rows, in_f, in_f, H.data_ptr(), in_f, zero, one,
                                                              ws.data_ptr(), need, _stream())))
    need_all = lib.vlmc_hessian_workspace(code, n * tp, in_f)
    ws_all = torch.empty(max(need_all, 16), dtype=torch.uint8, device=dev)
    us_all = timeit(lambda: _lib.check(lib.vlmc_hessian_accum(x.data_ptr(), code, n * tp, in_f, in_f, H.data_ptr(), in_f, zero, one, ws_all.data_ptr(),
                                                              need_all, _stream())))
    us_gather = timeit(lambda: x.reshape(-1, in_f).index_select(0, row_map[:n_rows]))
    print(f"| `vlmc_hessian_accum_rows` | {tag} | {shape} | {us:.1f} | {us_sib:.1f} (+ {us_gather:.1f} for the `index_select` that compacts) | "
          f"every padded row multiplied (`vlmc_hessian_accum` on all {n * tp}): {us_all:.1f} us; {2 * n_rows * in_f * in_f / us / 1e6:.0f} TFLOP/s of 2 T in^2 |",
          flush=True)
    del x, compact, H, ws, ws_all, stacks, outs
