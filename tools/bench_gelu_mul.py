"""T5's gated product at the headline prune's encoder shape: `vlmc_gelu` + torch's `mul` (two launches, five tensor passes over every
row) against `vlmc_gelu_mul` (one launch, three passes, over the real rows only when given the padded group's row map).

    python tools/bench_gelu_mul.py [--samples 128] [--tokens 160] [--cols 5120] [--iters 200]

Prints one line per variant: microseconds per call (device events around `iters` back-to-back calls, after a warm-up), the bytes the
variant has to move and the rate that makes, as a share of the 8 TB/s HBM peak."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vlm-compression_amd"))
from vlmc import ops  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=160)
    ap.add_argument("--cols", type=int, default=5120)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    n, P, cols = a.samples, a.tokens, a.cols
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(n, P, cols, generator=g, device=dev).bfloat16()
    y = torch.randn(n, P, cols, generator=g, device=dev).bfloat16()
    lengths = np.random.default_rng(0).integers(8, P + 1, size=n)          # ragged prompts: about half of the rows are padding
    tok = np.arange(P)[None, :]
    real = tok < lengths[:, None]
    flat = np.arange(n)[:, None] * P + tok
    rowmap = torch.from_numpy(np.concatenate([flat[real], flat[~real]]).astype(np.int32)).to(dev)
    n_real = int(real.sum())
    pad = torch.from_numpy(~real).to(dev)
    x[pad], y[pad] = 0, 0
    want = ops.gelu(x) * y
    assert torch.equal(ops.gelu_mul(x, y).view(torch.int16), want.view(torch.int16))
    assert torch.equal(ops.gelu_mul(x, y, "none", rowmap, n_real).view(torch.int16), want.view(torch.int16))
    rows = n * P
    variants = [("vlmc_gelu + torch mul, every row", lambda: ops.gelu(x) * y, 5 * rows * cols * 2),
                ("vlmc_gelu alone, every row", lambda: ops.gelu(x), 2 * rows * cols * 2),
                ("vlmc_gelu_mul, every row", lambda: ops.gelu_mul(x, y), 3 * rows * cols * 2),
                (f"vlmc_gelu_mul, row map ({n_real} of {rows} rows real)", lambda: ops.gelu_mul(x, y, "none", rowmap, n_real),
                 (2 * n_real + rows) * cols * 2)]
    print(f"[{n} x {P}, {cols}] bf16, {torch.cuda.get_device_name(0)}")
    for r in range(a.repeats):
        for name, fn, nbytes in variants:
            us = timed(fn, a.iters)
            print(f"run {r}: {name}: {us:8.1f} us  {nbytes / 1e6:7.1f} MB  {nbytes / us / 1e6:6.2f} TB/s  {100 * nbytes / (us * 1e-6) / HBM_PEAK:5.1f} % of peak")


if __name__ == "__main__":
    main()
