"""Whole `blipt5_sparsegpt_pruner.prune()` on the synthetic InstructBLIP-Vicuna-7B (`vlmc.synthetic.InstructBlipVicuna`: ViT-g
39 blocks + 32 LLaMA layers 4096 / 11008, fp16, 128 calibration samples; `t5_model_prefix="llm_model"`) at unstructured 50 %
and at 2:4.  Prints the warm wall-clock of each (the last of `--runs`), then one more run in which every `factorize_many`
(the inverse-factor chains of one block) is bracketed by device synchronisations, split by Hessian width -- 1408 / 6144
(ViT), 4096 / 11008 (LLaMA) -- and last one synchronised `inverse_upper_factor` of an 11008-wide Hessian alone.

    python tools/bench_sparsegpt_vicuna.py [--only u50|2:4] [--runs 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vlm-compression_amd"))
import torch  # noqa: E402
from vlmc import sparsegpt, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")


class FactorTimer:
    """Synchronised host time of every factorize_many call, summed per Hessian width of the block's largest input."""

    def __init__(self):
        self.t, self.calls, self.real = {}, {}, sparsegpt.factorize_many

    def __enter__(self):
        def timed(items, *a, **k):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = self.real(items, *a, **k)
            torch.cuda.synchronize(dev)
            widths = "/".join(str(w) for w in sorted({H.shape[0] for H, _ in items}))
            self.t[widths] = self.t.get(widths, 0.0) + time.perf_counter() - t0
            self.calls[widths] = self.calls.get(widths, 0) + 1
            return out
        sparsegpt.factorize_many = timed
        return self

    def __exit__(self, *exc):
        sparsegpt.factorize_many = self.real


print("| sparsity | warm prune s (runs) | synchronised run s | factorize_many s by block widths (blocks) | pruned |")
print("|---|---|---|---|---|", flush=True)
model = None
for sp, skw in (("u50", {}), ("2:4", {"prune_n": 2, "prune_m": 4})):
    if args.only and args.only != sp:
        continue
    ts = []
    for _ in range(args.runs):
        dt, model, info = synthetic.time_prune(dev, "blipt5_sparsegpt_pruner", model=model, t5_model_prefix="llm_model", **skw)
        ts.append(dt)
    with FactorTimer() as ft:
        dt_sync, model, _ = synthetic.time_prune(dev, "blipt5_sparsegpt_pruner", model=model, t5_model_prefix="llm_model", **skw)
    split = ", ".join(f"{w}: {ft.t[w]:.3f} ({ft.calls[w]})" for w in sorted(ft.t))
    print(f"| {sp} | {ts[-1]:.3f} ({', '.join(f'{t:.3f}' for t in ts)}) | {dt_sync:.3f} | {split} | {info['pruned_fraction']:.4f} |",
          flush=True)
del model
torch.cuda.empty_cache()

# one 11008-wide factorization alone (the down_proj Hessian), with the whole chip: H = (2/N) X^T X + 0.01 mean(diag) I
n = 11008
g = torch.Generator(device=dev).manual_seed(0)
X = (torch.randn(12288, n, generator=g, device=dev) * 0.5).half()
H = (X.float().t() @ X.float()) * (2.0 / X.shape[0])
H.diagonal().add_(0.01 * float(H.diagonal().mean()))
del X
for rep in range(4):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    U, info = sparsegpt.inverse_upper_factor(H)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
print(f"\ninverse_upper_factor, n = {n} (persistent: {sparsegpt.persistent_factor_usable(n)}): {dt * 1e3:.1f} ms (last of 4), "
      f"info {int(info.item())}", flush=True)
