"""Whole `blipt5_dsnot_pruner.prune()` with initial_method "wanda" against "sparsegpt" (unstructured 0.5 and 2:4) on the bench's
synthetic InstructBLIP-FlanT5-XL (128 samples) and on the InstructBLIP-Vicuna-7B shapes.  Prints the warm wall-clock of each
(third of three runs), then one instrumented run per configuration split into Hessian accumulation, factorization (the divisor)
and select + refine + apply -- every phase bracketed by device synchronisations, so the split's sum exceeds the plain run.

    python tools/bench_dsnot_init.py [--only flant5|vicuna] [--runs 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vlm-compression_amd"))
import torch  # noqa: E402
from vlmc import dsnot, sparsegpt, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")


class Phases:
    """Synchronised host timers around the three steps of the sparsegpt route (and prune_linear on every route)."""

    def __init__(self):
        self.t = {"hessian": 0.0, "factor": 0.0, "select+refine": 0.0}
        self.real = (sparsegpt.SparseGPT.add_batch, sparsegpt.SparseGPT._fold, dsnot.sparsegpt_divisors, dsnot.prune_linear)

    def wrap(self, key, fn):
        def timed(*a, **k):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize(dev)
            self.t[key] += time.perf_counter() - t0
            return out
        return timed

    def __enter__(self):
        add, fold, div, prune = self.real
        sparsegpt.SparseGPT.add_batch = self.wrap("hessian", add)
        sparsegpt.SparseGPT._fold = self.wrap("hessian", fold)
        dsnot.sparsegpt_divisors = self.wrap("factor", div)
        dsnot.prune_linear = self.wrap("select+refine", prune)
        return self

    def __exit__(self, *exc):
        sparsegpt.SparseGPT.add_batch, sparsegpt.SparseGPT._fold, dsnot.sparsegpt_divisors, dsnot.prune_linear = self.real


workloads = [("flant5", {}), ("vicuna", {"t5_model_prefix": "llm_model"})]
print("| workload | initial_method | sparsity | warm prune s (runs) | hessian s | factor s | select+refine s | pruned |")
print("|---|---|---|---|---|---|---|---|", flush=True)
for wl, wkw in workloads:
    if args.only and args.only != wl:
        continue
    model = None
    for init in ("wanda", "sparsegpt"):
        for sp, skw in (("u0.5", {}), ("2:4", {"prune_n": 2, "prune_m": 4})):
            ts = []
            for _ in range(args.runs):
                dt, model, info = synthetic.time_prune(dev, "blipt5_dsnot_pruner", model=model, initial_method=init, **wkw, **skw)
                ts.append(dt)
            with Phases() as ph:
                synthetic.time_prune(dev, "blipt5_dsnot_pruner", model=model, initial_method=init, **wkw, **skw)
            print(f"| {wl} | {init} | {sp} | {ts[-1]:.3f} ({', '.join(f'{t:.3f}' for t in ts)}) | {ph.t['hessian']:.3f} | "
                  f"{ph.t['factor']:.3f} | {ph.t['select+refine']:.3f} | {info['pruned_fraction']:.4f} |", flush=True)
    del model
    torch.cuda.empty_cache()
