"""Runs a test module's function once per size-picked kernel variant, each in a fresh child process.

The `VLMC_*` switches that force a variant are read once per process by the library (`static const` in csrc/), so a variant cannot
be set from inside the test process: each one runs `module.function()` in its own Python with the variable in its environment,
one child at a time, and hands its result back through `torch.save`.  The parent compares the results (bit for bit across the
variants, and against a float64 or oracle reference)."""
import os
import subprocess
import sys

import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
PKG = os.path.join(ROOT, "vlm-compression_amd")

_CHILD = """
import sys
sys.path[:0] = [{tests!r}, {pkg!r}, {root!r}]
import importlib
import torch
fn = getattr(importlib.import_module(sys.argv[1]), sys.argv[2])
out = fn()
torch.cuda.synchronize()
torch.save(out, sys.argv[3])
"""


def run_variants(tmp_dir, module, function, variants, timeout=600):
    """`variants`: {label: {VLMC_NAME: value}} (an empty dict: the size rule's own pick).  Returns {label: what `function` returned}.
    Every variable named by any variant is removed from the other variants' environments, so that "default" means the rule."""
    names = {k for env in variants.values() for k in env}
    code = _CHILD.format(tests=TESTS, pkg=PKG, root=ROOT)
    results = {}
    for i, (label, extra) in enumerate(variants.items()):
        env = {k: v for k, v in os.environ.items() if k not in names}
        env.update(extra)
        out = os.path.join(str(tmp_dir), f"{module}.{function}.{i}.pt")
        r = subprocess.run([sys.executable, "-c", code, module, function, out], env=env, capture_output=True, text=True,
                           timeout=timeout)
        assert r.returncode == 0, f"{label} ({extra}): exit {r.returncode}\n{r.stderr[-3000:]}"
        results[label] = torch.load(out)
        os.remove(out)
    return results


def same_bits(a, b):
    """Bit equality of two tensors of one dtype (NaN payloads and -0.0 included)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    if a.dtype == torch.bool:
        return torch.equal(a, b)
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def assert_variants_agree(results, base="default"):
    """Every variant's outputs (nested dicts / lists / tuples of tensors) have the bits of `base`'s."""
    ref = results[base]

    def walk(a, b, path):
        if isinstance(a, dict):
            assert a.keys() == b.keys(), path
            for k in a:
                walk(a[k], b[k], f"{path}/{k}")
        elif isinstance(a, (list, tuple)):
            assert len(a) == len(b), path
            for i, (x, y) in enumerate(zip(a, b)):
                walk(x, y, f"{path}[{i}]")
        elif isinstance(a, torch.Tensor):
            assert same_bits(a, b), f"{path}: {int((a != b).sum()) if a.shape == b.shape else 'shape'} entries differ"
        else:
            assert a == b, path

    for label, got in results.items():
        if label != base:
            walk(ref, got, label)
