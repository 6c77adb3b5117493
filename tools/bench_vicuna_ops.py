"""Whole `blipt5_wanda_pruner` / `blipt5_dsnot_pruner` / `blipt5_sparsegpt_pruner` prunes of the REFERENCE-OP InstructBLIP-Vicuna-7B stand-in
(`vlmc.synthetic_llama.InstructBlipVicunaOps`: ViT-g + 32 layers 4096 / 11008 written as modeling_llama.py writes them, fp16; 128
ragged samples from `calibration_batches(ragged=True, vocab=32000)`: 32 query tokens + 8..128 prompt + 4..16 answer tokens, at most
176 keys), three legs in ONE command:

    (a) the reference's loop: this build with VLMC_BATCH_REPLAY=1 VLMC_TOWER_BATCH=0 (one sample per block forward)
    (b) the PARENT COMMIT's routes: a checkout of the parent, built, with vlmc/synthetic_llama.py copied in (`--parent ROOT`); it runs
        the stand-in as it is (the chain is realized at the clamp, ragged samples are grouped by equal shape)
    (c) this build

Two builds of the library cannot live in one process, so each tree gets child processes of this script (`--child`): the parent's
runs first (b1), then this build's with (a) and (c) ALTERNATED prune by prune, then the parent's again (b2): the difference between
b1 and b2 is the spread the comparison of (c) with (b) is read against.  Every prune is warmed up once per leg and ends in a device
synchronise (`synthetic.time_prune`).  Masks (the zero pattern of every pruned linear, packed) are compared bit for bit: (a) against
(c) in the child, (b) against (c) through a file under `--scratch`; the number of differing bits is printed.

    python tools/bench_vicuna_ops.py --parent /path/to/parent_tree [--steps 2] [--samples 128] [--methods wanda,dsnot,sparsegpt] [--equal-lengths]

`--skip-loop`: without leg (a), so that (c) has its process to itself as (b) has (a whole SparseGPT prune sample by sample leaves the
allocator in another state than it found it: measured, profiles/ragged_dsnot_sparsegpt.md).  `--equal-lengths`: the same legs on text of ONE length (32 prompt + 16 answer tokens), where nothing is padded: what a change to the ragged
routes must leave as it was.

Kernel statistics come from a separate run under a tracer (`--child this --legs c --steps 1` after `rocprofv3 --kernel-trace --stats --`):
tracing and timing never share a run."""
import argparse
import json
import os
import subprocess
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default="", help="root of a built checkout of the parent commit with vlmc/synthetic_llama.py copied in")
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--samples", type=int, default=128)
ap.add_argument("--methods", default="wanda,dsnot")
ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), f"vlmc_vicuna_ops_{os.getpid()}"),
                help="where the parent's packed masks (~1 GB per method) wait for the comparison; removed at the end")
ap.add_argument("--child", default="", help="internal: `this` or `parent`")
ap.add_argument("--tree", default=ROOT)
ap.add_argument("--legs", default="")
ap.add_argument("--tag", default="")
ap.add_argument("--child-timeout", type=int, default=900)
ap.add_argument("--skip-loop", action="store_true", help="leave leg (a) out: (c) then runs alone in its process, as (b) does in its own")
ap.add_argument("--equal-lengths", action="store_true", help="calibration text of one length instead of the ragged set")
args = ap.parse_args()
METHODS = [m for m in args.methods.split(",") if m]

LEG_ENV = {"a": {"VLMC_BATCH_REPLAY": "1", "VLMC_TOWER_BATCH": "0"}, "b": {}, "c": {}}


def child():
    sys.path.insert(0, os.path.join(args.tree, "vlm-compression_amd"))
    import torch
    from vlmc import forward, synthetic, synthetic_llama
    dev = torch.device("cuda:0")
    legs = args.legs.split(",")
    torch.manual_seed(0)                                                   # (the linears' biases keep their default initialisation: the same in every process)
    with dev:                                                              # (7 B parameters: initialised where they will live)
        model = synthetic_llama.InstructBlipVicunaOps().eval()
    batches = synthetic.calibration_batches(args.samples, dev, vocab=32000, ragged=not args.equal_lengths)
    keys = [32 + b["text_input"].shape[1] + b["text_output"].shape[1] for b in batches]
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)

    def packed_masks():
        out = []
        for name, mod in model.named_modules():
            if isinstance(mod, torch.nn.Linear) and (".blocks." in name or ".layers." in name):
                z = (mod.weight.data == 0).view(-1, 8).to(torch.uint8)
                out.append((z * weights).sum(1, dtype=torch.uint8))
        return torch.cat(out)

    def popcount(x):
        return int(sum(int(((x >> s) & 1).sum()) for s in range(8)))

    def one(leg, method):
        old = {k: os.environ.get(k) for k in LEG_ENV[leg]}
        os.environ.update(LEG_ENV[leg])
        try:
            before = dict(forward.stats)
            dt, _, info = synthetic.time_prune(dev, f"blipt5_{method}_pruner", n_samples=args.samples, model=model, batches=batches,
                                               t5_model_prefix="llm_model")
            stats = {k: forward.stats[k] - before.get(k, 0) for k in forward.stats if forward.stats[k] != before.get(k, 0)}
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        return dt, info, stats

    result = {"tag": args.tag, "tree": args.tree, "keys_max": max(keys), "keys_mean": sum(keys) / len(keys), "legs": {}}
    for method in METHODS:
        masks = {}
        for leg in legs:
            one(leg, method)                                               # warm-up (kernel loading, signature checks, sibling groups)
        times = {leg: [] for leg in legs}
        for _ in range(args.steps):
            for leg in legs:                                               # alternated
                dt, info, stats = one(leg, method)
                times[leg].append(dt)
                print(f"# {args.tag} {method} leg {leg}: {dt:.3f} s", file=sys.stderr, flush=True)
                if leg not in masks:
                    masks[leg] = (packed_masks(), info, stats)
        for leg in legs:
            m, info, stats = masks[leg]
            result["legs"][f"{leg}/{method}"] = {"seconds": times[leg], "pruned_fraction": info["pruned_fraction"], "linears": info["linears"],
                                                 "mask_bits": int(m.numel()) * 8, "forward_stats": stats}
        if "a" in masks and "c" in masks:
            result[f"diff_a_c/{method}"] = popcount(masks["a"][0] ^ masks["c"][0])
        os.makedirs(args.scratch, exist_ok=True)
        path = os.path.join(args.scratch, f"masks_b_{method}.pt")
        if args.child == "parent" and args.tag == "b1":
            torch.save(masks["b"][0].cpu(), path)
        elif args.child == "this" and "c" in masks and os.path.exists(path):
            other = torch.load(path).to(dev)
            result[f"diff_b_c/{method}"] = popcount(other ^ masks["c"][0]) if other.shape == masks["c"][0].shape else -1
    print("RESULT " + json.dumps(result), flush=True)


def run_child(which, tree, legs, tag):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--tree", tree, "--legs", legs, "--tag", tag, "--steps", str(args.steps),
           "--samples", str(args.samples), "--methods", args.methods, "--scratch", args.scratch] + (["--equal-lengths"] if args.equal_lengths else [])
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)       # (progress goes to stderr as it happens)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        raise SystemExit(f"child {tag} ended with status {p.returncode}: nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    print(f"# child {tag} ({legs}) took {time.perf_counter() - t0:.0f} s", flush=True)
    return json.loads(line[7:])


def main():
    if not args.parent or not os.path.exists(os.path.join(args.parent, "vlm-compression_amd", "vlmc", "synthetic_llama.py")):
        raise SystemExit("--parent: a built checkout of the parent commit with vlmc/synthetic_llama.py copied in")
    b1 = run_child("parent", args.parent, "b", "b1")
    ac = run_child("this", ROOT, "c" if args.skip_loop else "a,c", "ac")
    b2 = run_child("parent", args.parent, "b", "b2")
    shutil.rmtree(args.scratch, ignore_errors=True)
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"\n{args.samples} {'equal-length' if args.equal_lengths else 'ragged'} samples, keys per sample: mean {ac['keys_mean']:.0f}, max {ac['keys_max']}; {args.steps} timed prunes per leg "
          f"after one warm-up\n")
    print("| method | leg | seconds per prune (each run) | median |")
    print("|---|---|---|---|")
    summary = {}
    for method in METHODS:
        rows = [("(a) per-sample loop, this build", ac["legs"].get(f"a/{method}", {"seconds": [float("nan")]})["seconds"]),
                ("(b) parent commit, first process", b1["legs"][f"b/{method}"]["seconds"]),
                ("(b) parent commit, second process", b2["legs"][f"b/{method}"]["seconds"]),
                ("(c) this build", ac["legs"][f"c/{method}"]["seconds"])]
        for leg, secs in rows:
            print(f"| {method} | {leg} | {', '.join(f'{t:.3f}' for t in secs)} | {med(secs):.3f} |")
        bs = b1["legs"][f"b/{method}"]["seconds"] + b2["legs"][f"b/{method}"]["seconds"]
        summary[method] = {"a": med(rows[0][1]), "b": med(bs), "b_spread": max(bs) - min(bs), "c": med(rows[3][1]),
                           "diff_a_c": ac.get(f"diff_a_c/{method}"), "diff_b_c": ac.get(f"diff_b_c/{method}"),
                           "mask_bits": ac["legs"][f"c/{method}"]["mask_bits"]}
    print()
    for method, s in summary.items():
        print(f"{method}: (c) {s['c']:.3f} s against (b) {s['b']:.3f} s (spread of (b) over both processes {s['b_spread']:.3f} s), (a) {s['a']:.3f} s; "
              f"mask bits differing of {s['mask_bits']}: (a) vs (c) {s['diff_a_c']}, (b) vs (c) {s['diff_b_c']}"
              + (" -- informational: SparseGPT's Hessian sums in another order per grouping, by design" if method == "sparsegpt" else ""))
    print("\nforward.stats per prune, (c):", json.dumps({m: ac["legs"][f"c/{m}"]["forward_stats"] for m in METHODS}))
    print("forward.stats per prune, (b):", json.dumps({m: b1["legs"][f"b/{m}"]["forward_stats"] for m in METHODS}))
    print("SUMMARY " + json.dumps(summary))


if __name__ == "__main__":
    child() if args.child else main()
