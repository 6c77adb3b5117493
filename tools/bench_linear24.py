"""The packed 2:4 linear (vlmc_linear_fwd_24), with `--format 48` the packed 4:8 linear (vlmc_linear_fwd_48), or with `--format bm` the
bitmap-packed linear of an UNSTRUCTURED prune (vlmc_linear_fwd_bm; `--density` of every row kept, 0.5 by default) against the dense
kernel (vlmc_linear_fwd on the unpacked weight) at the LLM shapes of Vicuna-7B and FlanT5-XL, fp16, COLD weights: every timed call
takes the next of a pool of weight copies, and a round over the pool
holds more than twice the 256 MiB Infinity Cache for the packed set and the dense set alike (one packed Vicuna layer is 228 MB
and would otherwise stay cached while its dense form does not).

Two clocks, both on the device:
  kernel   the kernel's own begin / end timestamps (vlmc_set_launch_events), summed over a round -- single-kernel routes only
  graph    a round of calls captured into one HIP graph and replayed between two events: what a stream of such calls costs, kernel
           gaps included; this is the only clock that sees the two kernels of the unpack route (unpack into scratch + dense)
Every row is measured `--repeats` times with the routes alternating; the table prints the median and the spread (max - min).

    python tools/bench_linear24.py [--format 24|48|bm] [--density 0.5] [--only v7b] [--rows 1,8,16] [--repeats 3] [--out profiles/linear24.md]

`--tiled` (every format; `--format bm` with `--density`): the PREFILL sizes instead -- for every shape above plus the four ViT-g linears and every row count of the
ladder 65 .. 4096, on the graph clock, alternating: (a) the unpack route (unpack into scratch + dense kernel: what runs above
`vlmc_linear_fwd_24_tiled_max_rows()` / `vlmc_linear_fwd_bm_tiled_max_rows()`), (b) the tiled kernel that takes the weight packed
(vlmc_linear_fwd_24_tiled / _48_tiled / _bm_tiled), (c) the
dense kernel on an unpacked weight that already exists (the floor, for orientation).  (a) and (b) are compared bit for bit before
anything is timed.  The last lines give, per row count, whether (b) beats (a) by more than the larger spread on EVERY shape, and the
largest ladder value up to which it does: the rule VLMC_LINEAR_NM_TILED_MAX_ROWS (profiles/linear_nm_tiled.md) and
VLMC_LINEARBM_TILED_MAX_ROWS (profiles/linearbm_tiled.md) are set by.
    python tools/bench_linear24.py --tiled --format 24 --out <file>;  python tools/bench_linear24.py --tiled --format 48 --out <file>
    python tools/bench_linear24.py --tiled --format bm [--density 0.5] --out <file>
(`--format 48 --rows 1,2,4,8,16,32,48,64,128 --out <file>` gives the table of profiles/linear48.md; `--format bm --out <file>` that of
profiles/linearbm.md, measured on a build whose VLMC_LINEARBM_MAX_ROWS is 64 so that the packed kernel is timed at every candidate limit)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vlm-compression_amd"), ROOT]
import torch  # noqa: E402

from vlmc import _lib, ops  # noqa: E402

SHAPES = {"v7b.qkvo": (4096, 4096), "v7b.gate_up": (11008, 4096), "v7b.down": (4096, 11008), "t5.qkvo": (2048, 2048), "t5.wi": (5120, 2048),
          "t5.wo": (2048, 5120)}
ROWS = (1, 8, 16, 32, 64, 128, 512, 4096)
VIT_SHAPES = {"vit.qkv": (4224, 1408), "vit.proj": (1408, 1408), "vit.fc1": (6144, 1408), "vit.fc2": (1408, 6144)}      # ViT-g, --tiled
LADDER = (65, 128, 257, 512, 1024, 2048, 4096)
CACHE = 256 << 20
DEV = "cuda:0"


_hipev = None


def kernel_us(call, pool):
    """sum of the kernels' own durations over one round, per call"""
    global _hipev
    if _hipev is None:
        from bench import HipEvents                    # HIP events of the loaded runtime, created through ctypes
        _hipev = HipEvents()
    arm = _lib.load().vlmc_set_launch_events
    evs = [(_hipev.new(), _hipev.new()) for _ in range(pool)]
    for i, (a, b) in enumerate(evs):
        arm(a, b)
        call(i)
    torch.cuda.synchronize()
    total = sum(_hipev.elapsed_ms(a, b) for a, b in evs)
    for a, b in evs:
        _hipev.free(a, b)
    return total / pool * 1e3


def make_graph(call, pool):
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(pool):
            call(i)                                    # warm: code objects, the scratch weight
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        for i in range(pool):
            call(i)
    return g


def graph_us(g, pool):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / pool * 1e3


def med_spread(v):
    return statistics.median(v), max(v) - min(v)


def tiled_main(args):
    """--tiled: the unpack route, the tiled packed kernel and the dense kernel at the prefill row counts"""
    n_keep, n_of = (2, 4) if args.format == "24" else (4, 8)
    pack, packed_fwd = getattr(ops, "pack_" + args.format), getattr(ops, "linear_fwd_" + args.format)
    rows = [int(r) for r in args.rows.split(",")] if args.rows else list(LADDER)
    what = f"unstructured, {args.density:g} of every row kept" if args.format == "bm" else f"{n_keep}:{n_of}"
    lines = [f"format {what} (`vlmc_linear_fwd_{args.format}_tiled`); fp16; cold weights; graph clock, us per call; median of {args.repeats} "
             "(spread = max - min); tiled wins = its median is below the unpack route's by more than the larger of the two spreads",
             "",
             "| shape (N x K) | M | (a) unpack route us (spread) | (b) tiled us (spread) | (c) dense us (spread) | (b) / (a) | (b) / (c) | tiled wins |",
             "|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    wins = {M: [] for M in rows}
    for name, (N, K) in {**SHAPES, **VIT_SHAPES}.items():
        if args.only and args.only not in name:
            continue
        g = torch.Generator(device=DEV).manual_seed(0)
        W = (torch.randn(N, K, device=DEV, generator=g) * 0.02).half()
        sq = torch.rand(K, device=DEV, generator=g) + 0.5
        if args.format == "bm":
            keep, _ = ops.wanda_select(W, sq, "row", k=K - int(round(K * args.density)))
        else:
            keep, _ = ops.wanda_select(W, sq, "nm", n=n_keep, m=n_of)
        packed = pack(W, keep)
        W = getattr(ops, "unpack_" + args.format)(*packed, want_mask=False)[0]      # the weight the packed bytes stand for
        packed_bytes = sum(t.numel() * t.element_size() for t in packed)
        pool = 2 * CACHE // packed_bytes + 1           # a round of the packed set holds more than twice the cache; the dense set more
        Ps, Ws = [tuple(t.clone() for t in packed) for _ in range(pool)], [W.clone() for _ in range(pool)]
        del keep
        for M in rows:
            x = torch.randn(M, K, device=DEV, generator=g).half()
            a, b = packed_fwd(x, *packed, unpack=True), packed_fwd(x, *packed, tiled=True)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (name, M)
            assert torch.equal(a.view(torch.int16), ops.linear_fwd(x, W).view(torch.int16)), (name, M)
            del a, b
            calls = {"unpack": lambda i: packed_fwd(x, *Ps[i], unpack=True), "tiled": lambda i: packed_fwd(x, *Ps[i], tiled=True),
                     "dense": lambda i: ops.linear_fwd(x, Ws[i])}
            graphs = {k: make_graph(f, pool) for k, f in calls.items()}
            t = {k: [] for k in calls}
            for _ in range(args.repeats):                                   # the routes alternate inside every repeat
                for k in calls:
                    t[k].append(graph_us(graphs[k], pool))
            (u, su), (ti, st), (d, sd) = (med_spread(t[k]) for k in ("unpack", "tiled", "dense"))
            win = ti < u - max(su, st)
            wins[M].append(win)
            line = (f"| {name} {N} x {K} | {M} | {u:.1f} ({su:.1f}) | {ti:.1f} ({st:.1f}) | {d:.1f} ({sd:.1f}) | {ti / u:.2f} | {ti / d:.2f} | "
                    f"{'yes' if win else 'no'} |")
            print(line, flush=True)
            lines.append(line)
            del graphs
        del Ps, Ws
        torch.cuda.empty_cache()
    limit = 0
    for M in rows:                                     # the largest ladder value with a win on every shape at it and at every one below
        if not (wins[M] and all(wins[M])):
            break
        limit = M
    tail = ["", "tiled wins on every shape: " + ", ".join(f"M = {M}: {sum(wins[M])} of {len(wins[M])}" for M in rows),
            f"largest row count up to which it wins on every shape, in this format: {limit}"]
    print("\n".join(tail), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines + tail) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--rows", default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--format", default="24", choices=("24", "48", "bm"), help="the packed format: 2:4 selectors, 4:8 bit masks or the bitmap of any mask")
    ap.add_argument("--density", type=float, default=0.5, help="--format bm: the share of every row's columns that is kept")
    ap.add_argument("--tiled", action="store_true", help="the unpack route, the tiled packed kernel and the dense kernel at the "
                    "prefill row counts " + ",".join(map(str, LADDER)))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_linear24.py measures on the GPU only"
    if args.tiled:
        return tiled_main(args)
    n_keep, n_of = (2, 4) if args.format == "24" else (4, 8)
    pack, packed_fwd = getattr(ops, "pack_" + args.format), getattr(ops, "linear_fwd_" + args.format)
    rows = [int(r) for r in args.rows.split(",")] if args.rows else list(ROWS)
    max_rows = ops.linear_fwd_bm_max_rows() if args.format == "bm" else ops.linear_fwd_24_max_rows()
    what = f"unstructured, {args.density:g} of every row kept" if args.format == "bm" else f"{n_keep}:{n_of}"
    lines = [f"format {what} (`vlmc_linear_fwd_{args.format}`); max_rows of this build: {max_rows}; fp16; median of {args.repeats} (spread = max - min); "
             "GB/s = weight bytes of the route / kernel time",
             "",
             "| shape (N x K) | M | packed kernel us (spread) | GB/s | dense kernel us (spread) | GB/s | packed / dense | "
             "graph: packed entry us | graph: unpack route us | graph: dense us |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    for name, (N, K) in SHAPES.items():
        if args.only and args.only not in name:
            continue
        g = torch.Generator(device=DEV).manual_seed(0)
        W = (torch.randn(N, K, device=DEV, generator=g) * 0.02).half()
        sq = torch.rand(K, device=DEV, generator=g) + 0.5
        if args.format == "bm":
            keep, _ = ops.wanda_select(W, sq, "row", k=K - int(round(K * args.density)))
        else:
            keep, _ = ops.wanda_select(W, sq, "nm", n=n_keep, m=n_of)
        packed = pack(W, keep)                         # (values, meta) or (values, meta, offs, rowptr)
        packed_bytes, dense_bytes = sum(t.numel() * t.element_size() for t in packed), W.numel() * 2
        pool = 2 * CACHE // min(packed_bytes, dense_bytes) + 1   # a round of the SMALLER set still holds more than twice the cache
        Ps, Ws = [tuple(t.clone() for t in packed) for _ in range(pool)], [W.clone() for _ in range(pool)]
        del keep
        for M in rows:
            x = torch.randn(M, K, device=DEV, generator=g).half()
            want = ops.linear_fwd(x, W)
            assert torch.equal(packed_fwd(x, *packed).view(torch.int16), want.view(torch.int16)), (name, M)
            calls = {"packed": lambda i: packed_fwd(x, *Ps[i]), "unpack": lambda i: packed_fwd(x, *Ps[i], unpack=True),
                     "dense": lambda i: ops.linear_fwd(x, Ws[i])}
            graphs = {k: make_graph(f, pool) for k, f in calls.items()}
            t = {k: [] for k in ("k_packed", "k_dense", "g_packed", "g_unpack", "g_dense")}
            for _ in range(args.repeats):                                   # the routes alternate inside every repeat
                if M <= max_rows:
                    t["k_packed"].append(kernel_us(calls["packed"], pool))
                t["k_dense"].append(kernel_us(calls["dense"], pool))
                for k in ("packed", "unpack", "dense"):
                    t["g_" + k].append(graph_us(graphs[k], pool))
            kd, sd = med_spread(t["k_dense"])
            if M <= max_rows:
                kp, sp = med_spread(t["k_packed"])
                pk = f"{kp:.1f} ({sp:.1f}) | {packed_bytes / kp / 1e3:.0f}"
                ratio = f"{kp / kd:.2f}"
            else:
                pk, ratio = "(unpack route) | -", "-"
            gp, gu, gd = (med_spread(t["g_" + k]) for k in ("packed", "unpack", "dense"))
            line = (f"| {name} {N} x {K} | {M} | {pk} | {kd:.1f} ({sd:.1f}) | {dense_bytes / kd / 1e3:.0f} | {ratio} | "
                    f"{gp[0]:.1f} ({gp[1]:.1f}) | {gu[0]:.1f} ({gu[1]:.1f}) | {gd[0]:.1f} ({gd[1]:.1f}) |")
            print(line, flush=True)
            lines.append(line)
            del graphs
        del Ps, Ws
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
