"""vlmc_attn_fwd against the unfused chain on this library's kernels and against vlmc_sdpa_fwd, at the shapes of a prune (us per call).
`--pre`: also the ViT-g attention front -- torch's qkv-bias add and q scale plus the kernel against vlmc_attn_fwd_pre on the raw slices."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vlm-compression_amd"))
import torch
from vlmc import ops

dev = "cuda:0"


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / n


def heads(B, T, H, d, dtype):
    return torch.randn(B, T, H * d, device=dev).to(dtype).view(B, T, H, d).transpose(1, 2)


SHAPES = [("vit-g self (fp16)", torch.float16, 128, 16, 257, 257, 88, 0, False),
          ("t5 enc self 96 (bf16, bias + mask)", torch.bfloat16, 128, 32, 96, 96, 64, 1, True),
          ("t5 enc self 160 (bf16, bias + mask)", torch.bfloat16, 128, 32, 160, 160, 64, 1, True),
          ("t5 dec self 16", torch.bfloat16, 128, 32, 16, 16, 64, 1, True),
          ("t5 dec cross 16 x 160", torch.bfloat16, 128, 32, 16, 160, 64, 1, True),
          ("qformer self 64 (fp16, /8 + mask)", torch.float16, 128, 12, 64, 64, 64, 1, False),
          ("qformer cross 32 x 257", torch.float16, 128, 12, 32, 257, 64, 0, False)]
print("| shape | fused us | unfused chain us | sdpa kernel us (no bias: another op) | score bytes MB |")
print("|---|---|---|---|---|")
for name, dt, B, H, Tq, Tk, d, nadd, f32 in SHAPES:
    q, k, v = heads(B, Tq, H, d, dt), heads(B, Tk, H, d, dt), heads(B, Tk, H, d, dt)
    adds = [torch.randn(B, H, Tq, Tk, device=dev).to(dt)] if nadd else []
    mul = 0.125 if "qformer" in name else None

    def unfused():
        s = ops.attn_matmul(q, k.transpose(-1, -2))
        if mul is not None:
            s = s * mul
        for t in adds:
            s = s + t
        p = ops.softmax_rows(s.float()).type_as(s) if f32 else ops.softmax_rows(s)
        return ops.attn_matmul(p, v)
    tf = timeit(lambda: ops.attn_fused(q, k, v, mul, adds))
    tu = timeit(unfused)
    try:
        ts = timeit(lambda: ops.sdpa(q, k, v))
    except Exception:
        ts = float("nan")
    print(f"| {name} [{B}, {H}, {Tq}, {Tk}, {d}] | {tf:.1f} | {tu:.1f} | {ts:.1f} | {B * H * Tq * Tk * 2 / 1e6:.0f} |", flush=True)

# ---- the ViT-g attention front (eva_vit.py:133-141): torch's bias add and q scale in front of the kernel against vlmc_attn_fwd_pre --
# `--pre` only: repeated, so that the spread of a route shows next to the difference between the routes
if "--pre" in sys.argv:
    import numpy as np
    B, H, N, d, dt = 128, 16, 257, 88, torch.float16
    C = H * d
    y = (torch.randn(B, N, 3 * C, device=dev) * 0.5).to(dt)
    bias = torch.cat(((torch.randn(C, device=dev) * 0.5).to(dt), torch.zeros(C, device=dev, dtype=dt), (torch.randn(C, device=dev) * 0.5).to(dt)))
    scale = d ** -0.5
    qmul = float(np.float32(scale))

    def slices(t):
        t = t.reshape(B, N, 3, H, -1).permute(2, 0, 3, 1, 4)
        return t[0], t[1], t[2]

    def materialized():
        q, k, v = slices(y + bias)
        return ops.attn_fused(q * scale, k, v)
    q0, k0, v0 = slices(y)
    kw = dict(q_add=bias[:C].view(H, d), k_add=bias[C:2 * C].view(H, d), v_add=bias[2 * C:].view(H, d), q_mul=qmul)
    assert torch.equal(materialized(), ops.attn_fused(q0, k0, v0, **kw))
    qm, km, vm = slices(y + bias)
    qm = qm * scale
    nbytes = {"add": 2 * B * N * 3 * C * 2, "mul": 2 * B * N * C * 2}
    print(f"\nViT-g attention front [{B}, {H}, {N}, {N}, {d}] fp16; `qkv + bias` moves {nbytes['add'] / 1e6:.0f} MB, `q * scale` {nbytes['mul'] / 1e6:.0f} MB (8 TB/s HBM peak)")
    print("| run | kernel on materialized operands us | torch add us (TB/s) | torch mul us (TB/s) | add + mul + kernel us | vlmc_attn_fwd_pre us | kernel without pre-ops on the packed slices us |")
    print("|---|---|---|---|---|---|---|")
    for r in range(5):
        t_k = timeit(lambda: ops.attn_fused(qm, km, vm), 50)
        t_a = timeit(lambda: y + bias, 50)
        t_m = timeit(lambda: q0 * scale, 50)
        t_all = timeit(materialized, 50)
        t_p = timeit(lambda: ops.attn_fused(q0, k0, v0, **kw), 50)
        t_0 = timeit(lambda: ops.attn_fused(q0, k0, v0), 50)
        print(f"| {r} | {t_k:.1f} | {t_a:.1f} ({nbytes['add'] / t_a / 1e6:.2f}) | {t_m:.1f} ({nbytes['mul'] / t_m / 1e6:.2f}) | {t_all:.1f} | {t_p:.1f} | {t_0:.1f} |", flush=True)
