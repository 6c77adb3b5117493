"""GPU: torch's `F.silu` gives an element the same bits wherever it lies in a tensor -- unlike `F.gelu`, whose last partial block is
compiled to other instructions (csrc/elementwise.hip).  The gated feed-forward of the reference's LLaMA layer
(modeling_llama.py:156-160, `act_fn(gate_proj(x)) * up_proj(x)`) therefore needs no kernel of this library to be batch-invariant
during a replay; this test is the evidence DESIGN.md cites, and the alarm if a later torch build changes it."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_silu_has_the_same_bits_in_a_tensors_body_and_in_its_tail(dtype):
    v = torch.arange(65536, dtype=torch.int32, device=DEV).to(torch.int16).view(dtype)        # every 16-bit input
    big = torch.cat([v, v, v, v, v[:12345]])
    body = F.silu(big)[:65536].view(torch.int16)
    nan = torch.isnan(v.float())
    for chunk in (100, 1000, 2048, 4096, 5000):                                             # tensors that are all "last partial block"
        tail = torch.cat([F.silu(v[i:i + chunk].clone()) for i in range(0, 65536, chunk)]).view(torch.int16)
        assert int(((tail != body) & ~nan).sum()) == 0, chunk
    odd = F.silu(big[:65536 + 777]).view(torch.int16)[65536:]
    assert torch.equal(odd, F.silu(big).view(torch.int16)[65536:65536 + 777])
    # .. and it is the documented formula in fp32, rounded once
    x = v.float()
    want = (x / (1.0 + torch.exp(-x))).to(dtype).view(torch.int16)
    assert int(((want != body) & ~nan).sum()) == 0


def test_gated_feed_forward_rows_do_not_depend_on_the_batch():
    g = torch.Generator(device=DEV).manual_seed(0)
    gate, up = (torch.randn(6, 77, 11008, generator=g, device=DEV) * 2).half(), torch.randn(6, 77, 11008, generator=g, device=DEV).half()
    whole = F.silu(gate) * up
    for i in range(6):
        for n in (77, 13, 1):
            assert torch.equal(F.silu(gate[i:i + 1, :n]) * up[i:i + 1, :n], whole[i:i + 1, :n])
