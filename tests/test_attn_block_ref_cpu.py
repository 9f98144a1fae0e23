"""CPU: the fp64 reference and the inputs of tests/test_gpu_attn_block_ops.py (the fused AttentionBlock front half, csrc/attn_fused.hip).

attn_block64 is the whole op in fp64 with no intermediate rounding: h = a x + b, qkv = W h + bias, the per-head split in the legacy or the new
channel order, softmax(q^T k / sqrt(ch)) v.  Here it is held to something independent before a GPU is involved: the oracle's AttentionBlock
front half (oracle/unet_ref.py: group_norm32 -> 1x1 conv -> qkv_attention, fp32 eager), with (a, b) derived from fp64 GroupNorm32 statistics.

The input builders live here too so that what they promise is checked without a GPU: operands that are exact in fp32, bf16 AND fp16 (one
reference serves the three element types), a per-image (a, b) table with one image at a constant offset, and the three planted softmax cases
(a dominant key in the fourth 64-key tile, every logit near -288, a staircase of tile maxima).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from mi355.synth import rand_uniform, randn, synth_state_dict
from oracle import unet_ref
from tests.test_gpu_vjp_ops import attention64

CH = 64                       # head size of every fused form
SPIKE_Q, SPIKE_KEY = 7, 200   # case (i): key 200 = 40 x key 7, fourth 64-key tile
STAIR_Q, STAIR_KEYS, STAIR_STEP = 5, (70, 140, 210), 5.0   # case (iii): one planted key per later tile, +5 natural units of logit each


def attn_block64(x, a, b, w, bias, heads, new_order):
    """x [N, C, T], a / b [N, C], w [3C, C], bias [3C] -> [N, C, T], all in fp64."""
    h = a.double()[:, :, None] * x.double() + b.double()[:, :, None]
    qkv = torch.einsum("oc,nct->not", w.double(), h) + bias.double()[None, :, None]
    return attention64(qkv, heads, new_order)


def exact16(t):
    """Round to values that fp32, bf16 and fp16 all hold exactly: bf16's 8 significant bits, and nothing below fp16's normal range."""
    t = t.float().bfloat16().float()
    t = torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)
    assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t)
    return t


def head_rows(part, h, C, new_order):
    """Rows of q (part 0), k (1) or v (2) of head h in the [3C] output channels of the qkv conv."""
    base = part * C + h * CH if new_order else h * 3 * CH + part * CH
    return slice(base, base + CH)


def make_case(seed, N, C, T, new_order, softmax=None):
    """-> dict(x [N, C, T], a, b [N, C], w [3C, C], bias [3C], heads, offset_image).  x and w are exact in all three element types.
    a in [0.5, 2], b in [-1, 1], independent per image and channel; image (N - 1) // 2 has b = 4 everywhere: a table indexed by the wrong
    image is an O(1) error.  softmax: None, "spike", "low" or "stair" (module docstring; T = 256 only)."""
    heads = C // CH
    x = randn(seed, N, C, T)
    sd = synth_state_dict({"qkv.weight": (3 * C, C, 1), "qkv.bias": (3 * C,)}, seed + 1)
    w, bias = sd["qkv.weight"][:, :, 0].clone(), sd["qkv.bias"].clone()
    a = rand_uniform(seed + 2, 0.5, 2.0, N, C)
    b = rand_uniform(seed + 3, -1.0, 1.0, N, C)
    off = (N - 1) // 2
    b[off] = 4.0
    if softmax in ("spike", "stair"):      # q and k of head 0 = the head's first 64 normalised channels
        assert T == 256
        for part in (0, 1):
            rows = head_rows(part, 0, C, new_order)
            w[rows] = 0.0
            w[rows, :CH] = torch.eye(CH)
            bias[rows] = 0.0
    if softmax == "spike":
        x[:, :CH, SPIKE_KEY] = 40.0 * exact16(x[:, :CH, SPIKE_Q])
    elif softmax == "low":                 # q ~ +6, k ~ -6: every logit near -64 * 36 / 8 = -288
        for h in range(heads):
            for part, level in ((0, 6.0), (1, -6.0)):
                rows = head_rows(part, h, C, new_order)
                w[rows] *= 0.1
                bias[rows] = level + 0.1 * bias[rows]
    elif softmax == "stair":               # key s_j = c_j x the query's own normalised vector: logit = c_j |h_q|^2 / 8
        hq = a[:, :CH] * exact16(x[:, :CH, STAIR_Q]) + b[:, :CH]                      # [N, 64]
        self_logit = hq.pow(2).sum(dim=1, keepdim=True) / math.sqrt(CH)               # [N, 1]: the first tile's maximum (key = query)
        for j, key in enumerate(STAIR_KEYS):
            c = (self_logit + STAIR_STEP * (j + 1)) / self_logit
            x[:, :CH, key] = (c * hq - b[:, :CH]) / a[:, :CH]
    return dict(x=exact16(x), a=a, b=b, w=exact16(w), bias=bias, heads=heads, offset_image=off)


@pytest.mark.parametrize("new_order", [False, True], ids=["legacy", "new"])
@pytest.mark.parametrize("C,T,N", [(128, 256, 3), (256, 128, 2)])
def test_reference_matches_oracle_attention_block(C, T, N, new_order):
    """fp64 reference == oracle group norm -> 1x1 conv -> qkv_attention, with (a, b) from real GroupNorm32 statistics."""
    heads = C // CH
    x = randn(5100 + C + T, N, C, T) * 1.3 + 0.2
    sd = synth_state_dict({"norm.weight": (C,), "norm.bias": (C,), "qkv.weight": (3 * C, C, 1), "qkv.bias": (3 * C,)}, 5200 + C)
    qkv = F.conv1d(unet_ref.group_norm32(x, sd["norm.weight"], sd["norm.bias"]), sd["qkv.weight"], sd["qkv.bias"])
    want = unet_ref.qkv_attention(qkv, heads, new_order)
    xg = x.double().reshape(N, 32, -1)
    mean, var = xg.mean(dim=2), xg.var(dim=2, unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    cpg = C // 32
    a = sd["norm.weight"].double()[None] * rstd.repeat_interleave(cpg, dim=1)
    b = sd["norm.bias"].double()[None] - mean.repeat_interleave(cpg, dim=1) * a
    got = attn_block64(x, a, b, sd["qkv.weight"][:, :, 0], sd["qkv.bias"], heads, new_order)
    assert got.dtype == torch.float64 and got.shape == want.shape
    torch.testing.assert_close(got.float(), want, rtol=0, atol=1e-5)   # fp32 eager against fp64: values are O(1), sums of <= 256 terms
    # the two orders are different functions of the same weights: the reference must not ignore the flag
    other = attn_block64(x, a, b, sd["qkv.weight"][:, :, 0], sd["qkv.bias"], heads, not new_order)
    assert (other - got).abs().max() > 1e-2


def _logits64(c, head, new_order):
    C = c["x"].shape[1]
    h = c["a"].double()[:, :, None] * c["x"].double() + c["b"].double()[:, :, None]
    qkv = torch.einsum("oc,nct->not", c["w"].double(), h) + c["bias"].double()[None, :, None]
    q, k = qkv[:, head_rows(0, head, C, new_order)], qkv[:, head_rows(1, head, C, new_order)]
    return torch.einsum("nct,ncs->nts", q, k) / math.sqrt(CH)


SOFTMAX_N = 4                                                    # images of a softmax case in the GPU tests
SOFTMAX_SEED = {"spike": 78, "low": 79, "stair": 80}             # + C: the GPU tests build the very cases checked here


@pytest.mark.parametrize("new_order", [False, True], ids=["legacy", "new"])
@pytest.mark.parametrize("C", [128, 256])
def test_inputs_are_what_the_gpu_tests_rely_on(C, new_order):
    N, T = SOFTMAX_N, 256
    c = make_case(77, N, C, T, new_order)
    assert c["a"].min() >= 0.5 and c["a"].max() <= 2.0 and (c["b"][c["offset_image"]] == 4.0).all()
    assert (c["a"][0] - c["a"][1]).abs().mean() > 0.2            # the tables differ from image to image
    plain = attn_block64(**{k: c[k] for k in ("x", "a", "b", "w", "bias", "heads")}, new_order=new_order)
    swapped = attn_block64(c["x"], c["a"].roll(1, 0), c["b"].roll(1, 0), c["w"], c["bias"], c["heads"], new_order)
    assert (swapped - plain).pow(2).mean().sqrt() > 0.3          # a table of the wrong image is an O(1) error

    s = make_case(SOFTMAX_SEED["spike"] + C, N, C, T, new_order, "spike")
    lg = _logits64(s, 0, new_order)
    assert SPIKE_KEY // 64 == 3
    rest = torch.cat([lg[:, SPIKE_Q, :SPIKE_KEY], lg[:, SPIKE_Q, SPIKE_KEY + 1:]], dim=1)
    assert (lg[:, SPIKE_Q, SPIKE_KEY] - rest.max(dim=1).values).min() > 100   # dominant, far beyond the rescale threshold

    lo = make_case(SOFTMAX_SEED["low"] + C, N, C, T, new_order, "low")
    for head in range(C // CH):
        lg = _logits64(lo, head, new_order)
        assert lg.max() < -200 and lg.min() > -400                # exp2 of the raw logits would underflow to an all-zero row

    st = make_case(SOFTMAX_SEED["stair"] + C, N, C, T, new_order, "stair")
    lg = _logits64(st, 0, new_order)[:, STAIR_Q].reshape(N, 4, 64).max(dim=2).values * math.log2(math.e)   # tile maxima, log2 domain
    ok = [n for n in range(N) if n != st["offset_image"]]
    steps = (lg[ok, 1:] - lg[ok, :-1])
    assert steps.min() > 6.0 and steps.max() < 8.0, steps          # each step stays below the threshold of 8 ...
    assert (lg[ok, 2] - lg[ok, 0]).min() > 8.0                     # ... and two of them exceed it: deferred first, then moved
