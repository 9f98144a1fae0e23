"""GPU parity of the attention backward (csrc/attention_bwd.hip, through the mi355_qkv_attention_vjp test op) against fp64 autograd of
softmax(q k^T / sqrt(ch)) v in both channel orders (QKVAttentionLegacy / QKVAttention, unet.py:424-487).

Every head size the backward instantiates (32, 64, 96, 128, 192, 256) x both orders x fp32 and bf16, at lengths shorter than one 64-row
tile (16, 49), exactly one tile (64), ragged tails (100, 300, 784) and a long sequence (1024), with several images and heads per call.
The op's workspace is filled with 0xFF bytes (NaN in fp32 and bf16) first, so a gradient entry the kernels never write fails the test.

Tolerances, max|err| / max|ref| of each of dq, dk, dv, set at about 3x the worst value measured on the MI355X over all 84 cases per
precision:
  fp32: < 1.5e-5 (measured: dq 3.8e-6, dk 4.6e-6, dv 2.6e-6).
  bf16: the reference is built from the bf16-rounded qkv and grad_out, so only the kernel's own roundings remain (A, P, dS as bf16 MFMA
        operands; the bf16 gradient store).  dq < 3.5e-2, dk < 4.5e-2, dv < 1.5e-2 (measured: 1.19e-2, 1.42e-2, 4.97e-3).  Bias of dq and
        dv: per channel, the mean of err and the mean of err * sign(ref) (a shrink or growth of the gradient, e.g. truncating instead of
        rounding) are each within 6 sigma of a mean of zero-mean errors (sigma = std(err) / sqrt(n)); measured worst: 0.89 of that bound.  dk has
        no bias check: its mean over keys is sum_q (sum_k dS) q, where the rounding of D = dA . A (A is the stored bf16 output, as in a
        differentiable plan) enters every key of a query alike, so its errors are not independent across keys (measured up to 1.3x the
        6 sigma of independent errors).
"""
import ctypes as C
import math

import pytest
import torch

from mi355 import _lib
from mi355.synth import randn
from oracle import unet_ref

DEV = "cuda:0"
HEAD_CHANNELS = (32, 64, 96, 128, 192, 256)
# (T, B, heads): below one tile, one tile, ragged tails, long; B > 1 and heads > 1 where the fp64 reference stays cheap
LENGTHS = ((16, 2, 3), (49, 2, 2), (64, 3, 2), (100, 2, 2), (300, 2, 1), (784, 1, 2), (1024, 1, 1))
FP32_MAX = 1.5e-5                                   # max|err| / max|ref|, every part
BF16_MAX = {"q": 3.5e-2, "k": 4.5e-2, "v": 1.5e-2}   # max|err| / max|ref| of dq, dk, dv


def attention64(qkv, heads, new_order):
    """fp64 softmax attention of qkv [B, 3 H ch, T] in the reference's two channel layouts (no intermediate rounding)."""
    B, width, T = qkv.shape
    ch = width // (3 * heads)
    if new_order:
        q, k, v = (t.reshape(B * heads, ch, T) for t in qkv.chunk(3, dim=1))
    else:
        q, k, v = qkv.reshape(B * heads, 3 * ch, T).split(ch, dim=1)
    w = torch.softmax(torch.einsum("bct,bcs->bts", q, k) / math.sqrt(ch), dim=-1)
    return torch.einsum("bts,bcs->bct", w, v).reshape(B, heads * ch, T)


def vjp64(qkv, grad_out, heads, new_order):
    x = qkv.double().requires_grad_()
    a = attention64(x, heads, new_order)
    (g,) = torch.autograd.grad((a * grad_out.double()).sum(), x)
    return g


def split_qkv(g, heads, new_order):
    """[B, 3 H ch, T] -> (dq, dk, dv), each [B, H ch, T] in head-major channel order."""
    B, width, T = g.shape
    ch = width // (3 * heads)
    if new_order:
        return tuple(g.chunk(3, dim=1))
    parts = g.reshape(B, heads, 3, ch, T)
    return tuple(parts[:, :, j].reshape(B, heads * ch, T) for j in range(3))


def _parts(got, ref, heads, new_order, centre):
    """(name, got, ref) of dq, dk, dv; centre: dq with its mean over channels removed (see test_attention_vjp_softmax_spike)."""
    for name, gp, rp in zip("qkv", split_qkv(got, heads, new_order), split_qkv(ref, heads, new_order)):
        if centre and name == "q":
            gp, rp = gp - gp.mean(dim=1, keepdim=True), rp - rp.mean(dim=1, keepdim=True)
        yield name, gp, rp


def check_fp32(got, ref, heads, new_order, tag, centre=False, bound=FP32_MAX):
    worst = 0.0
    for name, gp, rp in _parts(got, ref, heads, new_order, centre):
        scale = float(rp.abs().max())
        rel = float((gp - rp).abs().max()) / scale
        worst = max(worst, rel)
        print(f"   VJPSTAT {tag} d{name} max {rel:.3e}")
        assert rel < bound, f"{tag} d{name}: max|err| / max|ref| = {rel:.3e} (bound {bound})"
    return worst


def check_bf16(got, ref, heads, new_order, tag, bias=True, centre=False):
    worst, worst_bias = 0.0, 0.0
    for name, gp, rp in _parts(got, ref, heads, new_order, centre):
        scale = float(rp.abs().max())
        err = gp - rp
        rel = float(err.abs().max()) / scale
        worst = max(worst, rel)
        print(f"   VJPSTAT {tag} d{name} max {rel:.3e}")
        assert rel < BF16_MAX[name], f"{tag} d{name}: max|err| / max|ref| = {rel:.3e} (bound {BF16_MAX[name]})"
        if not bias or name == "k":
            continue
        n = err.shape[0] * err.shape[2]
        noise = 6.0 * float(err.std()) / math.sqrt(n) + 1e-7 * scale        # 6 sigma of a per-channel mean of zero-mean errors
        for what, e in (("mean error", err), ("mean error along sign(ref)", err * rp.sign())):
            b = float(e.mean(dim=(0, 2)).abs().max())
            worst_bias = max(worst_bias, b / noise)
            print(f"   VJPSTAT {tag} d{name} bias[{what}] {b / noise:.3f}")
            assert b < noise, f"{tag} d{name}: per-channel {what} {b:.3e} > 6 sigma {noise:.3e}"
    return worst, worst_bias


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


def test_fp64_reference_matches_the_oracle_layouts():
    """The fp64 reference is the oracle's attention (unet_ref.qkv_attention, fp32 softmax) in both channel orders."""
    q = randn(5, 2, 3 * 2 * 32, 40)
    for new in (False, True):
        torch.testing.assert_close(attention64(q.double(), 2, new).float(), unet_ref.qkv_attention(q, 2, new), rtol=1e-5, atol=1e-6)


def test_vjp_op_rejects_other_dtypes():
    """fp16 (and any other code) never reaches the backward kernels, which exist in fp32 and bf16 only: the op refuses it before launching."""
    L = _lib.lib()
    p = C.c_void_p(16)   # never dereferenced: the dtype check comes first
    rc = L.mi355_qkv_attention_vjp(p, p, p, 1, 1, 32, 16, 0, _lib.MI355_F16, p, 1 << 20, None)
    assert rc < 0 and b"qkv_attention_vjp" in L.mi355_last_error()
    rc = L.mi355_qkv_attention_vjp(p, p, p, 1, 1, 32, 16, 0, _lib.MI355_BF16X2, p, 1 << 20, None)
    assert rc < 0 and b"qkv_attention_vjp" in L.mi355_last_error()


def test_differentiable_plan_head_channel_limit():
    """The plan builder (host code) accepts head channels up to 256 in a differentiable plan and refuses 384 with the reason; the
    forward-only plan takes 384 (the forward kernels go to 512)."""
    def weight_bytes(mc, differentiable):
        c = _lib.make_config(image_size=8, in_channels=3, model_channels=mc, out_channels=3, num_res_blocks=1, attention_ds=(1,),
                             channel_mult=(1,), num_heads=1, dtype=_lib.MI355_F32, differentiable=differentiable)
        return _lib.lib().mi355_unet_weight_bytes(C.byref(c))

    assert weight_bytes(256, 1) > 0 and weight_bytes(384, 0) > 0
    assert weight_bytes(384, 1) < 0 and b"up to 256" in _lib.lib().mi355_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [_lib.MI355_F32, _lib.MI355_BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ch", HEAD_CHANNELS)
def test_attention_vjp_vs_fp64_autograd(ops, ch, dtype):
    bf = dtype == _lib.MI355_BF16
    worst, worst_bias = 0.0, 0.0
    for (T, B, heads) in LENGTHS:
        for new in (False, True):
            tag = f"ch={ch} T={T} B={B} heads={heads} new_order={new} {'bf16' if bf else 'fp32'}"
            seed = 100000 * ch + 10 * T + int(new)
            qkv = randn(seed, B, 3 * heads * ch, T) * 1.5          # logits of std ~2: peaked but not one-hot rows
            gout = randn(seed + 7, B, heads * ch, T)
            if bf:
                qkv, gout = qkv.bfloat16().float(), gout.bfloat16().float()
            ref = vjp64(qkv, gout, heads, new)
            got = ops.qkv_attention_vjp(qkv.to(DEV), gout.to(DEV), heads, new, dtype, ws_fill=0xFF).cpu().double()
            assert torch.isfinite(got).all(), f"{tag}: non-finite (unwritten) gradient entries"
            if bf:
                w, b = check_bf16(got, ref, heads, new, tag)
                worst_bias = max(worst_bias, b)
            else:
                w = check_fp32(got, ref, heads, new, tag)
            worst = max(worst, w)
    print(f"   ch={ch} {'bf16' if bf else 'fp32'}: worst max|err|/max|ref| {worst:.3e}, worst bias / 6 sigma {worst_bias:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [_lib.MI355_F32, _lib.MI355_BF16], ids=["fp32", "bf16"])
def test_attention_vjp_softmax_spike(ops, dtype):
    """The forward test's slow-path inputs (test_gpu_ops.py::test_attention_softmax_spike) through the backward, whose pass 1 rebuilds the
    softmax statistics L itself: a key far above the rest in a later tile (one query's row is one-hot), and every logit far below zero.
    The second input makes every q ~ +6 and every k ~ -6 in all channels (logits ~ -288): dq = sum_k dS k then carries -6 times the softmax
    row sum of dS, which is 0 in exact arithmetic and a rounding residue in fp32 / bf16 - an error along the all-channels direction, as large
    as dq itself, that any finite-precision implementation has.  So for that input dq is compared with its channel mean removed (dk and dv in
    full), and the fp32 bound is 2e-4: logits of magnitude 288 carry an fp32 rounding of ~3e-5 into every P (measured: 6e-5)."""
    bf = dtype == _lib.MI355_BF16
    B, heads, ch, T = 1, 1, 64, 256
    q = randn(11, B, 3 * ch, T) * 0.5
    q[0, ch:2 * ch, 200] = q[0, 0:ch, 7] * 40.0
    q2 = randn(12, B, 3 * ch, T) * 0.5
    q2[0, 0:ch] = 6.0 + 0.1 * q2[0, 0:ch]
    q2[0, ch:2 * ch] = -6.0 + 0.1 * q2[0, ch:2 * ch]
    for i, qkv in enumerate((q, q2)):
        gout = randn(13 + i, B, ch, T)
        if bf:
            qkv, gout = qkv.bfloat16().float(), gout.bfloat16().float()
        ref = vjp64(qkv, gout, heads, False)
        got = ops.qkv_attention_vjp(qkv.to(DEV), gout.to(DEV), heads, False, dtype, ws_fill=0xFF).cpu().double()
        assert torch.isfinite(got).all()
        tag = f"spike case {i} {'bf16' if bf else 'fp32'}"
        centre = i == 1
        if bf:
            w = check_bf16(got, ref, heads, False, tag, bias=False, centre=centre)[0]
        else:
            w = check_fp32(got, ref, heads, False, tag, centre=centre, bound=2e-4 if centre else FP32_MAX)
        print(f"   {tag}: max|err|/max|ref| {w:.3e}")
