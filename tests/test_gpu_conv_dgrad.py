"""GPU: the data gradient of a convolution as unet_backward computes it, op by op, against fp64 autograd.

mi355_conv2d_vjp packs the filter with conv_pack_weights_dgrad and calls conv_dgrad_launch (csrc/unet_backward.hip), the helper the backward
walker itself calls: zero stuffing for stride 2, one bias-free NHWC unit-mode conv on whichever kernel conv_route picks, 2x2 block sums for
nearest x2, and either the scatter into the one or two source gradients (with their accumulate flags) or the raw cin_pad-channel buffer the
GroupNorm adjoint reads.  Reference and shape table: tests/conv_dgrad_ref.py (held to the maths on the CPU by tests/test_conv_dgrad_ref_cpu.py).
For bf16 the filter, the cotangent and any pre-filled gradient are rounded to bf16 first: the reference is fp64 on the values the kernels read.
Every call fills the op's scratch with 0xFF bytes, so an element no kernel writes comes back NaN.

Budget, element by element, with mag = the same fp64 gradient of |W| and |G| (+ |pre-filled gradient|), the sum of |terms|:
  fp32   |err| <= 4 x max|fp32 eager CPU autograd - fp64| + C_SUM x 2^-24 x mag.  C_SUM = 20: fp32 eager's own error, measured on the CPU over
         this table, reaches 5.05 x 2^-24 x mag (the out conv's adjoint at 20x28; 4.4 for the 1x1 convs over a concat); 4 x that for a
         different summation order (MFMA partial sums per chunk and tap instead of a GEMM's blocking).
  bf16   the same, plus 1.01 x 2^-8 x |stored value| for every bf16 store on the path: the conv's output du (nearest x2: over the 2x2
         block's sum of |du|, the four stored values the block sum reads), and the destination once more where it is rounded a second time
         (the block sum of nearest x2; an accumulating scatter).  A scatter that overwrites copies du and rounds nothing.
Channels beyond the forward conv's input channels are exactly zero.  The padding channels of the out conv's cotangent (3 real channels of a
16- / 32-channel chunk) are zero by construction - pack_nhwc writes them, as for the network's own cotangent, and the packed filter has zero
columns there - so there is no junk variant of that case.  The stuffed zeros of stride 2 live in scratch; they show in the result only.
bf16 also gets the bias check of test_gpu_ops.test_first_conv_kernel per output channel, and the border ring and the interior are held to the
element-wise budget separately.

Measured on the MI355X (worst err / budget over all cases, the DGRADSUM lines; DESIGN.md section 8b has the table): fp32 0.276, bf16 0.984
(a correctly rounded bf16 store of an exact value alone measures 1 / 1.01 = 0.99 of its term).
"""
import math

import pytest
import torch

from mi355 import _lib
from mi355.synth import randn
from tests.conv_dgrad_ref import CASES, KERNEL_NAMES, UP2, WANT_KERNELS, chunk, cin_pad_of, dgrad_autograd, out_size

DEV = "cuda:0"
F32, BF16 = _lib.MI355_F32, _lib.MI355_BF16
NAME = {F32: "fp32", BF16: "bf16"}
T16 = {F32: None, BF16: torch.bfloat16}
U32, U16 = 2.0 ** -24, {F32: 0.0, BF16: 2.0 ** -8}
C_SUM = 20.0

REACHED = {F32: {}, BF16: {}}     # case index -> kernel the launch reported
WORST = {F32: {}, BF16: {}}       # case index -> worst err / budget


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


def _pad(t, C):
    out = torch.zeros(t.shape[0], C, *t.shape[2:], dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def _ring(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def _check(tag, dtype, got, want, f32, mag, stored, second, creal):
    """got against want [B, C, h, w] under the budget of the module docstring.  stored: |du| the first bf16 store rounds (summed over the 2x2 block
    for nearest x2); second: the destination is rounded once more; creal: channels from this index on are exactly zero.  -> worst err / budget"""
    got = got.cpu().double()
    assert torch.isfinite(got).all(), f"{tag}: {int((~torch.isfinite(got)).sum())} entries no kernel wrote (NaN)"
    assert torch.equal(got[:, creal:], torch.zeros_like(got[:, creal:])), f"{tag}: channels >= {creal} must be exactly zero"
    got, want, f32, mag, stored = (t[:, :creal] for t in (got, want, f32, mag, stored))
    e32 = float((f32.double() - want).abs().max())
    bud = 4 * e32 + C_SUM * U32 * mag + 1.01 * U16[dtype] * (stored + (want.abs() if second else 0.0))
    err = got - want
    ratio = err.abs() / bud
    h, w = got.shape[2:]
    ring = _ring(h, w)
    r_ring, r_in = float(ratio[..., ring].max()), float(ratio[..., ~ring].max()) if (~ring).any() else 0.0
    print(f"   DGRADSTAT {tag}: fp32 autograd err {e32:.3e} kernel err {float(err.abs().max()):.3e} worst err / budget ring {r_ring:.3f} interior {r_in:.3f}")
    assert r_ring <= 1.0, f"{tag}: border ring: err / budget {r_ring:.3f}"
    assert r_in <= 1.0, f"{tag}: interior: err / budget {r_in:.3f}"
    if dtype == BF16:       # zero-mean: truncation instead of rounding, or a tap that is always missing, shifts a channel's mean error
        n = got.shape[0] * h * w
        rms = err.pow(2).mean(dim=(0, 2, 3)).sqrt()
        noise = 6.0 * rms / math.sqrt(n) + C_SUM * U32 * mag.mean(dim=(0, 2, 3)) + 4 * e32
        m1 = err.mean(dim=(0, 2, 3)).abs()
        m2 = (err * want.sign()).mean(dim=(0, 2, 3)).abs()
        assert bool((m1 <= noise).all()), f"{tag}: mean error of channel {int((m1 - noise).argmax())}: {float((m1 / noise).max()):.2f} x 6 sigma"
        assert bool((m2 <= noise).all()), f"{tag}: mean signed error of channel {int((m2 - noise).argmax())}: {float((m2 / noise).max()):.2f} x 6 sigma"
    return max(r_ring, r_in)


def run_case(ops, dtype, idx):
    name, B, Co, Ci, c0, c1, h, w, k, mode, forms = CASES[idx]
    t16 = T16[dtype]
    rnd = (lambda t: t.to(t16).float()) if t16 else (lambda t: t)
    c0 = c0 if c0 is not None else chunk(dtype)
    Ho, Wo = out_size(h, w, mode)
    cp = cin_pad_of(c0, c1)
    W = rnd(randn(95000 + idx, Co, Ci, k, k) / math.sqrt(Ci * k * k))
    G = rnd(randn(96000 + idx, B, Co, Ho, Wo))
    pre = [rnd(randn(97000 + idx, B, c0, h, w) * 2.0), rnd(randn(97500 + idx, B, c1, h, w) * 2.0) if c1 else None]
    a0, a1, hi = dgrad_autograd(W, G, c0, c1, h, w, mode, with_hi=True)                       # the reference, computed once per case
    m = dgrad_autograd(W.abs(), G.abs(), c0, c1, h, w, mode)
    f = dgrad_autograd(W, G, c0, c1, h, w, mode, dtype=torch.float32)
    cat = lambda ts: torch.cat([t for t in ts if t is not None], dim=1)
    ref, mag, f32 = _pad(cat((a0, a1)), cp), _pad(cat(m), cp), _pad(cat(f), cp)
    stored = _pad(hi.abs().reshape(B, Ci, h, 2, w, 2).sum(dim=(3, 5)), cp) if mode == UP2 else ref.abs()
    Gd = G.to(DEV)
    worst, kernels = 0.0, set()
    for form in forms:
        info = {}
        if form == "raw":
            got = ops.conv2d_vjp(W, Gd, c0, c1, hw=(h, w), mode=mode, raw=True, dtype=dtype, ws_fill=0xFF, info=info)
            tag = f"{NAME[dtype]} {name} B={B} raw [{KERNEL_NAMES[info['kernel']]} form {info['form']} {info['tile_m']}x{info['tile_n']}]"
            assert tuple(got.shape) == (B, cp, h, w)
            worst = max(worst, _check(tag, dtype, got, ref, f32, mag, stored, mode == UP2, Ci))
        else:
            g_in = [pre[j].clone().to(DEV) if (form[j] and pre[j] is not None) else None for j in range(2)]
            got = ops.conv2d_vjp(W, Gd, c0, c1, hw=(h, w), mode=mode, g0=g_in[0], g1=g_in[1], dtype=dtype, ws_fill=0xFF, info=info)
            off = 0
            for j, cj in enumerate((c0, c1)):
                if not cj:
                    continue
                acc = bool(form[j])
                tag = (f"{NAME[dtype]} {name} B={B} scatter acc={tuple(form)} source {j} "
                       f"[{KERNEL_NAMES[info['kernel']]} form {info['form']} {info['tile_m']}x{info['tile_n']}]")
                sl = slice(off, off + cj)
                p64 = pre[j].double() if acc else 0.0
                p32 = (f32[:, sl] + pre[j]) if acc else f32[:, sl]            # fp32 eager: the gradient, then the add, both in fp32
                worst = max(worst, _check(tag, dtype, got[j], ref[:, sl] + p64, p32, mag[:, sl] + (pre[j].double().abs() if acc else 0.0),
                                          stored[:, sl], acc or mode == UP2, cj if acc else max(0, min(cj, Ci - off))))
                off += cj
        kernels.add(info["kernel"])
        want_route = ops.conv2d_vjp_route(B, Co, Ci, c0, c1, h, w, k, mode, dtype=dtype)
        assert info == want_route, f"{NAME[dtype]} {name}: launched {info}, conv_route says {want_route}"
    assert len(kernels) == 1
    REACHED[dtype][idx] = kernels.pop()
    WORST[dtype][idx] = worst


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0].replace("->", "_to_").replace(" ", "_") for c in CASES])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_conv_dgrad_vs_fp64_autograd(ops, dtype, idx):
    run_case(ops, dtype, idx)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_conv_dgrad_reaches_every_kernel(ops, dtype):
    """The routes the launches above reported (a case this session did not run is run here): every kernel a bias-free NHWC unit-mode conv can be
    routed to was launched at least once in this element type.  All six exist for fp32 and bf16: there is no documented exception."""
    for idx in range(len(CASES)):
        if idx not in REACHED[dtype]:
            run_case(ops, dtype, idx)
    by_kernel = {}
    for idx, kk in REACHED[dtype].items():
        by_kernel.setdefault(kk, []).append(idx)
    wi = max(WORST[dtype], key=WORST[dtype].get)
    print(f"   DGRADSUM conv dgrad {NAME[dtype]}: worst err / budget {WORST[dtype][wi]:.3f} ({CASES[wi][0]}); kernels "
          + ", ".join(f"{KERNEL_NAMES[kk]} x{len(v)}" for kk, v in sorted(by_kernel.items())))
    assert set(by_kernel) >= WANT_KERNELS, f"{NAME[dtype]}: reached {sorted(KERNEL_NAMES[x] for x in by_kernel)}, wanted {sorted(KERNEL_NAMES[x] for x in WANT_KERNELS)}"
