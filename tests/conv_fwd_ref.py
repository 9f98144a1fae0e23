"""One forward convolution of the U-Net: the fp64 reference on the values the kernel reads, its error budget, and the case table.

  out = bias + emb[n] + R(res) + conv(G(P(cat(x0, x1))), W, stride, pad)        (csrc/ops.h, the comment above ConvMode)

  operands(case, dt)   seeded inputs: x, res and W already rounded to the element type (bf16x2: W = bf16(W) + bf16(W - bf16(W)), the two halves the
                       packer stores), everything else fp32 numbers taken as exact
  reference(case, o)   want (fp64), mag (the same expression over the absolute value of every term, |P| included), magpro = conv(G(|a| |v| + |b|), |W|) for
                       SiLU rows (the magnitudes the fp32 evaluation of a v + b rounds), f32 (the same composition in fp32 eager torch), q =
                       sqrt(conv(G(P)^2, W^2)) (the 2-norm of the products) and cabs = conv(|G(P)|, |W|)
  budget(case, dt, r)  the element-wise bound, fixed before any GPU run (DESIGN.md section 8c derives every term):
      SiLU prologue   + 2.2 x 2^-24 magpro: two roundings of a v + b in fp32 through a slope of at most 1.1 (any type)
      fp32            4 max|f32 - want| + C_SUM 2^-24 mag                                   (C_SUM = 23: four times eager's own worst, below)
      16-bit, NHWC    + 1.01 u |want| for the rounded store (u = 2^-8 bf16, 2^-11 fp16; fp16: at least 2^-25, half the smallest subnormal)
      16-bit, SiLU    + 6 u / sqrt(3) q: the kernel rounds each staged activation, the reference does not (six sigma of the sum of independent
                      errors of at most u |w p| each).  An affine-only prologue gets no such term: its operands sit on a grid where a v + b is exact
      phase form      + 1.01 u_w cabs (u_w = 2^-24 / 2^-8 / 2^-11): one more rounding of the pre-summed filter.  That difference is fixed per weight, so
                      the per-channel MEAN checks of a phase launch are taken against fp64 on the filter the kernel reads (want_phase), unwidened
      axpy            the stored value is x + s v in fp32: mag includes |x|; the NCHW fp32 out conv has no store term in any type
  check(...)          finite everywhere (NaN = no kernel wrote it), the border ring and the interior under the budget separately, and for the 16-bit
                      types each output channel's mean error and mean signed error within six sigma
  emulate16(...)      what a correct 16-bit kernel computes, in plain torch (P rounded to the type, products and sums in fp32, the store rounded), with
                      three switchable defects; tests/test_conv_fwd_ref_cpu.py holds the budget to it
  CASES               the rows tests/test_gpu_conv_fwd.py runs; each names the kernel family and form conv_route must pick for it (fam, form) and
                      EXPECT holds the tile and the remaining route words per element type

The first conv: the packed channels beyond the real ones (cin_real .. 32) hold zeros and see zero weights.  A kernel that contracted over them
anyway would still be right; one that read the real channels from the wrong slot would not.  The rows therefore show that the real channels are read
where they are, not that the padding is skipped.
"""
import math

import torch
import torch.nn.functional as F

from mi355.synth import rand_uniform, randn

# csrc/ops.h ConvKernel
K_IGEMM, K_1X1, K_1X1_PP, K_IN, K_OUT, K_PP, K_WS, K_SMALL = range(8)
KERNEL_NAMES = ["igemm", "1x1", "1x1_pp", "in", "out", "pp", "ws", "small"]

TYPES = ("fp32", "bf16", "fp16", "bf16x2")
T16 = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16, "bf16x2": torch.bfloat16}
U16 = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "bf16x2": 2.0 ** -8}
UW = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
U32 = 2.0 ** -24
C_SUM = 23.0   # four times fp32 eager's own worst error over this table, 5.67 x 2^-24 x mag (tests/test_conv_fwd_ref_cpu.py; the dgrad table's 5.05 gave 20)
# a v + b in fp32 without a fused multiply-add is two roundings, at most 2 x 2^-24 (|a v| + |b|); SiLU's slope is at most 1.1
K_FMA = 2.2
ALL3 = ("fp32", "bf16", "fp16")
H16 = ("bf16", "fp16")


def dtype_code(dt):
    from mi355 import _lib

    return {"fp32": _lib.MI355_F32, "bf16": _lib.MI355_BF16, "fp16": _lib.MI355_F16, "bf16x2": _lib.MI355_BF16X2}[dt]


def rnd(t, dt):
    """t rounded to the element type of dt, as fp32."""
    return t if T16[dt] is None else t.to(T16[dt]).float()


def out_size(c):
    hc, wc = (2 * c["h"], 2 * c["w"]) if c["up"] else (c["h"], c["w"])
    p = c["k"] // 2
    return (hc + 2 * p - c["k"]) // c["s"] + 1, (wc + 2 * p - c["k"]) // c["s"] + 1


# ---- operands ----------------------------------------------------------------------------------------------------------------------------
def operands(c, dt):
    """Seeded operands of case c in element type dt (CPU fp32 tensors).  Activations carry a per-image offset and scale, (a, b) differ per image and
    channel, bias and emb are of order 1."""
    sd = 7000 + 37 * c["idx"]
    B, ci, c1, co, h, w, k = c["B"], c["cin"], c["c1"], c["cout"], c["h"], c["w"], c["k"]
    ct = ci + c1
    Ho, Wo = out_size(c)
    o = {}
    n = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    if c["pro"] == "affine":     # the grid on which a v + b is exact in bf16 and fp16: v = m / 16, a in {0.5, 1, 2}, b = j / 16
        m = (randn(sd, B, ct, h, w) * 30).round().clamp(-90, 90)
        x = m / 16
        a = torch.tensor([0.5, 1.0, 2.0])[(torch.arange(B * ct) * 7 % 3).view(B, ct)]
        j = (randn(sd + 1, B, ct) * 20).round().clamp(-60, 60)
        o["a"], o["b"] = a.contiguous(), (j / 16).contiguous()
    else:
        x = randn(sd, B, ct, h, w) * (0.6 + 0.4 * n) + 0.3 * (n - 0.5)
        if c["pro"] == "silu":
            a = 0.5 + 0.75 * rand_uniform(sd + 1, 0.0, 1.0, B, ct)
            a = torch.where((torch.arange(B * ct).view(B, ct) % 8) == 3, -a, a)
            o["a"], o["b"] = a.contiguous(), (0.5 * randn(sd + 2, B, ct)).contiguous()
    x = rnd(x, dt)
    o["x"], o["x1"] = x[:, :ci].contiguous(), (x[:, ci:].contiguous() if c1 else None)
    W = randn(sd + 3, co, ct, k, k) / math.sqrt(ct * k * k)
    if dt == "bf16x2":
        hi = rnd(W, "bf16")
        o["W64"] = hi.double() + rnd(W - hi, "bf16").double()      # what the two packed halves sum to
    else:
        o["W64"] = rnd(W, dt).double()
    o["W"] = W                                                   # what the op is given: the packer rounds it
    o["bias"] = randn(sd + 4, co) if c["bias"] else None
    o["emb"] = randn(sd + 5, B, co) if c["emb"] else None
    if c["res"]:
        hr, wr = (Ho, Wo) if c["res"] == 1 else (Ho // 2, Wo // 2)
        o["res"] = rnd(randn(sd + 6, B, co, hr, wr), dt)
    else:
        o["res"] = None
    o["dt"] = dt
    o["axpy_x"], o["axpy_s"] = (randn(sd + 8, B, co, Ho, Wo), 0.37) if c["axpy"] else (None, 0.0)
    return o


def axpy_applied(c):
    """The row hands over axpy_x and the launch applies it: conv_edge bit 3 (on by default); otherwise the out conv stores v and leaves axpy_x alone."""
    return bool(c["axpy"]) and bool(c.get("knobs", {}).get("conv_edge", 15) & 8)


def _pro(x, o, c, dtype, absval=False):
    if not c["pro"]:
        return x.abs() if absval else x
    a, b = o["a"].to(dtype)[:, :, None, None], o["b"].to(dtype)[:, :, None, None]
    if absval == "fma":
        return a.abs() * x.abs() + b.abs()
    v = a * x + b
    v = F.silu(v) if c["pro"] == "silu" else v
    return v.abs() if absval else v


def phase_weights(W, dt):
    """The four phase filters conv_pack_weights_up2 builds from the fp32 filter W [Co, Ci, 3, 3], as nine-tap filters of the up-sampled image: tap
    ky' of phase (a, b) is the sum of the rows ky with (a + ky + 1) / 2 == a + ky' (the same along x), summed in fp32 in the packer's order (ky, then kx,
    from 0) and rounded ONCE to the element type; here it sits on the first tap of its group (the group's taps read the same low-res pixel, zero
    padding included) and the group's other taps are zero.  -> [4][Co, Ci, 3, 3] fp32, phase 2 a + b"""
    out = []
    for pa in (0, 1):
        for pb in (0, 1):
            E = torch.zeros_like(W)
            for ty in (0, 1):
                for tx in (0, 1):
                    taps = [(ky, kx) for ky in range(3) for kx in range(3) if (pa + ky + 1) // 2 == pa + ty and (pb + kx + 1) // 2 == pb + tx]
                    v = torch.zeros_like(W[:, :, 0, 0])
                    for ky, kx in taps:
                        v = v + W[:, :, ky, kx]
                    E[:, :, taps[0][0], taps[0][1]] = rnd(v, dt)
            out.append(E)
    return out


def _phase_conv(p, Wph):
    """The up-sampled image p through the four phase filters: output pixel (2 i + a, 2 j + b) from filter 2 a + b."""
    y = None
    for ph, E in enumerate(Wph):
        t = F.conv2d(p, E.to(p.dtype), padding=1)
        y = torch.empty_like(t) if y is None else y
        y[..., ph >> 1::2, ph & 1::2] = t[..., ph >> 1::2, ph & 1::2]
    return y


def phase_row(c):
    """The row's shape is one the phase form of the ping-pong kernel can take (a prologue-free 3x3 conv behind nearest x2)."""
    return bool(c["up"]) and not c["pro"] and c["k"] == 3 and c["s"] == 1


def _compose(c, o, dtype, W, absval=False, square=False, conv_only=False, Wph=None):
    x = torch.cat([o["x"]] + ([o["x1"]] if o["x1"] is not None else []), dim=1).to(dtype)
    p = _pro(x, o, c, dtype, absval)
    if c["up"]:
        p = F.interpolate(p, scale_factor=2, mode="nearest")
    if square:
        p, W = p * p, W * W
    y = _phase_conv(p, Wph) if Wph is not None else F.conv2d(p, W, stride=c["s"], padding=c["k"] // 2)       # zero padding after P
    if conv_only:
        return y
    ab = (lambda t: t.abs()) if absval else (lambda t: t)
    if o["bias"] is not None:
        y = y + ab(o["bias"].to(dtype))[None, :, None, None]
    if o["emb"] is not None:
        y = y + ab(o["emb"].to(dtype))[:, :, None, None]
    if o["res"] is not None:
        r = o["res"].to(dtype)
        y = y + ab(F.interpolate(r, scale_factor=2, mode="nearest") if c["res"] == 2 else r)
    if axpy_applied(c):
        s = torch.tensor(o["axpy_s"], dtype=torch.float32).to(dtype)
        y = ab(o["axpy_x"].to(dtype)) + (s.abs() if absval else s) * y
    return y


def reference(c, o):
    """-> dict(want, mag, f32, q, cabs) for the operands o of case c.  For the phase form the reference is this nine-tap conv as well."""
    W64 = o["W64"]
    qs = abs(o["axpy_s"]) if axpy_applied(c) else 1.0                 # the Euler update scales the conv's error with it
    r = dict(want=_compose(c, o, torch.float64, W64), mag=_compose(c, o, torch.float64, W64.abs(), absval=True),
             f32=_compose(c, o, torch.float32, W64.float()),
             q=_compose(c, o, torch.float64, W64, square=True, conv_only=True).sqrt() * qs,
             cabs=_compose(c, o, torch.float64, W64.abs(), absval=True, conv_only=True) if not c["pro"] else None,
             magpro=_compose(c, o, torch.float64, W64.abs(), absval="fma", conv_only=True) * qs if c["pro"] == "silu" else None)
    if phase_row(c):
        # The phase form's filter is round(sum of the fp32 taps), the reference's the sum of the rounded taps: a difference that is FIXED per weight, so
        # it does not average out of a channel's mean error.  The mean checks of a phase launch are therefore taken against fp64 on the filter the
        # kernel reads (phase_weights); the element-wise check stays against the nine-tap reference with the budget's phase term.
        r["want_phase"] = _compose(c, o, torch.float64, None, Wph=phase_weights(o["W"], o["dt"]))
    return r


def nhwc_out(c):
    return c["cout"] % 32 == 0


def budget(c, dt, r, phase=False):
    """The element-wise error bound of the module docstring.  phase: the launch ran the pre-summed (phase) filter."""
    want = r["want"]
    e32 = float((r["f32"].double() - want).abs().max())
    bud = 4 * e32 + C_SUM * U32 * r["mag"]
    if c["pro"] == "silu":
        bud = bud + K_FMA * U32 * r["magpro"]
    u = U16[dt]
    if u and nhwc_out(c):
        st = 1.01 * u * want.abs()
        bud = bud + (st.clamp_min(2.0 ** -25) if dt == "fp16" else st)
    if u and c["pro"] == "silu":
        bud = bud + 6.0 * u / math.sqrt(3.0) * r["q"]
    if phase:
        bud = bud + 1.01 * UW["bf16" if dt == "bf16x2" else dt] * r["cabs"]
    return bud, e32


def _ring(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def check(tag, c, dt, got, r, phase=False, log=print):
    """got [B, Co, Ho, Wo] against the reference r under the budget.  -> worst err / budget.  Raises AssertionError naming what failed."""
    got = got.detach().cpu().double()
    want = r["want"]
    assert got.shape == want.shape, f"{tag}: shape {tuple(got.shape)}, wanted {tuple(want.shape)}"
    assert torch.isfinite(got).all(), f"{tag}: {int((~torch.isfinite(got)).sum())} entries no kernel wrote (NaN)"
    bud, e32 = budget(c, dt, r, phase)
    err = got - want
    ratio = err.abs() / bud
    h, w = got.shape[2:]
    ring = _ring(h, w)
    r_ring = float(ratio[..., ring].max())
    r_in = float(ratio[..., ~ring].max()) if (~ring).any() else 0.0
    log(f"   FWDSTAT {tag}: fp32 eager err {e32:.3e} kernel err {float(err.abs().max()):.3e} worst err / budget ring {r_ring:.3f} interior {r_in:.3f}")
    assert r_ring <= 1.0, f"{tag}: border ring: err / budget {r_ring:.3f}"
    assert r_in <= 1.0, f"{tag}: interior: err / budget {r_in:.3f}"
    if U16[dt]:    # zero-mean: a truncating store, a bias shifted by a tile or a padding pixel that is always wrong shifts a channel's mean error
        n = got.shape[0] * h * w
        if phase:     # against fp64 on the pre-summed filter the kernel reads: the fixed weight difference is not part of these means
            err = got - r["want_phase"]
        rms = err.pow(2).mean(dim=(0, 2, 3)).sqrt()
        noise = 6.0 * rms / math.sqrt(n) + C_SUM * U32 * r["mag"].mean(dim=(0, 2, 3)) + 4 * e32
        if c["pro"] == "silu":
            noise = noise + K_FMA * U32 * r["magpro"].mean(dim=(0, 2, 3))
        m1 = err.mean(dim=(0, 2, 3)).abs()
        m2 = (err * want.sign()).mean(dim=(0, 2, 3)).abs()
        assert bool((m1 <= noise).all()), f"{tag}: mean error of channel {int((m1 - noise).argmax())}: {float((m1 / noise).max()):.2f} x 6 sigma"
        assert bool((m2 <= noise).all()), f"{tag}: mean signed error of channel {int((m2 - noise).argmax())}: {float((m2 / noise).max()):.2f} x 6 sigma"
    return max(r_ring, r_in)


# ---- what a correct 16-bit kernel computes, and three defects -------------------------------------------------------------------------------
def _trunc(t, dt):
    """t (fp32) rounded toward zero to the element type."""
    if T16[dt] == torch.bfloat16:
        return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    hlf = t.to(torch.float16)
    over = hlf.float().abs() > t.abs()
    bits = hlf.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(torch.float16).float()


def emulate16(c, dt, o, store="round", drop_tap=False, shift_bias=False, phase=False):
    """P rounded to the element type as the staging code does, products and sums in fp32, the NHWC store rounded (store = "trunc": toward zero).
    phase: the four pre-summed filters of the phase form (phase_weights: the fp32 taps summed, rounded once) instead of the nine rounded taps.
    drop_tap: tap (0, 0) of input channel 0 is missing; shift_bias: the bias of the next channel."""
    x = torch.cat([o["x"]] + ([o["x1"]] if o["x1"] is not None else []), dim=1)
    p = rnd(_pro(x, o, c, torch.float32), dt)
    if c["up"]:
        p = F.interpolate(p, scale_factor=2, mode="nearest")
    W = o["W"].clone() if phase else o["W64"].float().clone()
    if drop_tap:
        W[:, 0, 0, 0] = 0.0
    y = _phase_conv(p, phase_weights(W, dt)) if phase else F.conv2d(p, W, stride=c["s"], padding=c["k"] // 2)
    if o["bias"] is not None:
        y = y + (o["bias"].roll(1) if shift_bias else o["bias"])[None, :, None, None]
    if o["emb"] is not None:
        y = y + o["emb"][:, :, None, None]
    if o["res"] is not None:
        y = y + (F.interpolate(o["res"], scale_factor=2, mode="nearest") if c["res"] == 2 else o["res"])
    if axpy_applied(c):
        return o["axpy_x"] + torch.tensor(o["axpy_s"]) * y
    if not nhwc_out(c):
        return y
    return _trunc(y, dt) if store == "trunc" else rnd(y, dt)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
GEN = dict(conv_pp=0, conv_ws=0, conv_small=0, conv_edge=0)     # every switch to another family off (the stationary 1x1 tile has none)
CASES = []


def R(name, fam, form, B, cin, cout, h, w, k=3, s=1, up=0, c1=0, bias=1, pro=None, emb=0, res=0, nchw=0, axpy=0, types=ALL3, knobs=None, why=None):
    """One row.  fam / form: the kernel family and ConvRoute::form conv_route must report (form: a dict per type where the types differ); types: the
    element types the row runs in (why: the named reason where that is not fp32, bf16 and fp16); knobs: mi355_debug_config overrides."""
    assert all(n["name"] != name for n in CASES), name
    assert types == ALL3 or set(types) - set(ALL3) or why, f"{name}: a missing type needs its reason"
    CASES.append(dict(idx=len(CASES), name=name, fam=fam, form=form, B=B, cin=cin, c1=c1, cout=cout, h=h, w=w, k=k, s=s, up=up, bias=bias, pro=pro,
                      emb=emb, res=res, nchw=nchw, axpy=axpy, types=tuple(types), knobs=dict(knobs or {}), why=why))


X2 = ALL3 + ("bf16x2",)
mw = lambda n, **kw: dict(GEN, conv_min_wgs=n, **kw)
# -- generic implicit GEMM (conv_igemm.hip): every tile of launch_cfg through conv_min_wgs (compute_geo takes the first candidate of 128 x P, 64 x P,
#    64 x min(P, 64) with at least that many workgroups, else the last; P = conv_tile_n(Cout))
R("ig 128x128 64->128 16x16", K_IGEMM, 0, 2, 64, 128, 16, 16, knobs=mw(1), types=X2)
R("ig 128x64 64->64 16x16", K_IGEMM, 0, 2, 64, 64, 16, 16, knobs=mw(1))
R("ig 128x32 64->32 16x16", K_IGEMM, 0, 2, 64, 32, 16, 16, knobs=mw(1))
R("ig 64x128 64->128 16x16", K_IGEMM, 0, 2, 64, 128, 16, 16, knobs=mw(8))
R("ig 64x64 64->128 16x16", K_IGEMM, 0, 2, 64, 128, 16, 16, knobs=mw(512))
R("ig 64x32 64->32 16x16", K_IGEMM, 0, 2, 64, 32, 16, 16, knobs=mw(512))
# several images per 64-pixel tile (4x4: four; the odd batch leaves the last tile partly empty), 7x7 and 8x8 (one image, a partly empty / a full tile)
R("ig 4x4 B9 32->32", K_IGEMM, 0, 9, 32, 32, 4, 4, knobs=mw(512))
R("ig 4x4 B5 64->128 emb", K_IGEMM, 0, 5, 64, 128, 4, 4, emb=1, knobs=mw(512))
R("ig 7x7 B3 64->64", K_IGEMM, 0, 3, 64, 64, 7, 7, knobs=mw(512))
R("ig 8x8 B3 96->32", K_IGEMM, 0, 3, 96, 32, 8, 8, knobs=mw(512))
# ks 1 (an NHWC 1x1 conv with Cout % 128 == 0 always goes to the stationary tile: 64 and 96 output channels stay here), split weights
R("ig 1x1 96->64 8x8", K_IGEMM, 0, 2, 96, 64, 8, 8, k=1, knobs=mw(512), types=X2)
R("ig 1x1 64->96 14x14 affine", K_IGEMM, 0, 2, 64, 96, 14, 14, k=1, pro="affine", knobs=mw(512))
R("ig 1x1 64+32->64 8x8", K_IGEMM, 0, 3, 64, 64, 8, 8, k=1, c1=32, emb=1, res=1, knobs=mw(512))
# stride 2: the 64-pixel tile's 17 x 17 patch (PIT 7) and the 128-pixel tile's 33 x 17 one (PIT 11); odd and even inputs
R("ig s2 64->64 16x16", K_IGEMM, 0, 2, 64, 64, 16, 16, s=2, knobs=mw(512), types=X2)
R("ig s2 32->32 7x7", K_IGEMM, 0, 2, 32, 32, 7, 7, s=2, knobs=mw(512))
R("ig s2 32->64 8x6", K_IGEMM, 0, 3, 32, 64, 8, 6, s=2, knobs=mw(512))
R("ig s2 64->128 32x32 128-tile", K_IGEMM, 0, 1, 64, 128, 32, 32, s=2, knobs=mw(1))
# nearest x2 in the gather
R("ig up 64->64 4x4", K_IGEMM, 0, 2, 64, 64, 4, 4, up=1, knobs=mw(512))
R("ig up 64->64 8x8 silu", K_IGEMM, 0, 2, 64, 64, 8, 8, up=1, pro="silu", emb=1, knobs=mw(512))
# two sources
R("ig cat 64+32->64 8x8", K_IGEMM, 0, 2, 64, 64, 8, 8, c1=32, knobs=mw(512))
R("ig cat 32+96->64 8x8 silu", K_IGEMM, 0, 2, 32, 64, 8, 8, c1=96, pro="silu", knobs=mw(512))
R("ig cat 128+128->128 8x8", K_IGEMM, 0, 2, 128, 128, 8, 8, c1=128, knobs=mw(512))
# prologues, ragged images, the epilogue terms
R("ig 64->64 20x28 silu", K_IGEMM, 0, 1, 64, 64, 20, 28, pro="silu", knobs=mw(512), types=X2)
R("ig 64->64 14x14 affine", K_IGEMM, 0, 2, 64, 64, 14, 14, pro="affine", knobs=mw(512))
R("ig 128->128 14x14 silu emb", K_IGEMM, 0, 2, 128, 128, 14, 14, pro="silu", emb=1, knobs=mw(1))
R("ig 64->64 14x14 res", K_IGEMM, 0, 2, 64, 64, 14, 14, res=1, knobs=mw(512))
R("ig 64->64 20x28 silu res up2", K_IGEMM, 0, 1, 64, 64, 20, 28, pro="silu", res=2, emb=1, knobs=mw(1))
# the out conv (NCHW fp32 output, Cout 1 .. 4) and the first conv (1, 3, 6, 8 real channels of a chunk) on this kernel
for co in (1, 2, 3, 4):
    R(f"ig out 128->{co} 16x16", K_IGEMM, 0, 2, 128, co, 16, 16, pro="silu", knobs=mw(512))
R("ig out 64->3 20x28 no pro", K_IGEMM, 0, 1, 64, 3, 20, 28, knobs=mw(512))
for ci in (1, 3, 6, 8):
    R(f"ig first {ci}->128 16x16", K_IGEMM, 0, 2, ci, 128, 16, 16, knobs=mw(512))
# -- 1x1 with a stationary activation tile (conv1x1.hip)
P0 = dict(conv_pp=0)
R("1x1 qkv 128->384 8x8", K_1X1, 0, 2, 128, 384, 8, 8, k=1, knobs=P0)
R("1x1 qkv 128->384 8x8 affine", K_1X1, 0, 3, 128, 384, 8, 8, k=1, pro="affine", knobs=P0)
R("1x1 qkv 128->384 16x16", K_1X1, 0, 2, 128, 384, 16, 16, k=1, knobs=P0)
R("1x1 qkv 128->384 16x16 affine", K_1X1, 0, 1, 128, 384, 16, 16, k=1, pro="affine", knobs=P0)
R("1x1 256->128 8x8 res", K_1X1, 0, 2, 256, 128, 8, 8, k=1, res=1, knobs=P0)
R("1x1 cat 128+128->128 8x8 emb", K_1X1, 0, 3, 128, 128, 8, 8, k=1, c1=128, emb=1, knobs=P0)
# -- 1x1 ping-pong (conv_pp1.hip): form 1 = 256 x 256, 0 = 512 x 128, 2 = 128 x 256 tiles (conv_pp bit 5); at least eight chunks in fours
R("pp1 256x256 256->256 16x16", K_1X1_PP, 1, 1, 256, 256, 16, 16, k=1, knobs=dict(conv_pp=2))
R("pp1 512x128 256->128 32x16", K_1X1_PP, 0, 1, 256, 128, 32, 16, k=1, knobs=dict(conv_pp=2))
R("pp1 512x128 256->384 32x16 emb res", K_1X1_PP, 0, 2, 256, 384, 32, 16, k=1, emb=1, res=1, knobs=dict(conv_pp=2))
R("pp1 128x256 256->256 16x16", K_1X1_PP, 2, 2, 256, 256, 16, 16, k=1, knobs=dict(conv_pp=34))
R("pp1 128x256 256->512 16x16 res", K_1X1_PP, 2, 1, 256, 512, 16, 16, k=1, res=1, knobs=dict(conv_pp=34))
R("pp1 256x256 cat 96+160->256 16x16 emb", K_1X1_PP, 1, 2, 96, 256, 16, 16, k=1, c1=160, emb=1, knobs=dict(conv_pp=2),
  types=H16, why="96 + 160 channels are 3 + 5 chunks in the 16-bit types: the source boundary falls mid-stream")
R("pp1 256x256 cat 48+80->256 16x16 emb", K_1X1_PP, 1, 2, 48, 256, 16, 16, k=1, c1=80, emb=1, knobs=dict(conv_pp=2),
  types=("fp32",), why="48 + 80 channels are 3 + 5 chunks in fp32 only (the 16-bit types need whole 32-channel chunks)")
# -- the first conv (conv_edge.hip conv3x3_in_kernel; no fp32 instantiation: conv_in_route declines DT_F32)
NOF32 = "conv3x3_in_kernel has no fp32 instantiation"
for ci in (1, 3, 6, 8):
    R(f"in {ci}->128 16x16", K_IN, 0, 2, ci, 128, 16, 16, types=H16, why=NOF32)
    R(f"in {ci}->128 48x16", K_IN, 0, 2, ci, 128, 48, 16, types=H16, why=NOF32)
R("in nchw 3->128 16x16", K_IN, 0, 2, 3, 128, 16, 16, nchw=1, types=H16, why=NOF32)
R("in nchw 3+3->128 48x16", K_IN, 0, 2, 3, 128, 48, 16, c1=3, nchw=1, types=H16, why=NOF32)
R("in nchw 1+1->128 16x16", K_IN, 0, 3, 1, 128, 16, 16, c1=1, nchw=1, types=H16, why=NOF32)
R("in nchw off 3+3->128 16x16", K_IN, 0, 2, 3, 128, 16, 16, c1=3, nchw=1, types=H16, why=NOF32, knobs=dict(conv_edge=11))   # bit 2 off: the packed copy of x | cond
R("ig nchw 3+3->128 16x16", K_IGEMM, 0, 2, 3, 128, 16, 16, c1=3, nchw=1, knobs=mw(512))
# -- the last conv (conv_edge.hip conv3x3_out_kernel): form 1 = FIXED (16 fragments per pixel: 64 fp32 / 128 16-bit channels), 0 = counted
BIG32 = "256 fp32 channels: the staged patch exceeds the 160 KB of LDS (conv_out_route declines); fp32 admits 64 and 128"
R("out 64->3 16x16", K_OUT, 1, 2, 64, 3, 16, 16, pro="silu", types=("fp32",), why="64 channels are half a swizzle group in the 16-bit types")
R("out 128->3 16x16", K_OUT, dict(fp32=0, bf16=1, fp16=1), 2, 128, 3, 16, 16, pro="silu")
R("out 128->1 20x28", K_OUT, dict(fp32=0, bf16=1, fp16=1), 1, 128, 1, 20, 28, pro="silu")
R("out 128->2 16x16 affine", K_OUT, dict(fp32=0, bf16=1, fp16=1), 3, 128, 2, 16, 16, pro="affine")
R("out 256->4 16x16", K_OUT, 0, 2, 256, 4, 16, 16, pro="silu", types=H16, why=BIG32)
R("out 256->3 20x28", K_OUT, 0, 1, 256, 3, 20, 28, pro="silu", types=H16, why=BIG32)
R("out 128->3 16x16 axpy", K_OUT, dict(fp32=0, bf16=1, fp16=1), 2, 128, 3, 16, 16, pro="silu", axpy=1)
R("out 256->3 20x28 axpy", K_OUT, 0, 1, 256, 3, 20, 28, pro="silu", axpy=1, types=H16, why=BIG32)
R("out 128->4 20x28 axpy", K_OUT, dict(fp32=0, bf16=1, fp16=1), 1, 128, 4, 20, 28, pro="silu", axpy=1)
R("out 128->3 16x16 axpy off", K_OUT, dict(fp32=0, bf16=1, fp16=1), 2, 128, 3, 16, 16, pro="silu", axpy=1, knobs=dict(conv_edge=7))
# -- ping-pong 3x3 (conv_pp.hip): form 0 wide (Cout % 256 == 0), 1 narrow (Cout % 128 == 0, Wo >= 32), 2 wide in phase form
PP = dict(conv_pp=2 | 4 | 8 | 16 | 64, conv_ws=0, conv_small=0)
R("pp wide 64->256 16x16", K_PP, 0, 1, 64, 256, 16, 16, knobs=PP)
R("pp wide 128->256 20x20", K_PP, 0, 2, 128, 256, 20, 20, knobs=PP)
R("pp wide 192->256 16x16 emb res", K_PP, 0, 2, 192, 256, 16, 16, emb=1, res=1, knobs=PP)
R("pp wide 32->256 16x16", K_PP, 0, 1, 32, 256, 16, 16, knobs=PP, types=("fp32",), why="32 channels are two chunks in fp32, one (no chunk pair) in the 16-bit types")
R("pp wide 96->256 20x20", K_PP, 0, 1, 96, 256, 20, 20, knobs=PP, types=("fp32",), why="96 channels are six chunks in fp32, three (odd) in the 16-bit types")
R("pp wide silu 128->256 16x16", K_PP, 0, 1, 128, 256, 16, 16, pro="silu", knobs=PP)
R("pp wide silu 192->256 28x28 emb", K_PP, 0, 1, 192, 256, 28, 28, pro="silu", emb=1, knobs=PP)
R("pp wide cat 32+96->256 16x16", K_PP, 0, 2, 32, 256, 16, 16, c1=96, knobs=PP)
R("pp wide cat 48+80->256 16x16 silu", K_PP, 0, 1, 48, 256, 16, 16, c1=80, pro="silu", knobs=PP, types=("fp32",),
  why="48 + 80 channels are 3 + 5 chunks in fp32 only: the source switch falls inside a chunk pair")
R("pp wide silu 128->256 16x16 res up2", K_PP, 0, 2, 128, 256, 16, 16, pro="silu", res=2, knobs=PP)
R("pp wide up 128->256 8x8", K_PP, 0, 2, 128, 256, 8, 8, up=1, knobs=dict(PP, conv_pp=30))
R("pp wide up silu 64->256 10x10", K_PP, 0, 1, 64, 256, 10, 10, up=1, pro="silu", knobs=PP)
R("pp narrow 64->128 16x32", K_PP, 1, 1, 64, 128, 16, 32, knobs=PP)
R("pp narrow 128->128 20x36 emb res", K_PP, 1, 1, 128, 128, 20, 36, emb=1, res=1, knobs=PP)
R("pp narrow silu 192->128 16x32", K_PP, 1, 1, 192, 128, 16, 32, pro="silu", knobs=PP)
R("pp narrow silu 64->384 20x36", K_PP, 1, 1, 64, 384, 20, 36, pro="silu", knobs=PP)
R("pp phase 64->256 16x16", K_PP, 2, 1, 64, 256, 16, 16, up=1, knobs=PP)
R("pp phase 128->256 20x20 emb", K_PP, 2, 1, 128, 256, 20, 20, up=1, emb=1, knobs=PP)
R("pp phase 192->512 16x16", K_PP, 2, 1, 192, 512, 16, 16, up=1, knobs=PP)
# -- warp-specialised 3x3 (conv_ws.hip): the plain tile must be 128 x 128 (conv_min_wgs = 1); bit 2 takes launches of fewer tiles than CUs
WS = dict(conv_min_wgs=1, conv_ws=5, conv_pp=0, conv_small=0)
R("ws 64->128 16x16", K_WS, 0, 1, 64, 128, 16, 16, knobs=WS)
R("ws 128->128 20x20 emb", K_WS, 0, 2, 128, 128, 20, 20, emb=1, knobs=WS)
R("ws silu 128->128 16x16", K_WS, 0, 1, 128, 128, 16, 16, pro="silu", knobs=WS)
R("ws silu 64->128 28x28 res", K_WS, 0, 1, 64, 128, 28, 28, pro="silu", res=1, knobs=WS)
R("ws affine 64->128 16x16", K_WS, 0, 2, 64, 128, 16, 16, pro="affine", knobs=WS)
R("ws cat 64+64->128 16x16", K_WS, 0, 2, 64, 128, 16, 16, c1=64, knobs=WS)
R("ws cat 32+96->128 20x20 silu", K_WS, 0, 1, 32, 128, 20, 20, c1=96, pro="silu", knobs=WS)
R("ws up 64->128 8x8", K_WS, 0, 2, 64, 128, 8, 8, up=1, knobs=WS)
R("ws up silu 128->128 10x10 emb", K_WS, 0, 1, 128, 128, 10, 10, up=1, pro="silu", emb=1, knobs=WS)
R("ws silu 128->128 16x16 res up2", K_WS, 0, 2, 128, 128, 16, 16, pro="silu", res=2, knobs=WS)
R("ws 64->256 16x16 two channel tiles", K_WS, 0, 1, 64, 256, 16, 16, knobs=WS)
R("ws 64->128 32x32 B2 two workgroups", K_WS, 0, 2, 64, 128, 32, 32, knobs=dict(WS, conv_ws=5 | (2 << 8)))
R("ws silu 128->256 32x32 B2 two workgroups", K_WS, 0, 2, 128, 256, 32, 32, pro="silu", emb=1, knobs=dict(WS, conv_ws=5 | (2 << 8)))
# -- small-level 3x3 (conv_small.hip): 8x8 / 4x4 outputs; the K split over 4 / 2 / 1 waves follows the launch size (a workgroup per CU: unsplit)
SM = dict(conv_small=15, conv_pp=0, conv_ws=0)
R("small 8x8 128->128 B2", K_SMALL, 0, 2, 128, 128, 8, 8, knobs=SM)
R("small 8x8 128->256 B3 emb res", K_SMALL, 0, 3, 128, 256, 8, 8, emb=1, res=1, knobs=SM)
R("small 8x8 cat 64+64->128", K_SMALL, 0, 2, 64, 128, 8, 8, c1=64, knobs=SM)
R("small 8x8 64->256 B128 ksplit 2", K_SMALL, 0, 128, 64, 256, 8, 8, knobs=SM)
R("small 8x8 32->256 B256 eight waves", K_SMALL, 1, 256, 32, 256, 8, 8, knobs=SM)
R("small 8x8 32->256 B256 unsplit", K_SMALL, 0, 256, 32, 256, 8, 8, knobs=dict(SM, conv_small=13))
R("small 4x4 128->128 B5", K_SMALL, 0, 5, 128, 128, 4, 4, knobs=SM)
R("small 4x4 128->256 B2 emb res", K_SMALL, 0, 2, 128, 256, 4, 4, emb=1, res=1, knobs=SM)
R("small 4x4 64->256 B512 ksplit 2", K_SMALL, 0, 512, 64, 256, 4, 4, knobs=SM)
R("small 4x4 32->256 B1024 unsplit", K_SMALL, 0, 1024, 32, 256, 4, 4, knobs=SM)
R("small 4x4 256->128 two K phases", K_SMALL, 0, 3, 256, 128, 4, 4, knobs=SM, types=("fp32",), why="256 channels are 16 chunks (two phases of 8) in fp32, 8 (one phase) in the 16-bit types")
R("small 4x4 512->128 two K phases", K_SMALL, 0, 3, 512, 128, 4, 4, knobs=SM, types=H16, why="512 channels are 16 chunks (two phases of 8) in the 16-bit types")
R("small s2 128->128 16->8", K_SMALL, 0, 2, 128, 128, 16, 16, s=2, knobs=SM)
R("small s2 128->128 8->4 B5", K_SMALL, 0, 5, 128, 128, 8, 8, s=2, knobs=SM)
R("small up 128->128 4->8", K_SMALL, 0, 2, 128, 128, 4, 4, up=1, emb=1, knobs=SM)

# The remaining route words per row: (tile pixels, tile channels, reads_nchw, axpy, ksplit), the same in every element type of the row.  The tile is
# ConvRoute::geom's: the ping-pong and warp-specialised kernels' own, else the plain tiling compute_geo worked out (64 x 64 where no row is listed).
EXPECT_DEFAULT = (64, 64, 0, 0, 0)
EXPECT = {
    "ig 128x128 64->128 16x16": (128, 128, 0, 0, 0), "ig 128x64 64->64 16x16": (128, 64, 0, 0, 0), "ig 128x32 64->32 16x16": (128, 32, 0, 0, 0),
    "ig 64x128 64->128 16x16": (64, 128, 0, 0, 0), "ig 64x32 64->32 16x16": (64, 32, 0, 0, 0), "ig 4x4 B9 32->32": (64, 32, 0, 0, 0),
    "ig 8x8 B3 96->32": (64, 32, 0, 0, 0), "ig 1x1 64->96 14x14 affine": (64, 32, 0, 0, 0), "ig s2 32->32 7x7": (64, 32, 0, 0, 0),
    "ig s2 64->128 32x32 128-tile": (128, 128, 0, 0, 0), "ig 128->128 14x14 silu emb": (128, 128, 0, 0, 0),
    "ig 64->64 20x28 silu res up2": (128, 64, 0, 0, 0),
    "ig out 128->1 16x16": (64, 32, 0, 0, 0), "ig out 128->2 16x16": (64, 32, 0, 0, 0), "ig out 128->3 16x16": (64, 32, 0, 0, 0),
    "ig out 128->4 16x16": (64, 32, 0, 0, 0), "ig out 64->3 20x28 no pro": (64, 32, 0, 0, 0),
    "in nchw 3->128 16x16": (64, 64, 1, 0, 0), "in nchw 3+3->128 48x16": (64, 64, 1, 0, 0), "in nchw 1+1->128 16x16": (64, 64, 1, 0, 0),
    "out 64->3 16x16": (64, 32, 0, 0, 0), "out 128->3 16x16": (64, 32, 0, 0, 0), "out 128->1 20x28": (64, 32, 0, 0, 0),
    "out 128->2 16x16 affine": (64, 32, 0, 0, 0), "out 256->4 16x16": (64, 32, 0, 0, 0), "out 256->3 20x28": (64, 32, 0, 0, 0),
    "out 128->3 16x16 axpy": (64, 32, 0, 1, 0), "out 256->3 20x28 axpy": (64, 32, 0, 1, 0), "out 128->4 20x28 axpy": (64, 32, 0, 1, 0),
    "out 128->3 16x16 axpy off": (64, 32, 0, 0, 0),
    "small 8x8 128->128 B2": (64, 64, 0, 0, 4), "small 8x8 128->256 B3 emb res": (64, 64, 0, 0, 4), "small 8x8 cat 64+64->128": (64, 64, 0, 0, 4),
    "small 8x8 64->256 B128 ksplit 2": (64, 64, 0, 0, 2), "small 8x8 32->256 B256 eight waves": (64, 128, 0, 0, 1),
    "small 8x8 32->256 B256 unsplit": (64, 128, 0, 0, 1), "small 4x4 128->128 B5": (64, 64, 0, 0, 4),
    "small 4x4 128->256 B2 emb res": (64, 64, 0, 0, 4), "small 4x4 64->256 B512 ksplit 2": (64, 64, 0, 0, 2),
    "small 4x4 32->256 B1024 unsplit": (64, 128, 0, 0, 1), "small 4x4 256->128 two K phases": (64, 64, 0, 0, 4),
    "small 4x4 512->128 two K phases": (64, 64, 0, 0, 4), "small s2 128->128 16->8": (64, 64, 0, 0, 4),
    "small s2 128->128 8->4 B5": (64, 64, 0, 0, 4), "small up 128->128 4->8": (64, 64, 0, 0, 4),
}
for _c in CASES:     # the ping-pong 3x3 and warp-specialised tiles follow from the form
    if _c["fam"] == K_PP:
        EXPECT[_c["name"]] = (512, 128, 0, 0, 0) if _c["form"] == 1 else (256, 256, 0, 0, 0)
    elif _c["fam"] == K_WS:
        EXPECT[_c["name"]] = (256, 128, 0, 0, 0)
assert set(EXPECT) <= {_c["name"] for _c in CASES}


def want_route(c, dt):
    tm, tn, rn, ax, ks = EXPECT.get(c["name"], EXPECT_DEFAULT)
    return dict(kernel=c["fam"], form=want_form(c, dt), tile_m=tm, tile_n=tn, reads_nchw=rn, axpy=ax, ksplit=ks)


# ConvRoute::form values the route functions can produce, per family: every one must be reached in every element type that has the family
WANT_FORMS = {K_IGEMM: {0}, K_1X1: {0}, K_1X1_PP: {0, 1, 2}, K_IN: {0}, K_OUT: {0, 1}, K_PP: {0, 1, 2}, K_WS: {0}, K_SMALL: {0, 1}}
# the named exceptions: families without an instantiation in a type
NO_FAMILY = {"fp32": {K_IN}, "bf16": set(), "fp16": set()}


def want_pairs(dt):
    return {(k, f) for k, fs in WANT_FORMS.items() if k not in NO_FAMILY[dt] for f in fs}


def want_form(c, dt):
    return c["form"][dt] if isinstance(c["form"], dict) else c["form"]


def route_query(ops, c, dt):
    """conv_route for the row, without a GPU (mi355_conv2d_fwd's route query)."""
    from mi355 import _lib

    return ops.conv2d_fwd_route(c["B"], c["cin"], c["cout"], c["h"], c["w"], c["k"], stride=c["s"], resample=2 if c["up"] else 0, Cin1=c["c1"],
                                bias=bool(c["bias"]), pro=bool(c["pro"]), pro_silu=c["pro"] == "silu", emb=bool(c["emb"]), res_mode=c["res"],
                                nchw_src=bool(c["nchw"]), axpy=bool(c["axpy"]), dtype=dtype_code(dt), debug=_lib.debug_config(**c["knobs"]))


_DATA = {}


def case_data(idx, dt):
    """(operands, reference) of row idx in type dt, computed once per process and shared by every test that needs it (left unchanged by them)."""
    if (idx, dt) not in _DATA:
        o = operands(CASES[idx], dt)
        _DATA[(idx, dt)] = (o, reference(CASES[idx], o))
    return _DATA[(idx, dt)]


def case_id(c):
    return c["name"].replace("->", "_to_").replace(" ", "_").replace("+", "p")
