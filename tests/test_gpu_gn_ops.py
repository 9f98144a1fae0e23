"""GPU: every GroupNorm32 kernel the network launches, op by op, against plain fp64 torch on the CPU.

  gn_affine_kernel (csrc/gn_stats.hip)          mi355_gn_affine    statistics -> (a, b), mean, rstd, optional silu?(a x + b); five template forms
  conv epilogue partial sums + gn_finalize      mi355_conv2d_gn    one run per conv route that fills statistics slots, and the two-producer form
  affine_pool_kernel                            mi355_affine_pool  AvgPool2d(2)(silu?(a x + b))
  gn_silu_bwd_kernel (csrc/backward.hip)        mi355_gn_silu_vjp  against fp64 autograd
  grad_gather_kernel                            mi355_grad_gather  against fp64 autograd of nearest x2, AvgPool2d(2), a stride-2 identity conv

References, input classes and the forward budget (4 x the fp32 eager reference's own error, per class of |mean| / std) are those of
tests/test_gn_ref_cpu.py, which proves on the CPU that the reference passes them and that single-pass E[x^2] - mean^2 sums do not.
For 16-bit element types the input is rounded to the type first: the reference sees exactly the values the kernel reads.

Measured on the MI355X (worst error / e_ref over the cases below; DESIGN.md "GroupNorm statistics: measured error" has the table):
the kernels before the pivoted sums failed every r16 / r64 / near class; the present ones pass every class.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from mi355 import _lib
from mi355.synth import randn
from tests.test_gn_ref_cpu import (CLASS_NAMES, EPS, GROUPS, ULP32, apply_ab, check_ab, check_stats, gn64, make_input, make_params, stats64)

DEV = "cuda:0"
F32, BF16, F16 = _lib.MI355_F32, _lib.MI355_BF16, _lib.MI355_F16
TORCH16 = {BF16: torch.bfloat16, F16: torch.float16}
U16 = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}     # unit roundoff (half an ulp, relative) of a store: 8 / 11 significand bits
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


def dev(t):
    return t.to(DEV) if t is not None else None


def silu64(v):
    return v * torch.sigmoid(v)


# (C0, C1, HW, B, expected form) per element size.  fp32: 4 channels per 16-byte fragment, 16-bit: 8; NL = HW * (C / V) / 512 when that is
# 1, 2, 4 or 8 and C / V divides 512, else 0.
AFFINE_CASES = {
    4: [(96, 0, 49, 2, 0), (160, 0, 196, 2, 0), (96, 0, 16, 3, 0), (160, 0, 64, 1, 0),                  # C / V = 24, 40: idle lane rows
        (128, 0, 16, 3, 1), (256, 0, 16, 2, 2), (128, 0, 64, 2, 4), (256, 0, 64, 2, 8),                 # the register forms
        (640, 0, 64, 1, 0), (1024, 0, 16, 1, 8), (1024, 0, 49, 1, 0), (1024, 512, 16, 1, 0),            # C > 512: the c += 512 sweeps
        (256, 128, 64, 2, 0), (256, 128, 196, 1, 0), (64, 32, 64, 2, 0), (64, 32, 16, 2, 0),            # groups of 12 / 3 straddle the sources
        (128, 0, 784, 1, 0), (128, 0, 1024, 1, 0), (128, 0, 4096, 1, 0), (32, 0, 16, 2, 0),             # large images; more lane rows than pixels
        (64, 0, 16, 300, 0), (128, 0, 64, 300, 4)],                                                     # a batch of a few hundred
    2: [(192, 0, 49, 2, 0), (320, 0, 196, 1, 0), (192, 0, 16, 3, 0), (320, 0, 64, 1, 0),                # C / V = 24, 40
        (256, 0, 16, 3, 1), (512, 0, 16, 2, 2), (256, 0, 64, 2, 4), (512, 0, 64, 2, 8),
        (640, 0, 64, 1, 0), (1024, 0, 16, 1, 4), (1024, 512, 64, 1, 0), (1024, 512, 16, 1, 0),
        (256, 128, 64, 2, 0), (256, 128, 196, 1, 0), (64, 32, 64, 2, 0),                                # 256 + 128: one 8-channel fragment spans two groups
        (128, 0, 784, 1, 0), (128, 0, 1024, 1, 0), (128, 0, 4096, 1, 0), (64, 0, 16, 2, 0),
        (64, 0, 16, 300, 0), (256, 0, 64, 300, 4)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_gn_affine_vs_fp64(ops, dtype):
    """a, b per channel, mean and rstd per group, and the apply output, for every case x FiLM on / off x apply affine / SiLU."""
    forms = set()
    worst = {}
    for ci, (C0, C1, HW, B, want_form) in enumerate(AFFINE_CASES[4 if dtype == F32 else 2]):
        C = C0 + C1
        x = make_input(41000 + 13 * ci, B, C, HW, dtype=TORCH16.get(dtype))
        xs = (x[:, :C0].contiguous(), x[:, C0:].contiguous() if C1 else None)
        for film_on in (False, True):
            gamma, beta, film = make_params(42000 + ci, B, C, film_on)
            for apply in ("silu", "affine"):
                tag = f"{NAME[dtype]} C={C0}+{C1} HW={HW} B={B} film={film_on} apply={apply}"
                r = ops.gn_affine(dev(xs[0]), dev(gamma), dev(beta), x1=dev(xs[1]), film=dev(film), dtype=dtype, apply=apply)
                forms.add(r["form"])
                assert r["form"] == want_form, f"{tag}: form NL={r['form']}, expected {want_form}"
                a, b, y = r["a"].cpu(), r["b"].cpu(), r["y"].cpu()
                assert torch.isfinite(a).all() and torch.isfinite(b).all() and torch.isfinite(y).all(), f"{tag}: unwritten (NaN) outputs"
                res = check_ab(a, b, x, gamma, beta, film, tag, report=print)
                for k, (e, err, bud) in res.items():
                    w = worst.setdefault(k, [0.0, 0.0, 0.0])
                    w[0], w[1], w[2] = max(w[0], e), max(w[1], err), max(w[2], err / max(e, 1e-30) if k != "const" else 0.0)
                check_stats(r["mean"].cpu(), r["rstd"].cpu(), x, tag)
                # an exactly constant group: var = 0, rstd = 1 / sqrt(eps)
                for g in range(GROUPS):
                    if CLASS_NAMES[g % len(CLASS_NAMES)] == "const":
                        got = r["rstd"].cpu()[:, g].double()
                        assert float((got * math.sqrt(EPS) - 1).abs().max()) < 4 * ULP32, f"{tag}: rstd of the constant group {g}"
                # the apply pass, against the kernel's own (a, b): fp32 fma + SiLU, then the store's rounding
                v = apply_ab(a, b, x)
                want = silu64(v) if apply == "silu" else v
                sh = a.shape + (1,)
                mag = (a.double().abs().reshape(sh) * x.double().abs() + b.double().abs().reshape(sh))
                tol = 4 * 2.0 ** -24 * mag + 2e-6 * (1 + v.abs()) + 1.01 * U16[dtype] * want.abs() + (2.0 ** -24 if dtype == F16 else 0.0)
                bad = ((y.double() - want).abs() - tol).max()
                assert float(bad) <= 0, f"{tag}: apply output off by {float(bad):.3e} beyond its tolerance"
    print(f"   GNSUM gn_affine {NAME[dtype]} forms {sorted(forms)}: " + " ".join(f"{k}: e_ref {w[0]:.2e} err {w[1]:.2e} ratio {w[2]:.2f};" for k, w in worst.items()))
    assert forms == {0, 1, 2, 4, 8}, f"template forms reached: {sorted(forms)}"


# ---- the partial-sum path ---------------------------------------------------------------------------------------------------------------
K_IGEMM, K_1X1, K_1X1_PP, K_IN, K_PP, K_WS = 0, 1, 2, 3, 5, 6
# name, B, Cin, Cout, H, W, ksize, stride, debug knobs, kernels accepted, 16-bit only
ROUTE_CASES = [
    ("igemm 28x28", 6, 128, 128, 28, 28, 3, 1, dict(conv_ws=0, conv_pp=0), {K_IGEMM}, False),
    ("igemm 20x28", 3, 128, 256, 20, 28, 3, 1, dict(conv_ws=0, conv_pp=0), {K_IGEMM}, False),
    ("igemm stride 2", 8, 128, 128, 32, 32, 3, 2, dict(conv_ws=0, conv_pp=0), {K_IGEMM}, False),
    ("igemm 16x16", 9, 128, 256, 16, 16, 3, 1, dict(conv_ws=0, conv_pp=0), {K_IGEMM}, False),
    # (conv_min_wgs: the plain geometry keeps its 128 x 128 tile at this batch, which the persistent kernel requires; it then needs a tile per CU)
    ("warp-specialised 28x28", 64, 128, 128, 28, 28, 3, 1, dict(conv_pp=0, conv_min_wgs=64), {K_WS}, False),
    ("warp-specialised 20x28", 70, 128, 128, 20, 28, 3, 1, dict(conv_pp=0, conv_min_wgs=64), {K_WS}, False),
    ("ping-pong wide 28x28", 10, 128, 256, 28, 28, 3, 1, dict(conv_pp=2), {K_PP}, False),
    ("ping-pong wide 20x28", 3, 128, 256, 20, 28, 3, 1, dict(conv_pp=2), {K_PP}, False),
    ("ping-pong narrow 40x40", 5, 128, 128, 40, 40, 3, 1, dict(conv_pp=30), {K_PP}, False),
    ("1x1 16x16", 6, 128, 256, 16, 16, 1, 1, dict(conv_pp=0), {K_1X1}, False),
    ("1x1 20x28", 5, 128, 128, 20, 28, 1, 1, dict(conv_pp=0), {K_1X1}, False),
    ("1x1 ping-pong 16x16", 6, 256, 256, 16, 16, 1, 1, dict(conv_pp=2), {K_1X1_PP}, False),
    ("1x1 ping-pong 32x32", 5, 256, 128, 32, 32, 1, 1, dict(conv_pp=2), {K_1X1_PP}, False),
    ("first conv 32x32", 4, 3, 128, 32, 32, 3, 1, dict(), {K_IN}, True),
]
CONV_CLASSES = 5   # |mean| / std = 0, 1, 4, 16, 64, produced through the conv's bias


def conv_weights(seed, Co, Ci, k):
    """Output of std ~1 for unit-variance input."""
    return randn(seed, Co, Ci, k, k) / math.sqrt(Ci * k * k)


def class_bias(seed, Co, C_total, coff):
    """Group g of the C_total-channel GroupNorm gets class g % 5 (sign alternating), each channel a jitter of its own."""
    cpg = C_total // GROUPS
    ratios = (0.0, 1.0, 4.0, 16.0, 64.0)
    b = randn(seed, Co) * 0.2
    for c in range(Co):
        g = (coff + c) // cpg
        b[c] += (-1.0 if g % 2 else 1.0) * ratios[g % CONV_CLASSES]
    return b


def rounding_gap(dtype, y, gamma, beta, film):
    """Additional budget of the partial-sum path in a 16-bit element type.  The epilogue sums the fp32 accumulators v; the reference
    normalises the stored tensor fl(v) = v + e, |e_i| <= u |v_i|, u = the type's unit roundoff.  With n elements per group, rms(v)^2 =
    sigma^2 (1 + r^2), r = |mean| / sigma, and the e_i independent, zero-mean, of variance <= u^2 v_i^2 / 3:
        |mean(fl v) - mean(v)|      <= 6 u sigma sqrt((1 + r^2) / (3 n))                         (six standard deviations of a mean of n)
        |var(fl v) - var(v)|        <= 2 |cov(v, e)| + var(e) <= 12 u sigma^2 sqrt((1 + r^2) / (3 n)) + u^2 sigma^2 (1 + r^2)
    and y = gamma_eff (x - mean) rstd moves by |gamma_eff| (dmean / sigma + |xhat| dvar / (2 sigma^2)):
        gap = |gamma_eff| [ 6 u sqrt((1 + r^2) / (3 n)) (1 + |xhat|) + u^2 (1 + r^2) |xhat| / 2 ].
    Evaluated per class with the largest r, |xhat| and |gamma_eff| of the class; zero in fp32."""
    u = U16[dtype]
    B, C = y.shape[:2]
    n = (C // GROUPS) * y[0, 0].numel()
    m, v = stats64(y)
    r2 = (m * m / (v + EPS))                                                    # [B, 32]
    xh = ((y.double().reshape(B, GROUPS, -1) - m[:, :, None]) / torch.sqrt(v + EPS)[:, :, None]).abs().amax(dim=2)
    geff = gamma.double()[None, :] * (1 + (film[:, :C].double() if film is not None else 0.0))
    geff = geff.abs().expand(B, C).reshape(B, GROUPS, -1).amax(dim=2)
    gap = geff * (6 * u * torch.sqrt((1 + r2) / (3 * n)) * (1 + xh) + u * u * (1 + r2) * xh / 2)   # [B, 32]

    def extra(name, mask):
        if u == 0.0:
            return 0.0
        gm = mask.reshape(GROUPS, -1).any(dim=1)
        return float(gap[:, gm].max())

    return extra


def check_partial(r, ys, gamma, beta, film, dtype, tag, worst):
    y = torch.cat(ys, dim=1)
    a, b = r["a"].cpu(), r["b"].cpu()
    assert torch.isfinite(a).all() and torch.isfinite(b).all(), f"{tag}: (a, b) not written"
    res = check_ab(a, b, y, gamma, beta, film, tag, ncls=CONV_CLASSES, report=print, extra=rounding_gap(dtype, y, gamma, beta, film))
    for k, (e, err, bud) in res.items():
        w = worst.setdefault(k, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], e), max(w[1], err), max(w[2], err / max(e, 1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_conv_partial_sums_and_finalize_vs_fp64(ops, dtype):
    """Each conv route that fills statistics slots, the offset coming from the conv's bias, then gn_finalize: (a, b) against fp64 GroupNorm
    of the tensor the conv stored.  Also the conv output itself against F.conv2d (the op must run the conv it reports)."""
    reached, pp_forms = set(), set()
    worst = {}
    for ci, (name, B, Cin, Co, H, W, k, stride, knobs, accept, only16) in enumerate(ROUTE_CASES):
        if only16 and dtype == F32:
            continue
        x = randn(51000 + ci, B, Cin, H, W)
        w = conv_weights(52000 + ci, Co, Cin, k)
        bias = class_bias(53000 + ci, Co, Co, 0)
        for film_on in (False, True):
            gamma, beta, film = make_params(54000 + ci, B, Co, film_on)
            tag = f"{NAME[dtype]} {name} B={B} {Cin}->{Co} film={film_on}"
            r = ops.conv2d_gn(dev(x), w, bias, dev(gamma), dev(beta), film=dev(film), stride=stride, dtype=dtype, debug=_lib.debug_config(**knobs))
            print(f"   GNROUTE {tag}: kernel {r['kernel']} slots {r['slots']}")
            assert r["slots"] > 0, f"{tag}: the route (kernel {r['kernel']}) filled no statistics slots"
            assert r["kernel"] in accept, f"{tag}: kernel {r['kernel']}, expected one of {sorted(accept)}"
            reached.add(r["kernel"])
            if r["kernel"] == K_PP:          # both geometries of the ping-pong kernel: 0 = 256 pixels x 256 channels, 1 = 512 x 128
                assert r["form"] == (1 if "narrow" in name else 0), f"{tag}: ping-pong form {r['form']}"
                pp_forms.add(r["form"])
            y = r["y"].cpu()
            xr, wr = (x, w) if dtype == F32 else (x.to(TORCH16[dtype]).float(), w.to(TORCH16[dtype]).float())
            want = F.conv2d(xr.double(), wr.double(), bias.double(), stride=stride, padding=k // 2)
            tol = (1e-4 if dtype == F32 else 2.5 * U16[dtype]) * float(want.abs().max())
            assert float((y.double() - want).abs().max()) < tol, f"{tag}: conv output"
            check_partial(r, [y], gamma, beta, film, dtype, tag, worst)
    # two producers feed one finalize (the concat sites): 256 + 128 channels, groups of 12 straddle the boundary; 128 + 128
    for ci, (B, Ci0, Co0, Ci1, Co1, H, W, knobs) in enumerate([(4, 128, 256, 128, 128, 28, 28, dict(conv_pp=0, conv_ws=0)),
                                                                (3, 128, 256, 128, 128, 20, 28, dict(conv_pp=2)),
                                                                (5, 128, 128, 128, 128, 32, 32, dict(conv_pp=0))]):
        C = Co0 + Co1
        x0, x1 = randn(56000 + ci, B, Ci0, H, W), randn(56100 + ci, B, Ci1, H, W)
        w0, w1 = conv_weights(56200 + ci, Co0, Ci0, 3), conv_weights(56300 + ci, Co1, Ci1, 3)
        b0, b1 = class_bias(56400 + ci, Co0, C, 0), class_bias(56500 + ci, Co1, C, Co0)
        for film_on in (False, True):
            gamma, beta, film = make_params(56600 + ci, B, C, film_on)
            tag = f"{NAME[dtype]} two producers {Co0}+{Co1} {H}x{W} film={film_on}"
            r = ops.conv2d_gn(dev(x0), w0, b0, dev(gamma), dev(beta), x1=dev(x1), weight1=w1, bias1=b1, film=dev(film), dtype=dtype,
                              debug=_lib.debug_config(**knobs))
            print(f"   GNROUTE {tag}: kernels {r['kernel']}, {r['kernel1']} slots {r['slots']}, {r['slots1']}")
            assert r["slots"] > 0 and r["slots1"] > 0, f"{tag}: a producer filled no slots"
            check_partial(r, [r["y"].cpu(), r["y1"].cpu()], gamma, beta, film, dtype, tag, worst)
    print(f"   GNSUM partial sums {NAME[dtype]} kernels {sorted(reached)}: " + " ".join(f"{k}: e_ref {w[0]:.2e} err {w[1]:.2e} ratio {w[2]:.2f};" for k, w in worst.items()))
    want = {K_IGEMM, K_1X1, K_1X1_PP, K_PP, K_WS} | (set() if dtype == F32 else {K_IN})
    assert reached >= want, f"conv routes reached: {sorted(reached)}, wanted {sorted(want)}"
    assert pp_forms == {0, 1}, f"ping-pong geometries reached: {sorted(pp_forms)}"


# ---- affine pool -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_affine_pool_vs_fp64(ops, dtype):
    for ci, (B, C, H, W) in enumerate([(3, 128, 16, 16), (2, 96, 14, 10), (1, 640, 8, 8), (300, 64, 4, 4), (2, 160, 28, 20)]):
        x = make_input(61000 + ci, B, C, H * W, dtype=TORCH16.get(dtype)).reshape(B, C, H, W)
        gamma, beta, film = make_params(62000 + ci, B, C, True)
        m, v = stats64(x)
        from tests.test_gn_ref_cpu import fold64

        a64, b64 = fold64(m, v, gamma * 4.0, beta, film)      # SiLU arguments reach +-15
        a, b = a64.float(), b64.float()
        for silu in (True, False):
            tag = f"{NAME[dtype]} pool B={B} C={C} {H}x{W} silu={silu}"
            got = ops.affine_pool(dev(x), dev(a), dev(b), silu=silu, dtype=dtype).cpu().double()
            v4 = apply_ab(a, b, x)
            want = F.avg_pool2d(silu64(v4) if silu else v4, 2)
            mag = F.avg_pool2d(a.double().abs()[:, :, None, None] * x.double().abs() + b.double().abs()[:, :, None, None] + 1.0, 2)
            tol = 8 * 2.0 ** -24 * mag + 1.01 * U16[dtype] * want.abs() + (2.0 ** -24 if dtype == F16 else 0.0)   # four fma + SiLU + three adds, then the store
            assert torch.isfinite(got).all(), f"{tag}: unwritten outputs"
            bad = float(((got - want).abs() - tol).max())
            assert bad <= 0, f"{tag}: off by {bad:.3e} beyond the tolerance"
        got = ops.affine_pool(dev(x), dtype=dtype).cpu().double()          # no affine: plain pooling
        want = F.avg_pool2d(x.double(), 2)
        tol = 4 * 2.0 ** -24 * F.avg_pool2d(x.double().abs(), 2) + 1.01 * U16[dtype] * want.abs() + (2.0 ** -24 if dtype == F16 else 0.0)   # three adds of the four |x|
        assert float(((got - want).abs() - tol).max()) <= 0, f"{NAME[dtype]} pool B={B} C={C} {H}x{W} without affine"


# ---- backward --------------------------------------------------------------------------------------------------------------------------
def vjp_refs(xs, du, gamma, beta, film, silu):
    """fp64 autograd and fp32 eager autograd of the same expression -> (grads64, grads32) per source."""
    out = []
    for dt in (torch.float64, torch.float32):
        leaves = [t.to(dt).requires_grad_() for t in xs if t is not None]
        x = torch.cat(leaves, dim=1)
        B, C = x.shape[:2]
        if dt == torch.float64:
            u = gn64(x, gamma, beta, film, silu=silu)
        else:
            h = F.group_norm(x, GROUPS, gamma, beta, EPS)
            if film is not None:
                h = h * (1 + film[:, :C, None]) + film[:, C:, None]
            u = F.silu(h) if silu else h
        out.append(torch.autograd.grad((u * du.to(dt)).sum(), leaves))
    return out


BWD_CASES = {
    # C0, C1, HW, B, du_stride (0 = C), accumulate into (g0, g1)
    F32: [(96, 0, 49, 2, 0, (False, False)), (160, 0, 196, 1, 192, (True, False)), (128, 0, 16, 3, 0, (False, False)), (256, 128, 64, 2, 0, (True, True)),
          (256, 128, 196, 1, 512, (False, True)), (64, 32, 64, 2, 0, (True, False)), (640, 0, 64, 1, 0, (False, False)), (1024, 512, 16, 1, 0, (True, True)),
          (128, 0, 784, 1, 0, (False, False)), (128, 0, 1024, 1, 160, (True, False)), (128, 0, 4096, 1, 0, (False, False)), (64, 0, 16, 300, 0, (True, False))],
    BF16: [(192, 0, 49, 2, 0, (False, False)), (320, 0, 196, 1, 384, (True, False)), (256, 0, 16, 3, 0, (False, False)), (256, 128, 64, 2, 0, (True, True)),
           (256, 128, 196, 1, 512, (False, True)), (64, 32, 64, 2, 0, (True, False)), (640, 0, 64, 1, 0, (False, False)), (1024, 512, 16, 1, 0, (True, True)),
           (128, 0, 784, 1, 0, (False, False)), (128, 0, 1024, 1, 160, (True, False)), (128, 0, 4096, 1, 0, (False, False)), (64, 0, 16, 300, 0, (True, False))],
}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_gn_silu_vjp_vs_fp64_autograd(ops, dtype):
    """fp32: |err| <= 4 x the error of fp32 eager autograd on the same inputs + 4 ulps of the largest gradient.  bf16 (inputs, cotangent
    and pre-filled gradients rounded to bf16 first, as in test_gpu_vjp_ops.py): the same plus the one rounding the kernel adds, the bf16
    store of the result: 2^-8 (half an ulp) of the largest stored value."""
    worst = 0.0
    for ci, (C0, C1, HW, B, stride, accs) in enumerate(BWD_CASES[dtype]):
        C = C0 + C1
        t16 = TORCH16.get(dtype)
        x = make_input(71000 + ci, B, C, HW, dtype=t16)
        # constant groups carry rstd = 316: their gradient is cancellation noise in any precision; keep the other classes (r16 included)
        cpg = C // GROUPS
        for g in range(GROUPS):
            if CLASS_NAMES[g % len(CLASS_NAMES)] in ("const", "near"):
                x[:, g * cpg:(g + 1) * cpg] = randn(71500 + g, B, cpg, HW) * 1.2 + 0.3
        du = randn(72000 + ci, B, C, HW)
        pre = [randn(73000 + ci, B, C0, HW) * 2.0, randn(73100 + ci, B, C1, HW) * 2.0 if C1 else None]
        if t16:
            x, du = x.to(t16).float(), du.to(t16).float()
            pre = [p.to(t16).float() if p is not None else None for p in pre]
        xs = (x[:, :C0].contiguous(), x[:, C0:].contiguous() if C1 else None)
        for film_on, silu in ((True, True), (False, True), (True, False)):
            gamma, beta, film = make_params(74000 + ci, B, C, film_on)
            gamma = gamma * 5.0                       # SiLU arguments across +-20
            tag = f"{NAME[dtype]} vjp C={C0}+{C1} HW={HW} B={B} du_stride={stride or C} acc={accs} film={film_on} silu={silu}"
            g64, g32 = vjp_refs(xs, du, gamma, beta, film, silu)
            g0 = dev(pre[0].clone()) if accs[0] else None
            g1 = dev(pre[1].clone()) if (accs[1] and C1) else None
            got = ops.gn_silu_vjp(dev(xs[0]), dev(du), dev(gamma), dev(beta), x1=dev(xs[1]), film=dev(film), silu=silu, du_stride=stride or None,
                                  g0=g0, g1=g1, dtype=dtype)
            for k in range(2 if C1 else 1):          # each source's gradient on its own tensor
                have = got[k].cpu().double()
                assert torch.isfinite(have).all(), f"{tag}: source {k}: unwritten gradient entries"
                want = g64[k] + (pre[k].double() if accs[k] else 0.0)
                e32 = float((g32[k].double() - g64[k]).abs().max())
                bud = 4 * e32 + 4 * ULP32 * float(g64[k].abs().max()) + 1.01 * U16[dtype] * float(want.abs().max())
                err = float((have - want).abs().max())
                worst = max(worst, err / bud)
                print(f"   GNSTAT {tag} source {k}: fp32 autograd err {e32:.3e} kernel err {err:.3e} budget {bud:.3e}")
                assert err <= bud, f"{tag}: source {k}: err {err:.3e} > budget {bud:.3e} (fp32 autograd err {e32:.3e})"
    print(f"   GNSUM gn_silu_vjp {NAME[dtype]}: worst err / budget {worst:.3f}")


def test_backward_ops_reject_other_dtypes():
    """fp16 never reaches the backward kernels (fp32 and bf16 only): refused before anything is launched or allocated."""
    import ctypes as C

    L = _lib.lib()
    p = C.c_void_p(16)   # never dereferenced: the dtype check comes first
    for bad in (_lib.MI355_F16, _lib.MI355_BF16X2):
        rc = L.mi355_gn_silu_vjp(p, None, p, p, None, 1e-5, 1, p, 32, p, None, 0, 0, 1, 32, 0, 16, bad, None)
        assert rc < 0 and b"gn_silu_vjp" in L.mi355_last_error()
        rc = L.mi355_grad_gather(p, p, 1, 32, 4, 4, 4, 4, 32, 0, 0, 0, 1.0, bad, None)
        assert rc < 0 and b"grad_gather" in L.mi355_last_error()
        route = (C.c_int32 * 4)(7, 7, 7, 7)
        rc = L.mi355_conv2d_vjp(C.cast(p, C.POINTER(C.c_float)), p, p, None, None, 0, 0, 1, 32, 32, 32, 0, 4, 4, 3, 0, 32, bad, None, route, p, 1 << 20, None)
        assert rc < 0 and b"conv2d_vjp" in L.mi355_last_error() and list(route) == [-1, -1, -1, -1]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_grad_gather_vs_fp64_autograd(ops, dtype):
    """The four modes as the adjoints they stand for, with a channel offset into a wider source, accumulate and scale."""
    t16 = TORCH16.get(dtype)

    def rnd(t):
        return t.to(t16).float() if t16 else t

    # mode, B, Cd, Hd, Wd, source channels, coff
    cases = [(0, 3, 64, 7, 5, 96, 32), (0, 300, 32, 4, 4, 32, 0), (1, 2, 96, 7, 5, 160, 64), (1, 1, 640, 4, 4, 640, 0),
             (2, 2, 64, 14, 10, 128, 64), (2, 1, 160, 8, 8, 160, 0), (3, 2, 64, 14, 10, 96, 32), (3, 2, 32, 7, 5, 32, 0), (3, 1, 128, 16, 16, 128, 0)]
    for ci, (mode, B, Cd, Hd, Wd, Cs, coff) in enumerate(cases):
        Hs, Ws = {0: (Hd, Wd), 1: (2 * Hd, 2 * Wd), 2: ((Hd + 1) // 2, (Wd + 1) // 2), 3: ((Hd + 1) // 2, (Wd + 1) // 2)}[mode]
        if mode == 2:
            Hd, Wd = 2 * Hs, 2 * Ws     # AvgPool2d(2) of an even image
        src = rnd(randn(81000 + ci, B, Cs, Hs, Ws))
        pre = rnd(randn(82000 + ci, B, Cd, Hd, Wd))
        cot = src[:, coff:coff + Cd].double()
        z = torch.zeros(B, Cd, Hd, Wd, dtype=torch.float64, requires_grad=True)
        if mode == 0:
            fwd = z
        elif mode == 1:
            fwd = F.interpolate(z, scale_factor=2, mode="nearest")
        elif mode == 2:
            fwd = F.avg_pool2d(z, 2) * 4.0           # the kernel's G; the engine passes scale = 1/4
        else:
            fwd = F.conv2d(z, torch.eye(Cd, dtype=torch.float64)[:, :, None, None], stride=2)
        (G, Gabs) = (torch.autograd.grad((fwd * c).sum(), z, retain_graph=True)[0] for c in (cot, cot.abs()))   # Gabs: the sum of |terms|
        for acc, scale in ((False, 1.0), (True, 0.25), (True, -1.5)):
            tag = f"{NAME[dtype]} gather mode={mode} B={B} Cd={Cd} {Hd}x{Wd} src C={Cs} coff={coff} acc={acc} scale={scale}"
            dst = dev(pre.clone()) if acc else None
            got = ops.grad_gather(dev(src), (Cd, Hd, Wd), mode, coff=coff, scale=scale, dst=dst, dtype=dtype).cpu().double()
            want = scale * G + (pre.double() if acc else 0.0)
            assert torch.isfinite(got).all(), f"{tag}: unwritten entries"
            mag = abs(scale) * Gabs + (pre.double().abs() if acc else 0.0)
            tol = 4 * ULP32 * mag + 1.01 * U16[dtype] * want.abs() + 1e-30
            bad = float(((got - want).abs() - tol).max())
            assert bad <= 0, f"{tag}: off by {bad:.3e} beyond the tolerance"
