"""CPU: the fp64 references and the error budgets of tests/test_gpu_gn_ops.py, proved without a GPU.

GroupNorm32 (nn.py:11-13, 87-94: nn.GroupNorm(32, C), eps 1e-5) with FiLM (unet.py:343-347) is, per image and group of C / 32 channels,
    y = (x - mean) * rstd * gamma * (1 + scale) + beta * (1 + scale) + shift,   rstd = 1 / sqrt(var + eps),   var biased.
The engine never forms y in a pass of its own: a kernel folds the statistics into a per-(image, channel) affine  y = a x + b  that the
consumer applies.  The GPU tests evaluate the kernel's fp32 (a, b) as a x + b in fp64 and compare with the fp64 y.

Budget (fixed before any kernel was measured; nothing here is fitted to a kernel):
    e_ref  = max |fp32 eager reference - fp64 y| on the same input: torch.nn.functional.group_norm in fp32, then the FiLM expression in fp32;
    budget = 4 * e_ref + 4 * 2^-23 * max |y|.
The factor 4 allows a different but sound summation order; the floor is four fp32 ulps of the largest output.  Inputs are made of groups
with chosen |mean| / std (0, 1, 4, 16, 64), a nearly constant group (std = 1e-3 |mean|) and an exactly constant group, one class per
group, and e_ref, the error and the budget are taken PER CLASS so that the ill-conditioned groups do not pay for the others.
The constant and nearly constant classes get one more term (see fold_limit): the rounding of b and of the mean at the size of |a x|.

This module shows that (i) the fp64 helpers are the oracle's GroupNorm and torch autograd, (ii) the reference itself and an exact-statistics
(a, b) rounded to fp32 pass the budget for every case family, and (iii) the single-pass fp32  E[x^2] - mean^2  that the kernels used before
fails it at ratios 16 and 64, i.e. the GPU test can see that defect.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from mi355.synth import randn
from oracle import unet_ref

GROUPS = 32
EPS = 1e-5
ULP32 = 2.0 ** -23
# one class per group, cyclic: |mean| / std, or a tag
CLASSES = (0.0, 1.0, 4.0, 16.0, 64.0, "near", "const")
CLASS_NAMES = ("r0", "r1", "r4", "r16", "r64", "near", "const")


def group_class(g):
    return g % len(CLASSES)


def make_input(seed, B, C, HW, classes=True, dtype=None):
    """x [B, C, HW] fp32: group g of every image is std-1 noise scaled and offset by its class (sign alternating with the group), each
    channel with its own small extra offset so that channels of a group differ; classes=False: plain noise * 1.5 + 0.2.
    dtype: a 16-bit torch dtype the values are rounded to (the kernel reads exactly those)."""
    x = randn(seed, B, C, HW)
    if not classes:
        x = x * 1.5 + 0.2
    else:
        cpg = C // GROUPS
        chan_off = randn(seed + 1, C) * 0.3
        for g in range(GROUPS):
            k = CLASSES[group_class(g)]
            sl = slice(g * cpg, (g + 1) * cpg)
            sign = -1.0 if g % 2 else 1.0
            std = 0.5 + 0.25 * (g % 5)
            if k == "const":
                x[:, sl] = sign * (0.75 + 0.125 * (g % 3))
            elif k == "near":
                m = sign * (1.0 + 0.5 * (g % 3))
                x[:, sl] = m + x[:, sl] * (1e-3 * abs(m))
            else:
                x[:, sl] = (x[:, sl] + chan_off[sl, None]) * std + sign * k * std
    if dtype is not None:
        x = x.to(dtype).float()
    return x.contiguous()


def make_params(seed, B, C, film):
    """gamma (with negative and zero entries), beta, FiLM [B, 2C] = scale | shift: all drawn independently per channel."""
    gamma = randn(seed, C) * 0.8 + 0.3
    gamma[3::17] = 0.0
    beta = randn(seed + 1, C) * 0.5
    fl = torch.cat((randn(seed + 2, B, C) * 0.4, randn(seed + 3, B, C) * 0.7), dim=1).contiguous() if film else None
    return gamma, beta, fl


def stats64(x):
    """mean, biased var [B, 32] of x [B, C, *] in fp64."""
    B, C = x.shape[:2]
    xg = x.double().reshape(B, GROUPS, -1)
    return xg.mean(dim=2), xg.var(dim=2, unbiased=False)


def per_channel(v, C):
    """[B, 32] group values -> [B, C]."""
    return v.repeat_interleave(C // GROUPS, dim=1)


def film_parts(film, C, like):
    if film is None:
        return torch.zeros_like(like), torch.zeros_like(like)
    return film[:, :C].to(like.dtype), film[:, C:].to(like.dtype)


def gn64(x, gamma, beta, film=None, eps=EPS, silu=False):
    """The definition in fp64 (differentiable): x [B, C, *]."""
    B, C = x.shape[:2]
    xd = x.double() if x.dtype != torch.float64 else x
    xg = xd.reshape(B, GROUPS, -1)
    mean, var = xg.mean(dim=2, keepdim=True), xg.var(dim=2, unbiased=False, keepdim=True)
    xh = ((xg - mean) / torch.sqrt(var + eps)).reshape(B, C, -1)
    sc, sh = film_parts(film, C, xh[:, :, 0])
    y = xh * (gamma.double() * (1 + sc))[:, :, None] + (beta.double() * (1 + sc) + sh)[:, :, None]
    y = y.reshape(xd.shape)
    return F.silu(y) if silu else y


def gn32_eager(x, gamma, beta, film=None, eps=EPS):
    """The reference implementation in fp32: torch's GroupNorm, then the FiLM expression h * (1 + scale) + shift (unet.py:346)."""
    B, C = x.shape[:2]
    h = F.group_norm(x.float(), GROUPS, gamma.float(), beta.float(), eps)
    if film is not None:
        shp = (B, C) + (1,) * (x.dim() - 2)
        h = h * (1 + film[:, :C].float().reshape(shp)) + film[:, C:].float().reshape(shp)
    return h


def fold64(mean, var, gamma, beta, film, eps=EPS):
    """(a, b) [B, C] in fp64 from group statistics [B, 32]."""
    C = gamma.numel()
    rstd = 1.0 / torch.sqrt(var.double() + eps)
    a = per_channel(rstd, C) * gamma.double()
    b = beta.double() - per_channel(mean.double(), C) * a
    sc, sh = film_parts(film, C, a)
    return a * (1 + sc), b * (1 + sc) + sh


def apply_ab(a, b, x):
    """a x + b in fp64 for fp32 (a, b) [B, C] and x [B, C, *]."""
    shp = a.shape + (1,) * (x.dim() - 2)
    return a.double().reshape(shp) * x.double() + b.double().reshape(shp)


def class_masks(C, ncls=len(CLASSES)):
    """name -> bool [C]: the channels whose group has that class (group g has class g % ncls)."""
    cpg = C // GROUPS
    cls = torch.tensor([(c // cpg) % ncls for c in range(C)])
    return {n: cls == i for i, n in enumerate(CLASS_NAMES[:ncls])}


def fold_limit(a, x):
    """What no fp32 (a, b) can avoid where rstd |mean| is large.  In the constant and the nearly constant class var << eps, so
    a = gamma_eff / sqrt(eps) ~ 316 gamma_eff and y = a x + b is the difference of two numbers of size |a x| ~ 300 |y|.  Whatever rounding a
    carries cancels when b is formed from the rounded a (a x + b = a (x - mean) + beta_eff); what cannot cancel is b's own rounding,
    2^-24 |b| with |b| ~ |a x|, and the rounding of the fp32 mean, 2^-24 |mean| |a|: 2 * 2^-24 max |a x| in all.  e_ref knows nothing of it
    (the reference subtracts the mean before it multiplies), so these two classes get it on top of 4 e_ref + floor; the offset classes do not
    (there 4 e_ref covers it: test_reference_and_exact_fold_pass_and_single_pass_fails).  That the nearly constant class needs it, and not
    only the constant one, is shown by test_near_class_needs_the_fold_limit: the EXACT statistics, folded in fp64 and rounded once to fp32,
    miss 4 e_ref + floor there."""
    xmax = x.double().abs().reshape(x.shape[0], x.shape[1], -1).max(dim=2).values   # [B, C]
    return 2.0 * 2.0 ** -24 * float((a.double().abs() * xmax).max())


def budgets(x, gamma, beta, film, ncls=len(CLASSES)):
    """-> (y64, {class: (e_ref, budget, channel mask)})."""
    C = x.shape[1]
    y64 = gn64(x, gamma, beta, film)
    y32 = gn32_eager(x, gamma, beta, film).double()
    out = {}
    masks = class_masks(C, ncls)
    for name, m in masks.items():
        if not bool(m.any()):
            continue
        e = float((y32[:, m] - y64[:, m]).abs().max())
        bud = 4 * e + 4 * ULP32 * float(y64[:, m].abs().max())
        out[name] = (e, bud, m)
    return y64, out


def check_ab(a, b, x, gamma, beta, film, tag, ncls=len(CLASSES), report=None, extra=None):
    """Assert a x + b (fp64 evaluation of the fp32 a, b) against fp64 GroupNorm, class by class (group g: class g % ncls).  extra: a callable (class name, channel
    mask) -> an additional absolute budget with its own derivation (the partial-sum path).  -> {class: (e_ref, err, budget)}."""
    y64, buds = budgets(x, gamma, beta, film, ncls)
    got = apply_ab(a, b, x)
    res = {}
    for name, (e, bud, m) in buds.items():
        if name in ("const", "near"):
            bud += fold_limit(a[:, m], x[:, m])
        if extra is not None:
            bud += extra(name, m)
        err = float((got[:, m] - y64[:, m]).abs().max())
        res[name] = (e, err, bud)
        if report is not None:
            report(f"   GNSTAT {tag} class={name} e_ref {e:.3e} err {err:.3e} budget {bud:.3e} err/e_ref {err / max(e, 1e-30):.2f}")
    for name, (e, err, bud) in res.items():
        assert err <= bud, f"{tag} class {name}: |a x + b - y64| = {err:.3e} > budget {bud:.3e} (e_ref {e:.3e})"
    return res


def check_stats(mean, rstd, x, tag, eps=EPS):
    """mean, rstd [B, 32] against fp64: 4 x the error of torch's own fp32 statistics (native_group_norm) plus a floor.  torch's CPU kernel
    accumulates wider than fp32, so its error is half an ulp or less and says nothing about an fp32 summation tree; the floor is therefore
    the a priori bound of PAIRWISE fp32 summation over the n = cpg * HW elements of a group (Higham, Accuracy and Stability of Numerical
    Algorithms, section 4.2: relative error (log2 n + 1) u on a sum of like-signed terms, u = 2^-24), the best a kernel that sums in fp32
    can promise:
      rstd: the sum of squared deviations carries (log2 n + 1) u, the square root halves it, sqrt and divide add u each;
      mean: the sum of the deviations carries (log2 n + 1) u of the group's mean |x - mean|, the result is rounded once at |mean|."""
    B, C = x.shape[:2]
    n = (C // GROUPS) * x[0, 0].numel()
    u, lg = 2.0 ** -24, math.log2(n) + 1
    m64, v64 = stats64(x)
    r64 = 1.0 / torch.sqrt(v64 + eps)
    dev64 = (x.double().reshape(B, GROUPS, -1) - m64[:, :, None]).abs().mean(dim=2)
    _, m32, r32 = torch.native_group_norm(x.float().reshape(B, C, -1), None, None, B, C, x[0, 0].numel(), GROUPS, eps)
    floors = {"mean": lg * u * dev64 + u * m64.abs(), "rstd": (0.5 * lg + 2) * u * r64}
    for g in range(GROUPS):
        k = group_class(g)
        for what, got, ref, ref32 in (("mean", mean, m64, m32), ("rstd", rstd, r64, r32)):
            e = float((ref32[:, g].double() - ref[:, g]).abs().max())
            err = (got[:, g].double() - ref[:, g]).abs()
            bud = 4 * e + floors[what][:, g]
            assert bool((err <= bud).all()), (f"{tag} group {g} ({CLASS_NAMES[k]}) {what}: err {float(err.max()):.3e} > budget {float(bud.min()):.3e} "
                                              f"(torch fp32 err {e:.3e})")


def single_pass_ab(x, gamma, beta, film, eps=EPS):
    """The arithmetic the kernels used before: per channel, fp32 sums of x and x^2 accumulated pixel by pixel, channels added per group,
    var = max(E[x^2] - mean^2, 0), everything in fp32."""
    B, C = x.shape[:2]
    xf = x.float().reshape(B, C, -1)
    HW = xf.shape[2]
    s = torch.cumsum(xf, dim=2)[:, :, -1].reshape(B, GROUPS, -1).sum(dim=2)
    q = torch.cumsum(xf * xf, dim=2)[:, :, -1].reshape(B, GROUPS, -1).sum(dim=2)
    inv = torch.tensor(1.0 / ((C // GROUPS) * HW), dtype=torch.float32)
    mean = s * inv
    var = torch.clamp(q * inv - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    a = per_channel(rstd, C) * gamma.float()
    b = beta.float() - per_channel(mean, C) * a
    if film is not None:
        sc = 1.0 + film[:, :C].float()
        a, b = a * sc, b * sc + film[:, C:].float()
    return a, b


# (C0, C1, HW, B, 16-bit?) of every case family of the GPU test, at sizes an fp64 reference on the CPU affords
FAMILIES = [
    (96, 0, 49, 2, False), (160, 0, 196, 2, False), (192, 0, 49, 2, True), (320, 0, 196, 1, True),          # C / V does not divide 512
    (128, 0, 16, 3, False), (256, 0, 16, 2, False), (128, 0, 64, 2, False), (256, 0, 64, 2, False),        # NL = 1, 2, 4, 8 (fp32)
    (640, 0, 64, 1, False), (1024, 0, 16, 1, False), (1024, 512, 64, 1, True),                              # C > 512
    (256, 128, 64, 2, True), (256, 128, 196, 1, False), (64, 32, 64, 2, False),                             # groups straddle the sources
    (128, 0, 784, 1, False), (128, 0, 1024, 1, True), (128, 0, 4096, 1, False),                             # large images
    (64, 0, 16, 300, False),                                                                                # a batch of a few hundred
]


def test_fp64_helpers_match_the_oracle_and_autograd():
    x = make_input(11, 2, 96, 49)
    gamma, beta, film = make_params(12, 2, 96, True)
    torch.testing.assert_close(gn64(x, gamma, beta).float(), unet_ref.group_norm32(x, gamma, beta), rtol=0, atol=2e-4)
    plain = randn(13, 2, 64, 5, 5)
    g2, b2, f2 = make_params(14, 2, 64, True)
    torch.testing.assert_close(gn64(plain, g2, b2).float(), unet_ref.group_norm32(plain, g2, b2), rtol=1e-5, atol=1e-5)
    # folded statistics are the definition
    m, v = stats64(plain)
    a, b = fold64(m, v, g2, b2, f2)
    torch.testing.assert_close(apply_ab(a, b, plain), gn64(plain, g2, b2, f2), rtol=1e-12, atol=1e-12)
    # the backward reference: autograd through gn64 equals autograd through torch's own fp64 group_norm + FiLM + SiLU
    xd = plain.double().requires_grad_()
    du = randn(15, 2, 64, 5, 5).double()
    (g_ours,) = torch.autograd.grad((gn64(xd, g2, b2, f2, silu=True) * du).sum(), xd)
    xe = plain.double().requires_grad_()
    h = F.group_norm(xe, GROUPS, g2.double(), b2.double(), EPS)
    h = F.silu(h * (1 + f2[:, :64].double()[:, :, None, None]) + f2[:, 64:].double()[:, :, None, None])
    (g_torch,) = torch.autograd.grad((h * du).sum(), xe)
    torch.testing.assert_close(g_ours, g_torch, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: "C%d+%d_HW%d_B%d_%s" % (f[0], f[1], f[2], f[3], "bf16" if f[4] else "fp32"))
def test_reference_and_exact_fold_pass_and_single_pass_fails(fam):
    C0, C1, HW, B, half = fam
    C = C0 + C1
    seed = 31000 + C * 7 + HW
    x = make_input(seed, B, C, HW, dtype=torch.bfloat16 if half else None)
    for film_on in (False, True):
        gamma, beta, film = make_params(seed + 5, B, C, film_on)
        tag = f"C={C0}+{C1} HW={HW} B={B} film={film_on}"
        # (ii) the fp32 reference is inside the budget by construction (4 e_ref); the exact statistics, folded and rounded to fp32, are too
        m, v = stats64(x)
        a, b = fold64(m, v, gamma, beta, film)
        res = check_ab(a.float(), b.float(), x, gamma, beta, film, tag + " exact-fold")
        m32, r32 = m.float(), (1.0 / torch.sqrt(v + EPS)).float()
        check_stats(m32, r32, x, tag + " exact-stats")
        # (iii) the single-pass sums fall outside it where the offset dominates
        a1, b1 = single_pass_ab(x, gamma, beta, film)
        y64 = gn64(x, gamma, beta, film)
        got = apply_ab(a1, b1, x)
        masks = class_masks(C)
        for name in ("r16", "r64"):
            mk = masks[name]
            err = float((got[:, mk] - y64[:, mk]).abs().max())
            assert err > res[name][2], f"{tag}: single-pass error {err:.3e} at {name} is inside the budget {res[name][2]:.3e}: the test could not see the defect"


def test_near_class_needs_the_fold_limit():
    """Why the nearly constant class carries fold_limit.  A bf16 input of that class is a handful of grid values around the mean (the
    spacing, 2^-7 |mean|, is eight times the class's std), so var << eps and a ~ 316 gamma_eff as in the constant class.  For this input
    the best any kernel can return, the fp64 statistics folded in fp64 and rounded once to fp32, is off by 6.9e-5 where
    4 e_ref + floor is 4.7e-5 (e_ref 1.1e-5); with the term (1.7e-4 here) it passes."""
    x = make_input(2052, 1, 128, 1024, dtype=torch.bfloat16)
    gamma, beta, film = make_params(5, 1, 128, True)
    m, v = stats64(x)
    a, b = fold64(m, v, gamma, beta, film)
    y64, buds = budgets(x, gamma, beta, film)
    e, bud, mk = buds["near"]
    err = float((apply_ab(a.float(), b.float(), x)[:, mk] - y64[:, mk]).abs().max())
    assert err > bud, (err, bud)
    assert err <= bud + fold_limit(a.float()[:, mk], x[:, mk])
    check_ab(a.float(), b.float(), x, gamma, beta, film, "exact fold, near class, bf16 input")


def test_constant_group_statistics_are_exact():
    x = make_input(77, 2, 128, 64)
    m, v = stats64(x)
    for g in range(GROUPS):
        if CLASS_NAMES[group_class(g)] == "const":
            assert float(v[:, g].abs().max()) == 0.0
            assert math.isclose(float(1.0 / torch.sqrt(v[0, g] + EPS)), 1.0 / math.sqrt(EPS), rel_tol=1e-12)
