"""CPU: the variational bound of a DDPM net (mi355_ddpm_vlb, mi355_vlb_terms, mi355_vlb_prior; image_diffusion.bound, DDPM.vlb_log_variances).
  1. the fp64 restatement tests/vlb_ref.py against answers it does not compute itself: torch.distributions' KL of two Normals (the step KL
     and the prior), a composite Gauss-Legendre quadrature of the Gaussian density over the bin (the decoder), the 256 bins summing to 1, and
     the far tail against math.erfc arithmetic;
  2. vlb_budget, the per-output error bound the GPU tests hold the kernels to, with the operand sets it is used on;
  3. the host logic: the index-0 convention of vlb_log_variances, the Python refusals, the library's refusals through the ABI (they come before
     any launch and before the handle is looked at).

vlb_budget.  The kernel evaluates every element in fp64 from the fp32 operands, sums in fp64 and rounds each output to fp32 once.  With U = 2^-53
(one fp64 rounding), a transcendental (exp, log, erfc, tanh) allowed 4 ulp = 8 U relative, and first-order propagation through each formula:
  x0_hat   E = 2 U (|c_recip x_k| + |c_recipm1 eps|)           two products and a difference; the clip is 1-Lipschitz
  mean_p   E = |coef1| E(x0_hat) + 2 U (|coef1 x0_hat| + |coef2 x_k|);   mean_q alike without the first term
  lp       learned: frac = (v + 1) / 2 has U |frac|; 1 - frac adds U |1 - frac|; the two products and the sum add U each on their magnitudes
  kl       d = mean_q - mean_p: E(d) = E(mean_q) + E(mean_p) + U |d|;  d^2: 2 |d| E(d) + E(d)^2 + U d^2;  exp(lq - lp), exp(-lp): relative
           E(argument) + 8 U;  the five-term sum: the terms' errors + 4 U (1 + |lp| + |lq| + e1 + t);  the halving is exact
  decoder  c = x0 - mean_p: E(mean_p) + U |c|;  s = exp(-0.5 lp): relative 0.5 E(lp) + 8 U;  a+- = s (c +- 1/255): product rule + U each;
           exact: Phi(a) = 0.5 erfc(y), y = -a / sqrt 2: E(y) = E(a) / sqrt 2 + 2 U |y|, E(Phi) = 0.5 (2 / sqrt pi exp(-y^2) E(y) + 8 U erfc(y));
           where c is within 4 E(c) of 0 the other branch may be taken: erfc <= 2 there;  tanh: g = k (a + 0.044715 a^3),
           E(g) = k E(a) (1 + 0.134145 a^2) + 6 U k (|a| + 0.044715 |a|^3), E(T) = 0.5 (sech^2(g) E(g) + 8 U |tanh g| + 2 U);
           P: the sum of its terms' errors + U |P|;  log(max(P, 1e-12)): E(P) / max(P, 1e-12) + 8 U |log| (max is 1-Lipschitz)
  squares  (x0_hat - x0)^2: E(dx) = E(x0_hat) + U |dx|, then 2 |dx| E(dx) + E(dx)^2 + U dx^2;  (eps - z)^2: 3 U de^2
  output   mean of n terms: mean(E) + (n + 2) U mean(|f|);  / ln 2: 2 U more;  then ONE fp32 rounding: EPS32 |result|.
Nothing here comes from a GPU output.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import vlb_ref as VR
from tests.test_ddpm_respace_cpu import EPS32, STEPS7
from tests.test_learned_variance_cpu import PERS

U64 = 2.0 ** -53
TRANS = 8 * U64     # 4 ulp of an fp64 transcendental
B = 3


def _ddpm(Ns):
    from image_diffusion.sde_diffusion import DDPM

    return DDPM(Ns)


# ---- 1. the restatement against independent answers ---------------------------------------------------------------------------------------------

def test_kl_against_torch_distributions():
    from torch.distributions import Normal, kl_divergence

    rng = np.random.default_rng(11)
    mq, mp = rng.normal(size=400) * 2, rng.normal(size=400) * 2
    lq, lp = rng.uniform(-12, 1, 400), rng.uniform(-12, 1, 400)
    want = kl_divergence(Normal(torch.from_numpy(mq), torch.from_numpy(np.exp(0.5 * lq))), Normal(torch.from_numpy(mp), torch.from_numpy(np.exp(0.5 * lp)))).numpy()
    got = VR.kl_normal(mq, lq, mp, lp)
    assert np.allclose(got, want, rtol=1e-11, atol=1e-13), float(np.abs(got - want).max())
    # the step term through elements(): coef1 = 1, coef2 = 0, c_recip = 1, c_recipm1 = -1 make x0_hat = x_k + eps the model mean, x0 the true one
    sc = dict(c_recip=1.0, c_recipm1=-1.0, coef1=1.0, coef2=0.0, true_log=-3.0, model_log=-2.5)
    x0, xk, eps = (rng.normal(size=50).astype(np.float32) * 0.3 for _ in range(3))
    e = VR.elements(x0, xk, eps, None, eps, sc, k_is_zero=False, learned=False, clip=False)
    xh = xk.astype(np.float64) + eps.astype(np.float64)
    want = kl_divergence(Normal(torch.from_numpy(x0.astype(np.float64)), math.exp(-1.5)), Normal(torch.from_numpy(xh), math.exp(-1.25))).numpy()
    assert np.allclose(e["term"], want, rtol=1e-11, atol=1e-13)


def test_prior_against_torch_distributions():
    from torch.distributions import Normal, kl_divergence

    x0 = np.random.default_rng(12).uniform(-1, 1, (B, 3, 5, 5)).astype(np.float32)
    sa, sb = np.float32(0.0123), np.float32(0.99992)
    want = kl_divergence(Normal(torch.from_numpy(float(sa) * x0.astype(np.float64)), float(sb)), Normal(0.0, 1.0)).reshape(B, -1).mean(1).numpy() / math.log(2.0)
    got = VR.prior(x0, sa, sb)
    assert np.allclose(got, want, rtol=1e-10, atol=1e-15), (got, want)


def _quadrature(lo, hi, mean, sigma, pieces=4000):
    """Integral of the N(mean, sigma^2) density over [lo, hi]: composite 20-point Gauss-Legendre in fp64."""
    xg, wg = np.polynomial.legendre.leggauss(20)
    edges = np.linspace(lo, hi, pieces + 1)
    h = np.diff(edges) / 2
    mid = (edges[:-1] + edges[1:]) / 2
    x = mid[:, None] + h[:, None] * xg[None, :]
    dens = np.exp(-0.5 * ((x - mean) / sigma) ** 2) / (sigma * math.sqrt(2 * math.pi))
    return float((dens * wg[None, :] * h[:, None]).sum())


@pytest.mark.parametrize("width_in_sigma", [0.05, 1.0, 20.0])
def test_decoder_against_quadrature(width_in_sigma):
    sigma = (2.0 / 255.0) / width_in_sigma
    lp = 2.0 * math.log(sigma)
    worst = 0.0
    for n in (3, 128, 200):
        x0 = n / 127.5 - 1.0
        for off in (0.0, 0.3 / 255.0, -0.9 / 255.0, 2.5 * sigma, -4.0 * sigma):
            mean = x0 - off
            want = _quadrature(x0 - 1.0 / 255.0, x0 + 1.0 / 255.0, mean, sigma)
            got = float(VR.bin_probability(np.array([x0]), np.array([mean]), np.array([lp]))[0])
            worst = max(worst, abs(got - want) / want)
            assert abs(got - want) <= 1e-10 * want + 1e-300, (n, off, got, want)
    print(f"bin {width_in_sigma} sigma wide: restatement vs quadrature, worst relative difference {worst:.2e}")


def test_the_256_bins_sum_to_one():
    grid = np.arange(256) / 127.5 - 1.0     # fp64 pixel values: adjacent bins then share their edge to fp64 rounding
    worst_exact = worst_tanh = worst_p = 0.0
    for mean in (-1.3, -0.97, -0.2, 0.0031, 0.55, 0.999, 1.2):
        for lp in (-14.0, -9.0, -5.0, -1.0, 1.5):
            pe = VR.bin_probability(grid, np.full(256, mean), np.full(256, lp), "exact")
            pt = VR.bin_probability(grid, np.full(256, mean), np.full(256, lp), "tanh")
            assert abs(pe.sum() - 1.0) <= 1e-12, (mean, lp, pe.sum())
            assert (pe >= 0).all()
            worst_exact = max(worst_exact, abs(pe.sum() - 1.0))
            worst_tanh = max(worst_tanh, abs(pt.sum() - 1.0))
            worst_p = max(worst_p, float(np.abs(pt - pe).max()))
    # informational: how far guided-diffusion's tanh approximation is from the exact CDF on the same inputs (not asserted small)
    print(f"256 bins: |sum - 1| exact {worst_exact:.2e}, tanh {worst_tanh:.2e}; max |P_tanh - P_exact| {worst_p:.3e}")


def test_exact_tail_against_math_erfc():
    """c = +-12 sigma: the bin's probability is ~1e-33; Phi(a+) - Phi(a-) through 1 + erf cancels to 0 on the right side."""
    r2 = math.sqrt(2.0)
    for lp in (-9.0, -4.0):
        s = math.exp(-0.5 * lp)
        sigma = 1.0 / s
        for sign in (1.0, -1.0):
            x0 = 40 / 127.5 - 1.0
            mean = x0 - sign * 12.0 * sigma
            c = x0 - mean
            ap, am = s * (c + 1.0 / 255.0), s * (c - 1.0 / 255.0)
            want = 0.5 * math.erfc(am / r2) - 0.5 * math.erfc(ap / r2) if sign > 0 else 0.5 * math.erfc(-ap / r2) - 0.5 * math.erfc(-am / r2)
            got = float(VR.bin_probability(np.array([x0]), np.array([mean]), np.array([lp]))[0])
            assert want > 0 and abs(got - want) <= 1e-10 * want, (lp, sign, got, want)
            naive = 0.5 * (1.0 + math.erf(ap / r2)) - 0.5 * (1.0 + math.erf(am / r2))
            if sign > 0:
                assert abs(naive - want) > 0.5 * want, "the naive form was expected to lose the right tail"


# ---- 2. the budget ----------------------------------------------------------------------------------------------------------------------------------

def vlb_cases():
    """(k, scalars) on DDPM(100) at 7 logSNR-even steps: step 0 (the decoder) and steps 1, 3 and 6 (the KL), with the learned range and both
    fixed variances' tables."""
    d = _ddpm(100)
    r = d.respace(d.logsnr_steps(7))
    T = r.host_tables()
    small, large, ml = r.vlb_log_variances("fixed_small")["true_log"], r.vlb_log_variances("fixed_large")["model_log"], r.max_log()
    out = []
    for k in (0, 1, 3, r.Ns - 1):
        out.append((k, dict(c_recip=float(T["sqrt_recip_alphas_cumprod"][k]), c_recipm1=float(T["sqrt_recipm1_alphas_cumprod"][k]),
                            coef1=float(T["posterior_mean_coef1"][k]), coef2=float(T["posterior_mean_coef2"][k]), true_log=float(small[k]),
                            model_log=float(large[k]), min_log=float(small[k]), max_log=float(ml[k]),
                            sa=float(T["sqrt_alphas_cumprod"][k]), sb=float(T["sqrt_one_minus_alphas_cumprod"][k]))))
    return out


def vlb_operands(per, sc, seed, batch=B):
    """fp32 x0, x_k, eps, v, z, each [batch, per].  x0: 8-bit pixels n / 127.5 - 1 (flat element 0 is -1, element 1 is +1); z normal; x_k the
    fp32 noising of x0 with the step's sa, sb; eps = z + 0.05 noise (a good model), but every 7th flat element (element 0 among them) is off by 100
    towards the far side: x0_hat is clipped there and, at step 0, the bin's probability sits under the 1e-12 floor; v uniform in [-1, 1] plus
    an offset per image in [-2, 2] (a cross-image mix-up moves lp by far more than the budget)."""
    rng = np.random.default_rng(seed)
    n = batch * per
    f = np.float32
    pix = rng.integers(0, 256, n)
    pix[0] = 0
    if n > 1:
        pix[1] = 255
    x0 = (pix.astype(f) / f(127.5) - f(1.0)).astype(f)
    z = rng.standard_normal(n).astype(f)
    xk = VR.q_sample32(x0, z, sc["sa"], sc["sb"])
    eps = (z + f(0.05) * rng.standard_normal(n).astype(f)).astype(f)
    bad = np.arange(n) % 7 == 0
    eps[bad] = (z[bad] + np.where(x0[bad] <= 0, f(-100.0), f(100.0))).astype(f)
    v = (rng.uniform(-1.0, 1.0, (batch, per)) + np.linspace(-2.0, 2.0, batch)[:, None]).astype(f)
    return tuple(a.reshape(batch, per) for a in (x0, xk, eps)) + (v, z.reshape(batch, per))


def operand_census(x0, xk, eps, v, z, sc, *, k_is_zero, learned, cdf, clip):
    """How many elements sit on each hard branch (asserted on the CPU so that the GPU test cannot pass on inputs that avoid them)."""
    e = VR.elements(x0, xk, eps, v, z, sc, k_is_zero=k_is_zero, learned=learned, cdf=cdf, clip=False)
    pix = np.rint((x0.astype(np.float64) + 1.0) * 127.5)
    return dict(minus_one=int((x0 == -1.0).sum()), plus_one=int((x0 == 1.0).sum()),
                on_grid=int((x0 == (pix.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).astype(np.float32)).sum()),
                clipped=int((np.abs(e["x0_hat"]) > 1.0).sum()), v_outside=int((np.abs(v) > 1.0).sum()),
                floor=int((VR.elements(x0, xk, eps, v, z, sc, k_is_zero=True, learned=learned, cdf=cdf, clip=clip)["P"] < 1e-12).sum()) if k_is_zero else -1)


def vlb_budget(x0, xk, eps, v, z, sc, *, k_is_zero, learned, cdf="exact", clip=True):
    """-> (fp64 [B, 3] = vb, xstart_mse, mse from the fp32 operands; its bound [B, 3]).  The derivation: this module's docstring."""
    want = VR.terms(x0, xk, eps, v, z, sc, k_is_zero=k_is_zero, learned=learned, cdf=cdf, clip=clip)
    e = VR.elements(x0, xk, eps, v, z, sc, k_is_zero=k_is_zero, learned=learned, cdf=cdf, clip=clip)
    c = {n: float(np.float32(sc[n])) for n in VR.SCALARS}
    X0, XK, EP, Z = (np.asarray(t, np.float64) for t in (x0, xk, eps, z))
    xh, mp, lp = e["x0_hat"], e["mean_p"], e["lp"]
    E_xh = 2 * U64 * (np.abs(c["c_recip"] * XK) + np.abs(c["c_recipm1"] * EP))
    E_mp = abs(c["coef1"]) * E_xh + 2 * U64 * (np.abs(c["coef1"] * xh) + np.abs(c["coef2"] * XK))
    if learned:
        frac = (np.asarray(v, np.float64) + 1.0) / 2.0
        E_fr = U64 * np.abs(frac)
        E_1f = E_fr + U64 * np.abs(1.0 - frac)
        p1, p2 = np.abs(frac * c["max_log"]), np.abs((1.0 - frac) * c["min_log"])
        E_lp = E_fr * abs(c["max_log"]) + E_1f * abs(c["min_log"]) + 2 * U64 * (p1 + p2)
    else:
        E_lp = np.zeros_like(X0)
    if not k_is_zero:
        lq = c["true_log"]
        mq = c["coef1"] * X0 + c["coef2"] * XK
        E_mq = 2 * U64 * (np.abs(c["coef1"] * X0) + np.abs(c["coef2"] * XK))
        d = mq - mp
        E_d = E_mq + E_mp + U64 * np.abs(d)
        E_d2 = 2 * np.abs(d) * E_d + E_d ** 2 + U64 * d * d
        e1, e2 = np.exp(lq - lp), np.exp(-lp)
        E_e1 = e1 * (E_lp + U64 * np.abs(lq - lp) + TRANS)
        E_e2 = e2 * (E_lp + TRANS)
        t = d * d * e2
        E_t = E_d2 * e2 + d * d * E_e2 + U64 * t
        E_term = 0.5 * (E_lp + E_e1 + E_t + 4 * U64 * (1.0 + np.abs(lp) + abs(lq) + e1 + t))
    else:
        cc = X0 - mp
        E_c = E_mp + U64 * np.abs(cc)
        s = np.exp(-0.5 * lp)
        E_s = s * (0.5 * E_lp + TRANS)
        E_P = np.zeros_like(X0)
        ambiguous = np.abs(cc) <= 4 * E_c
        lower, upper = X0 < -0.999, X0 > 0.999
        for sign, used in ((1.0, ~upper), (-1.0, ~lower)):   # a+ is read everywhere but in the upper open bin, a- everywhere but in the lower
            cpm = cc + sign / 255.0
            a = s * cpm
            E_a = E_s * np.abs(cpm) + s * (E_c + U64 / 255.0 + U64 * np.abs(cpm)) + U64 * np.abs(a)
            if cdf == "exact":
                y = a / math.sqrt(2.0)
                E_y = E_a / math.sqrt(2.0) + 2 * U64 * np.abs(y)
                # the erfc actually evaluated: of -y (the lower side), or of +y (right of the mean and in the upper open bin)
                right = (cc > 0.0) & ~lower | upper
                val = np.where(ambiguous, 2.0, np.where(right, VR.erfc(y), VR.erfc(-y)))
                E_phi = 0.5 * (2.0 / math.sqrt(math.pi) * np.exp(-y * y) * E_y + TRANS * val)
            else:
                kk = math.sqrt(2.0 / math.pi)
                g = kk * (a + 0.044715 * a ** 3)
                E_g = kk * E_a * (1.0 + 0.134145 * a * a) + 6 * U64 * kk * (np.abs(a) + 0.044715 * np.abs(a) ** 3)
                E_phi = 0.5 * (E_g / np.cosh(np.minimum(np.abs(g), 300.0)) ** 2 + TRANS * np.abs(np.tanh(g)) + 2 * U64)
            E_P = E_P + np.where(used, E_phi, 0.0)
        E_P = E_P + U64 * np.abs(e["P"])
        Pm = np.maximum(e["P"], 1e-12)
        E_term = E_P / Pm + TRANS * np.abs(np.log(Pm))
    dx = xh - X0
    E_dx = E_xh + U64 * np.abs(dx)
    E_dx2 = 2 * np.abs(dx) * E_dx + E_dx ** 2 + U64 * dx * dx
    E_de2 = 3 * U64 * (EP - Z) ** 2
    Bn = X0.shape[0]
    n = X0.reshape(Bn, -1).shape[1]
    red = lambda a: a.reshape(Bn, -1).mean(axis=1)   # noqa: E731
    cols = []
    for j, (f, E, scale) in enumerate(((e["term"], E_term, 1.0 / VR.LN2), (e["dx2"], E_dx2, 1.0), (e["de2"], E_de2, 1.0))):
        b64 = (red(E) + (n + 2) * U64 * red(np.abs(f))) * scale + 2 * U64 * np.abs(want[:, j])
        cols.append(b64 + EPS32 * np.abs(want[:, j]))
    return want, np.stack(cols, axis=1)


def prior_budget(x0, sa_last, sb_last):
    """-> (fp64 [B] prior_bpd from the fp32 operands, its bound).  L = 2 log(sb): 8 U |L|;  exp(L): relative E(L) + 8 U;  m = sa x0, m^2: 3 U m^2;
    the four-term sum: 4 U (1 + |L| + exp(L) + m^2);  then the mean, / ln 2 and the one fp32 rounding as in vlb_budget."""
    want = VR.prior(x0, sa_last, sb_last)
    X0 = np.asarray(x0, np.float64)
    sa, sb = float(np.float32(sa_last)), float(np.float32(sb_last))
    L = 2.0 * math.log(sb)
    eL = math.exp(L)
    E_L = TRANS * abs(L)
    m2 = (sa * X0) ** 2
    f = 0.5 * (-1.0 - L + eL + m2)
    E = 0.5 * (E_L + eL * (E_L + TRANS) + 3 * U64 * m2 + 4 * U64 * (1.0 + abs(L) + eL + m2))
    Bn = X0.shape[0]
    n = X0.reshape(Bn, -1).shape[1]
    red = lambda a: a.reshape(Bn, -1).mean(axis=1)   # noqa: E731
    return want, (red(E) + (n + 2) * U64 * red(np.abs(f))) / VR.LN2 + 2 * U64 * np.abs(want) + EPS32 * np.abs(want)


def test_prior_budget_holds_the_rounded_answer_and_not_a_wrong_one():
    x0 = vlb_operands(257, vlb_cases()[0][1], 5)[0]
    sa, sb = 0.0123, 0.99992
    want, bound = prior_budget(x0, sa, sb)
    assert (np.abs(want.astype(np.float32) - want) <= bound).all() and (bound <= 1.001 * EPS32 * np.abs(want) + 1e-18).all()
    assert (np.abs(VR.prior(np.roll(x0, 1, axis=0), sa, sb) - want) > bound).all()      # another image's data
    assert (np.abs(VR.prior(x0, sb, sa) - want) > bound).all()                          # the two scalars swapped


MODES = [(learned, cdf, clip) for learned in (True, False) for cdf in ("exact", "tanh") for clip in (True, False)]


@pytest.mark.parametrize("per", PERS)
def test_budget_operands_hit_the_hard_branches_and_mutants_break_it(per):
    cases = vlb_cases()
    assert [k for k, _ in cases] == [0, 1, 3, 6] and all(math.isfinite(t) for _, sc in cases for t in sc.values())
    broke = dict(next_image=0, clamped=0, swapped=0, unclipped=0, no_floor=0)
    tried = dict(broke)
    worst = 0.0
    for j, (k, sc) in enumerate(cases):
        x0, xk, eps, v, z = vlb_operands(per, sc, 700 * j + per)
        for learned, cdf, clip in MODES:
            kw = dict(k_is_zero=k == 0, learned=learned, cdf=cdf, clip=clip)
            cen = operand_census(x0, xk, eps, v, z, sc, **kw)
            assert cen["minus_one"] >= 1 and cen["plus_one"] >= 1 and cen["on_grid"] == B * per and cen["clipped"] >= 1 and cen["v_outside"] >= 1, cen
            assert k != 0 or cen["floor"] >= 1, cen
            want, bound = vlb_budget(x0, xk, eps, v, z, sc, **kw)
            assert np.isfinite(want).all() and np.isfinite(bound).all() and (bound > 0).all()
            # the fp64 answer rounded once is inside; so is the fp64 answer of a reordered evaluation (per-image sums taken back to front)
            got32 = want.astype(np.float32).astype(np.float64)
            rev = VR.terms(x0[:, ::-1].copy(), xk[:, ::-1].copy(), eps[:, ::-1].copy(), v[:, ::-1].copy(), z[:, ::-1].copy(), sc, **kw)
            worst = max(worst, float((np.abs(got32 - want) / bound).max()), float((np.abs(rev.astype(np.float32) - want) / bound).max()))
            # ... and a wrong kernel is outside
            mutants = {}
            if learned:
                mutants["next_image"] = VR.terms(x0, xk, eps, np.roll(v, 1, axis=0), z, sc, **kw)
                mutants["clamped"] = VR.terms(x0, xk, eps, np.clip(v, -1, 1), z, sc, **kw)
                mutants["swapped"] = VR.terms(x0, xk, eps, v, z, dict(sc, min_log=sc["max_log"], max_log=sc["min_log"]), **kw)
            if clip:
                mutants["unclipped"] = VR.terms(x0, xk, eps, v, z, sc, **dict(kw, clip=False))
            if k == 0:
                e = VR.elements(x0, xk, eps, v, z, sc, **kw)
                with np.errstate(divide="ignore"):
                    nf = (-np.log(np.maximum(e["P"], 1e-300))).reshape(B, -1).mean(axis=1) / VR.LN2
                mutants["no_floor"] = np.stack((nf, want[:, 1], want[:, 2]), axis=1)
            for name, bad in mutants.items():
                tried[name] += 1
                broke[name] += bool((np.abs(bad - want) > bound).any())
    print(f"per = {per}: vlb terms, rounded fp64 and reordered fp64: max err / budget {worst:.3f}; mutants outside the budget: {broke} of {tried}")
    assert worst <= 1.0
    assert all(broke[m] == tried[m] and tried[m] > 0 for m in broke), (broke, tried)


def test_budget_is_a_rounding_budget_not_a_tolerance():
    """Away from the floor the bound is a few fp32 roundings of the result: the fp64 part does not dominate."""
    (k0, sc0), (k1, sc1) = vlb_cases()[:2]
    for k, sc in ((k0, sc0), (k1, sc1)):
        x0, xk, eps, v, z = vlb_operands(257, sc, 99)
        want, bound = vlb_budget(x0, xk, eps, v, z, sc, k_is_zero=k == 0, learned=True, cdf="exact", clip=True)
        assert (bound <= 2 * EPS32 * np.abs(want) + 1e-30).all(), (k, bound / np.abs(want))


# ---- 3. host logic ----------------------------------------------------------------------------------------------------------------------------------------

def _chains():
    from image_diffusion.sde_diffusion import DDPM, cosine_betas

    d = _ddpm(100)
    return {"plain": d, "from_betas": DDPM.from_betas(cosine_betas(50), time_scale=50), "respaced": d.respace(STEPS7),
            "respaced_learned": d.with_learned_variance().respace(STEPS7)}


@pytest.mark.parametrize("name", ["plain", "from_betas", "respaced", "respaced_learned"])
def test_vlb_log_variances_index_zero_convention(name):
    d = _chains()[name]
    b = d._betas64.numpy() if d._betas64 is not None else d.betas.double().numpy()
    T = VR.tables_from_betas(b)
    pv = T["posterior_variance"]
    small = np.log(np.concatenate(([pv[1]], pv[1:])))
    large = np.log(np.concatenate(([pv[1]], b[1:])))
    fs, fl, le = (d.vlb_log_variances(kind) for kind in ("fixed_small", "fixed_large", "learned"))
    assert sorted(fs) == sorted(fl) == ["model_log", "true_log"] and sorted(le) == ["max_log", "min_log", "true_log"]
    for t in list(fs.values()) + list(fl.values()) + list(le.values()):
        assert t.dtype == torch.float32 and t.device.type == "cpu" and tuple(t.shape) == (d.Ns,) and bool(torch.isfinite(t).all())
    for got, want in ((fs["true_log"], small), (fs["model_log"], small), (fl["true_log"], small), (fl["model_log"], large), (le["true_log"], small),
                      (le["min_log"], small)):
        assert np.array_equal(got.numpy(), want.astype(np.float32)), name
    assert torch.equal(le["max_log"], d.max_log())
    # entry 0 is entry 1's posterior variance, not the samplers' log(1e-20) clip, which stays where it was
    assert fs["true_log"][0] == fs["true_log"][1] and fl["model_log"][0] == fs["true_log"][1] and float(fs["true_log"][0]) > -20.0
    assert float(d.posterior_log_variance_clipped[0]) == pytest.approx(math.log(1e-20), rel=1e-6)
    assert float(le["max_log"][0]) == pytest.approx(math.log(b[0]), rel=1e-6)


def test_python_refusals():
    from image_diffusion import bound, loss_functions, sampling
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance, Replacement
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM

    d = _ddpm(100)
    lik = InPainting(patch_size=6, pad_value=-2)
    net = lambda x, t: x   # noqa: E731
    em = sampling.make_eps_model(net, d)
    with pytest.raises(ValueError, match="kind must be"):
        d.vlb_log_variances("fixed")
    with pytest.raises(ValueError, match="at least 2 steps"):
        DDPM.from_betas([0.1]).vlb_log_variances("fixed_small")
    with pytest.raises(ValueError, match="at least 2 steps"):
        d.respace([40]).vlb_log_variances("learned")
    with pytest.raises(ValueError, match="at least 2 steps"):
        bound.get_vlb_fn(em, d.respace([40]))
    for view, pair in ((d.with_x0_shaping(dynamic_threshold=0.99), "x0_shaping"), (d.with_tiling(sampling.Tiling(stride=8)), "tiling"),
                       (d.with_feature_cache(sampling.FeatureCache(interval=2)), "feature_cache")):
        with pytest.raises(NotImplementedError, match=f"get_vlb_fn with {pair}"):
            bound.get_vlb_fn(em, view)
        with pytest.raises(NotImplementedError, match=f"get_vlb_fn with {pair}"):
            bound.get_vlb_fn(em, view.respace(10))
    with pytest.raises(NotImplementedError, match="get_vlb_fn with guidance_scale"):
        bound.get_vlb_fn(em, d, ClassifierFreeGuidance(1.0, 0, 0.1, 2.0), lik)
    with pytest.raises(ValueError, match="variance must be one of"):
        bound.get_vlb_fn(em, d, variance="small")
    with pytest.raises(ValueError, match="cdf must be"):
        bound.get_vlb_fn(em, d, cdf="erf")
    with pytest.raises(ValueError, match="needs the likelihood"):
        bound.get_vlb_fn(em, d, Amortized(1.0, 0, 0.1))
    # an untagged callable, CPU tensors: the fused loop is the only path
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(NotImplementedError, match="make_eps_model"):
        bound.get_vlb_fn(lambda xi, i: xi, d)(x)
    with pytest.raises(NotImplementedError, match="make_eps_model"):
        bound.get_vlb_fn(em, d)(x)
    # the default variance follows the chain
    import inspect

    p = inspect.signature(bound.get_vlb_fn).parameters
    assert list(p) == ["eps_model", "ddpm", "conditioning", "likelihood", "variance", "cdf", "clip_denoised"]
    assert p["variance"].default is None and p["cdf"].default == "exact" and p["clip_denoised"].default is True
    assert bound.VLBResult._fields == ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")
    # the loss functions
    loss, em2 = loss_functions.get_loss_function(net, d, Replacement(0.1, 1.0, True, 0), lik)
    assert em2._mi355_Ns == d.Ns
    with pytest.raises(ValueError, match="use_condition belongs to Amortized"):
        loss(x, use_condition=True)
    with pytest.raises(ValueError, match="i must have shape"):
        loss(x, i=torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError, match="i must lie in"):
        loss(x, i=torch.tensor([0, 100]))
    with pytest.raises(ValueError, match="noise must have x's shape"):
        loss(x, i=torch.tensor([0, 5]), noise=torch.zeros(2, 1, 8, 8))
    assert "no autograd graph" in loss_functions.get_loss_function.__doc__


def test_engine_ops_and_evaluate_signatures():
    import inspect

    import evaluation
    from mi355.engine import UNetEngine
    from mi355.ops import Ops

    p = inspect.signature(UNetEngine.ddpm_vlb).parameters
    assert list(p)[:4] == ["self", "x0", "tables", "logs"]
    for name, default in (("times", None), ("cond", None), ("y", None), ("noise", None), ("seed", None), ("cdf", "exact"), ("clip_denoised", True)):
        assert p[name].default == default and p[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert p["learned"].kind is inspect.Parameter.KEYWORD_ONLY and p["learned"].default is inspect.Parameter.empty
    assert hasattr(Ops, "vlb_terms") and hasattr(Ops, "vlb_prior") and hasattr(Ops, "q_sample")
    q = inspect.signature(evaluation.evaluate).parameters
    assert q["vlb_fn"].default is None and q["metrics"].default == ("mse", "lpips")
    with pytest.raises(ValueError, match="unknown metrics"):
        evaluation.evaluate(None, None, [], "/nonexistent", metrics=("bits",))


def _tables_c(d):
    from mi355 import _lib

    T = d.host_tables()
    tb = _lib.DDPMTablesC()
    fp = C.POINTER(C.c_float)
    for name, _ in _lib.DDPMTablesC._fields_[1:]:
        setattr(tb, name, C.cast(T[name].data_ptr(), fp))
    tb.Ns = d.Ns
    return tb, T


def test_library_refusals_name_their_argument():
    from mi355 import _lib

    L = _lib.lib()
    for name in ("mi355_ddpm_vlb_workspace_bytes", "mi355_ddpm_vlb", "mi355_vlb_terms", "mi355_vlb_prior", "mi355_q_sample"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.mi355_version() == 108
    d = _ddpm(100).respace(STEPS7).with_learned_variance()
    tb, keep = _tables_c(d)
    fp = C.POINTER(C.c_float)
    logs = {**d.vlb_log_variances("fixed_large"), **d.vlb_log_variances("learned")}
    good_t = [d.time(k) for k in range(d.Ns)]
    nan, inf = float("nan"), float("inf")

    def opt(learned=1, cdf=0, clip=1, times=None, **over):
        o = _lib.VLBOptionsC(learned, cdf, clip, None, None, None, None, None, -2.0, 0)
        o._keep = {}
        for name in ("true_log", "model_log", "min_log", "max_log"):
            v = over.get(name, logs[name])
            if v is not None:
                o._keep[name] = torch.as_tensor(v, dtype=torch.float32).clone()
                setattr(o, name, C.cast(o._keep[name].data_ptr(), fp))
        if times is not None:
            o._keep["times"] = torch.tensor(times, dtype=torch.float32)
            o.times = C.cast(o._keep["times"].data_ptr(), fp)
        return o

    def call(o, tables=tb, n_draws=0, noise=None):
        return L.mi355_ddpm_vlb(None, None, 1, None, None, C.byref(tables) if tables is not None else None, C.byref(o) if o is not None else None, noise,
                                n_draws, None, None, 3, None, 0, None)

    def bad(t, k, val):
        t = t.clone()
        t[k] = val
        return t

    cases = [(opt(learned=2), b"opt->learned"), (opt(learned=-1), b"opt->learned"), (opt(cdf=2), b"opt->cdf"), (opt(clip=3), b"opt->clip_denoised"),
             (opt(true_log=None), b"opt->true_log is null"), (opt(learned=0, model_log=None), b"opt->model_log is null"),
             (opt(min_log=None), b"opt->min_log is null"), (opt(max_log=None), b"opt->max_log is null"),
             (opt(true_log=bad(logs["true_log"], 3, nan)), b"opt->true_log must be finite"),
             (opt(learned=0, model_log=bad(logs["model_log"], 0, -inf)), b"opt->model_log must be finite"),
             (opt(min_log=bad(logs["min_log"], 6, inf)), b"opt->min_log must be finite"), (opt(max_log=bad(logs["max_log"], 1, nan)), b"opt->max_log must be finite"),
             (opt(times=good_t[:2] + [nan] + good_t[3:]), b"opt->times must be finite")]
    for o, msg in cases:
        assert call(o) == -1 and msg in L.mi355_last_error() and b"ddpm_vlb" in L.mi355_last_error(), (msg, L.mi355_last_error())
    # a table the mode does not read may be missing or hold anything: the next refusal is the missing handle
    for o in (opt(learned=1, model_log=None), opt(learned=0, min_log=None, max_log=None), opt(learned=0, max_log=bad(logs["max_log"], 2, nan)),
              opt(times=good_t)):
        assert call(o) == -1 and b"ddpm_vlb: net is null" in L.mi355_last_error(), L.mi355_last_error()
    assert call(None) == -1 and b"ddpm_vlb: opt is null" in L.mi355_last_error()
    assert call(opt(), tables=None) == -1 and b"ddpm_vlb: tables is null" in L.mi355_last_error()
    one, keep1 = _tables_c(_ddpm(100).respace([40]))
    assert call(opt(), tables=one) == -1 and b"tables->Ns must be >= 2" in L.mi355_last_error()
    # the chain tables are read too: DDPM(Ns <= 20) leaves them non-finite
    quirk, keep2 = _tables_c(_ddpm(20))
    o20 = opt(**{n: torch.zeros(20) for n in ("true_log", "model_log", "min_log", "max_log")})
    assert call(o20, tables=quirk) == -1 and b"ddpm_vlb: tables->" in L.mi355_last_error() and b"must be finite" in L.mi355_last_error()
    assert L.mi355_ddpm_vlb_workspace_bytes(None, 3) == -1 and b"ddpm_vlb_workspace_bytes" in L.mi355_last_error()
    # the ops refuse before they look at a pointer
    def terms(batch=3, per=16, stride=32, off=0, k0=0, learned=1, cdf=0, clip=1, sc=(1.0, 0.5, 0.5, 0.5, -3.0, -3.0, -3.0, -1.0), dstride=3, philox=1):
        return L.mi355_vlb_terms(None, None, None, stride, None, philox, 0, off, *sc, k0, learned, cdf, clip, None, dstride, batch, per, None)

    for kw, msg in ((dict(k0=2), b"k_is_zero"), (dict(learned=2), b"vlb_terms: learned"), (dict(cdf=-1), b"vlb_terms: cdf"), (dict(clip=2), b"clip_denoised"),
                    (dict(per=0), b"elems_per_image"), (dict(batch=-1), b"batch"), (dict(stride=31), b"out_stride"), (dict(learned=0, stride=15), b"out_stride"),
                    (dict(dstride=2), b"dst_stride"), (dict(off=6), b"the Philox offset"),
                    (dict(sc=(nan, 0.5, 0.5, 0.5, -3.0, -3.0, -3.0, -1.0)), b"c_recip"), (dict(sc=(1.0, 0.5, 0.5, 0.5, inf, -3.0, -3.0, -1.0)), b"true_log"),
                    (dict(sc=(1.0, 0.5, 0.5, 0.5, -3.0, -3.0, nan, -1.0)), b"min_log and max_log"),
                    (dict(learned=0, stride=16, sc=(1.0, 0.5, 0.5, 0.5, -3.0, nan, -3.0, -1.0)), b"model_log"), (dict(), b"vlb_terms: null argument")):
        assert terms(**kw) == -1 and msg in L.mi355_last_error(), (kw, L.mi355_last_error())
    # a scalar the mode does not read may be anything; an empty batch asks for no pointer
    assert terms(batch=0, sc=(1.0, 0.5, 0.5, 0.5, -3.0, nan, -3.0, -1.0)) == 0
    assert terms(batch=0, learned=0, stride=16, sc=(1.0, 0.5, 0.5, 0.5, -3.0, -3.0, nan, nan)) == 0
    prior = lambda sa=0.01, sb=0.99, K=0, stride=0, batch=3, per=16, terms=None: L.mi355_vlb_prior(None, sa, sb, terms, stride, K, None, batch, per, None)  # noqa: E731
    for kw, msg in ((dict(per=0), b"elems_per_image"), (dict(sa=nan), b"sqrt_alphas_cumprod"), (dict(sb=0.0), b"sqrt_one_minus_alphas_cumprod"),
                    (dict(sb=inf), b"sqrt_one_minus_alphas_cumprod"), (dict(), b"vlb_prior: null argument")):
        assert prior(**kw) == -1 and msg in L.mi355_last_error(), (kw, L.mi355_last_error())
    hold = torch.zeros(4)
    assert prior(terms=C.c_void_p(hold.data_ptr()), K=2, stride=5) == -1 and b"terms_stride" in L.mi355_last_error()
    assert prior(batch=0) == 0
    assert L.mi355_q_sample(None, None, None, 1.0, 0.5, 1, 0, 2, 16, None) == -1 and b"q_sample: the Philox offset" in L.mi355_last_error()
    assert L.mi355_q_sample(None, None, None, 1.0, 0.5, 1, 0, 0, 16, None) == -1 and b"q_sample: null argument" in L.mi355_last_error()
    del keep, keep1, keep2
