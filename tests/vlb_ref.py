"""fp64 restatement of the variational bound of a DDPM net (mi355_ddpm_vlb, image_diffusion.bound) and of the denoising loss
(image_diffusion.loss_functions).  Pure numpy / torch on the CPU, written from the definitions (Ho et al. 2020, eq. 5 and the decoder of
section 3.3; Nichol & Dhariwal 2021, eq. 15):

    x_k      = fl32(fl32(sa[k] x0) + fl32(sb[k] z_k))                z_k = draw number K-1-k
    out      = net(x_k [| cond], time_k);  eps = out[:, :C], v = out[:, C:2C]
    x0_hat   = c_recip[k] x_k - c_recipm1[k] eps   (clipped to [-1, 1] iff clip_denoised)
    mean_p   = coef1[k] x0_hat + coef2[k] x_k;     mean_q = coef1[k] x0 + coef2[k] x_k
    lq       = true_log[k];   lp = model_log[k], or learned: frac max_log[k] + (1 - frac) min_log[k], frac = (v + 1) / 2
    k > 0    kl = 0.5 (-1 + lp - lq + exp(lq - lp) + (mean_q - mean_p)^2 exp(-lp));   vb = mean(kl) / ln 2
    k == 0   c = x0 - mean_p, s = exp(-0.5 lp), a+- = s (c +- 1/255);  P = Phi(a+) | 1 - Phi(a-) | Phi(a+) - Phi(a-) for x0 < -0.999 | x0 > 0.999 |
             otherwise;  vb = mean(-log(max(P, 1e-12))) / ln 2
    xstart_mse = mean((x0_hat - x0)^2);  mse = mean((eps - z_k)^2)
    prior    = mean(0.5 (-1 - L + exp(L) + (sa[K-1] x0)^2)) / ln 2,  L = 2 log(sb[K-1])
    total    = sum_k fl32(vb[k]) + fl32(prior)

Phi exact: 0.5 erfc(-a / sqrt 2), every probability taken where the values are at most 0.5 (1 - Phi(a) as Phi(-a); right of the mean the inner
bin as Phi(-a-) - Phi(-a+)).  Phi tanh: 0.5 (1 + tanh(sqrt(2 / pi) (a + 0.044715 a^3))) in the three expressions verbatim.
"""
import math

import numpy as np
import torch

from tests.learned_variance_ref import tables_from_betas  # noqa: F401  (re-exported: the chain tables in fp64)

LN2 = math.log(2.0)
SCALARS = ("c_recip", "c_recipm1", "coef1", "coef2", "true_log", "model_log", "min_log", "max_log")


def erfc(y):
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(np.asarray(y, np.float64)))).numpy()


def phi_exact(a):
    return 0.5 * erfc(-np.asarray(a, np.float64) / math.sqrt(2.0))


def phi_tanh(a):
    a = np.asarray(a, np.float64)
    return 0.5 * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (a + 0.044715 * (a * a * a))))


def bin_probability(x0, mean_p, lp, cdf="exact"):
    """P of the 8-bit bin around x0 (open-ended at the two edge pixels) under N(mean_p, exp(lp)), before the 1e-12 floor; fp64 arrays."""
    x0, mean_p, lp = (np.asarray(t, np.float64) for t in (x0, mean_p, lp))
    c = x0 - mean_p
    s = np.exp(-0.5 * lp)
    ap, am = s * (c + 1.0 / 255.0), s * (c - 1.0 / 255.0)
    if cdf == "exact":
        inner = np.where(c > 0.0, phi_exact(-am) - phi_exact(-ap), phi_exact(ap) - phi_exact(am))
        return np.where(x0 < -0.999, phi_exact(ap), np.where(x0 > 0.999, phi_exact(-am), inner))
    assert cdf == "tanh"
    return np.where(x0 < -0.999, phi_tanh(ap), np.where(x0 > 0.999, 1.0 - phi_tanh(am), phi_tanh(ap) - phi_tanh(am)))


def kl_normal(mean_q, lq, mean_p, lp):
    return 0.5 * (-1.0 + lp - lq + np.exp(lq - lp) + (mean_q - mean_p) ** 2 * np.exp(-lp))


def elements(x0, x_k, eps, v, z, sc, *, k_is_zero, learned, cdf="exact", clip=True):
    """The per-element quantities in fp64 from the fp32 operands (arrays of one shape; v is read iff learned) -> dict with "x0_hat", "mean_p",
    "lp", "term" (the KL, or -log p at k == 0), "P" (k == 0: the probability before the floor), "dx2", "de2"."""
    x0, x_k, eps, z = (np.asarray(t, np.float64) for t in (x0, x_k, eps, z))
    c = {n: float(np.float32(sc[n])) for n in SCALARS if n in sc}
    xh = c["c_recip"] * x_k - c["c_recipm1"] * eps
    if clip:
        xh = np.where(xh < -1.0, -1.0, np.where(xh > 1.0, 1.0, xh))
    mean_p = c["coef1"] * xh + c["coef2"] * x_k
    if learned:
        frac = (np.asarray(v, np.float64) + 1.0) / 2.0
        lp = frac * c["max_log"] + (1.0 - frac) * c["min_log"]
    else:
        lp = np.full_like(x0, c["model_log"])
    out = {"x0_hat": xh, "mean_p": mean_p, "lp": lp}
    if k_is_zero:
        P = bin_probability(x0, mean_p, lp, cdf)
        out["P"] = P
        out["term"] = -np.log(np.maximum(P, 1e-12))
    else:
        mean_q = c["coef1"] * x0 + c["coef2"] * x_k
        out["term"] = kl_normal(mean_q, c["true_log"], mean_p, lp)
    out["dx2"] = (xh - x0) ** 2
    out["de2"] = (eps - z) ** 2
    return out


def terms(x0, x_k, eps, v, z, sc, *, k_is_zero, learned, cdf="exact", clip=True):
    """[B, ...] operands -> fp64 [B, 3] = vb (bits/dim), xstart_mse, mse of every image."""
    e = elements(x0, x_k, eps, v, z, sc, k_is_zero=k_is_zero, learned=learned, cdf=cdf, clip=clip)
    B = np.asarray(x0).shape[0]
    red = lambda a: a.reshape(B, -1).mean(axis=1)   # noqa: E731
    return np.stack((red(e["term"]) / LN2, red(e["dx2"]), red(e["de2"])), axis=1)


def prior(x0, sa_last, sb_last):
    """fp64 [B]: KL(q(x_K | x0) || N(0, 1)) in bits/dim."""
    x0 = np.asarray(x0, np.float64)
    sa, sb = float(np.float32(sa_last)), float(np.float32(sb_last))
    L = 2.0 * math.log(sb)
    return (0.5 * (-1.0 - L + math.exp(L) + (sa * x0) ** 2)).reshape(x0.shape[0], -1).mean(axis=1) / LN2


def q_sample32(x0, z, sa, sb):
    """fl32(fl32(sa x0) + fl32(sb z)): numpy float32 arithmetic rounds every operation."""
    f = np.float32
    return (f(sa) * np.asarray(x0, f) + f(sb) * np.asarray(z, f)).astype(f)


def loop(out_fn, T, logs, x0, noise, *, learned, cdf="exact", clip=True, cond=None, none_value=-2.0, amortized=False):
    """The bound of one batch.  out_fn(net_in, k): the network's output at step k, a torch tensor [B, C or 2C, H, W] (net_in fp32 torch: x_k, or
    x_k | cond, or x_k | none_value under amortized without cond).  T: the chain's tables (name -> [K]), logs: name -> [K] (true_log, model_log or
    min_log and max_log).  x0 [B, C, H, W], noise [>= K, B, C, H, W] (torch or numpy, fp32).
    -> dict of fp64 arrays: total_bpd [B], prior_bpd [B], vb, xstart_mse, mse [B, K]."""
    x0 = np.asarray(x0, np.float32)
    noise = np.asarray(noise, np.float32)
    T = {k: np.asarray(t, np.float32) for k, t in T.items()}
    logs = {k: np.asarray(t, np.float32) for k, t in logs.items()}
    K = len(T["sqrt_alphas_cumprod"])
    B, C = x0.shape[:2]
    cnd = None
    if cond is not None:
        cnd = np.asarray(cond, np.float32)
    elif amortized:
        cnd = np.full_like(x0, none_value)
    out = {n: np.zeros((B, K)) for n in ("vb", "xstart_mse", "mse")}
    for k in reversed(range(K)):
        z = noise[K - 1 - k]
        xk = q_sample32(x0, z, T["sqrt_alphas_cumprod"][k], T["sqrt_one_minus_alphas_cumprod"][k])
        net_in = torch.from_numpy(xk if cnd is None else np.concatenate((xk, cnd), axis=1))
        o = np.asarray(out_fn(net_in, k).detach().cpu().numpy(), np.float32)
        sc = dict(c_recip=T["sqrt_recip_alphas_cumprod"][k], c_recipm1=T["sqrt_recipm1_alphas_cumprod"][k], coef1=T["posterior_mean_coef1"][k],
                  coef2=T["posterior_mean_coef2"][k], true_log=logs["true_log"][k])
        if learned:
            sc.update(min_log=logs["min_log"][k], max_log=logs["max_log"][k])
        else:
            sc.update(model_log=logs["model_log"][k])
        t = terms(x0, xk, o[:, :C], o[:, C:2 * C] if learned else None, z, sc, k_is_zero=k == 0, learned=learned, cdf=cdf, clip=clip)
        out["vb"][:, k], out["xstart_mse"][:, k], out["mse"][:, k] = t[:, 0], t[:, 1], t[:, 2]
    out["prior_bpd"] = prior(x0, T["sqrt_alphas_cumprod"][K - 1], T["sqrt_one_minus_alphas_cumprod"][K - 1])
    out["total_bpd"] = out["vb"].astype(np.float32).astype(np.float64).sum(axis=1) + out["prior_bpd"].astype(np.float32).astype(np.float64)
    return out


def loss(out_fn, T, x, i, noise, cond=None):
    """The denoising loss mean_b mean((eps_hat - noise)^2) in fp64.  out_fn(net_in, i): the network's output for the per-image steps i ([B] ints);
    the noising is the fp32 one (per-image sa[i], sb[i]); cond: concatenated behind x_i."""
    x, noise = np.asarray(x, np.float32), np.asarray(noise, np.float32)
    i = np.asarray(i, np.int64)
    shape = (-1,) + (1,) * (x.ndim - 1)
    sa = np.asarray(T["sqrt_alphas_cumprod"], np.float32)[i].reshape(shape)
    sb = np.asarray(T["sqrt_one_minus_alphas_cumprod"], np.float32)[i].reshape(shape)
    xi = (sa * x + sb * noise).astype(np.float32)
    net_in = torch.from_numpy(xi if cond is None else np.concatenate((xi, np.asarray(cond, np.float32)), axis=1))
    eps_hat = np.asarray(out_fn(net_in, i).detach().cpu().numpy(), np.float64)
    return float(((eps_hat - noise.astype(np.float64)) ** 2).reshape(x.shape[0], -1).mean(axis=1).mean())
