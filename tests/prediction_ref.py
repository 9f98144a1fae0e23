"""fp64 restatement of sampling and scoring x0- and v-prediction DDPM nets (DDPM.with_prediction; mi355_ddpm_pred_sample, mi355_ddpm_vlb_pred).
Pure numpy / torch on the CPU, written from the formulas and not by calling the library.

A chain has a prediction kind.  With `out` the network output for the state x at step i (under classifier-free guidance the mix
out_u + w (out_c - out_u) of the raw outputs, under guidance rescale then scaled by f_b) the unclipped data prediction is

    eps : x0_pre = c_recip x - c_recipm1 out
    x0  : x0_pre = out                                   (x is not read)
    v   : x0_pre = sa x - sb out                         sa = sqrt_alphas_cumprod[i], sb = sqrt_one_minus_alphas_cumprod[i]

and everything behind it is the samplers' own:

    x0_hat     = clip(x0_pre, -1, 1), or clip(x0_pre, -s_b, s_b) / s_b with the image's row (f_b, s_b)
    ancestral  : x <- coef1 x0_hat + coef2 x + sigma z              sigma = exp(0.5 logvar); logvar the table's (fixed small: the clipped posterior
                 log-variance; fixed large: log(beta_i) for i >= 1), or learned: frac max_log + (1 - frac) min_log, frac = (var + 1) / 2 with var
                 the net's second half; step 0 adds no noise
    DDIM(eta)  : e2 = (c_recip x - x0_hat) / c_recipm1;  x <- sqrt(prev) x0_hat + sqrt(max(1 - prev - sigma^2, 0)) e2 + sigma z
    DPM-Solver++ : x <- cx x + c0 x0_hat + c1 hist;  hist <- x0_hat
    corrector  : x <- x + (0.5 dt delta (-rsm1 clip(x0_pre, -1, 1)) + sqrt(dt delta) z)

In the bound, x0_hat comes from x0_pre of the kind and mse = mean((out - target)^2) with target = z (eps), x0 (x0), sa z - sb x0 (v).
"""
import math

import numpy as np
import torch

from tests import vlb_ref as VR

KINDS = ("eps", "x0", "v")


def x0_pre(pred, x, out, cr, crm1, sa, sb):
    """The unclipped data prediction of the kind, in the dtype of the operands (numpy arrays or torch tensors)."""
    if pred == "eps":
        return cr * x - crm1 * out
    if pred == "x0":
        return out
    assert pred == "v", pred
    return sa * x - sb * out


def mix(out_c, out_u, w):
    return out_u + w * (out_c - out_u)


def _clip(a, lo, hi):
    if isinstance(a, torch.Tensor):
        return torch.maximum(torch.minimum(a, torch.as_tensor(hi, dtype=a.dtype)), torch.as_tensor(lo, dtype=a.dtype))   # a NaN stays one
    return np.where(np.isnan(a), a, np.clip(a, lo, hi))


def x0_hat(pre, s=None):
    """clip(pre, -1, 1), or with the per-element threshold s: clip(pre, -s, s) / s."""
    if s is None:
        return _clip(pre, -1.0, 1.0)
    return _clip(pre, -s, s) / s


def step(kind, pred, x, out, c, *, sa=0.0, sb=0.0, z=None, hist=None, var=None, f=None, s=None):
    """One step of `kind` on numpy fp64 operands.  c: ("ddpm": cr, crm1, coef1, coef2, sigma), ("ddpm_lv": cr, crm1, coef1, coef2, min_log, max_log;
    var = the variance channel), ("ddim" / "ddim_eta": cr, crm1, prev, sigma), ("dpmpp": cr, crm1, cx, c0, c1), ("corrector": cr, crm1, rsm1, dt,
    delta).  f, s: per-element rows (None: the static clip).  -> (x_new, x0_hat)"""
    cr, crm1 = c[0], c[1]
    o = out if f is None else f * out
    xh = x0_hat(x0_pre(pred, x, o, cr, crm1, sa, sb), s)
    if kind == "ddpm":
        m = c[2] * xh + c[3] * x
        return (m if z is None else m + c[4] * z), xh
    if kind == "ddpm_lv":
        frac = (var + 1.0) * 0.5
        logvar = frac * c[5] + (1.0 - frac) * c[4]
        m = c[2] * xh + c[3] * x
        return (m if z is None else m + np.exp(0.5 * logvar) * z), xh
    if kind in ("ddim", "ddim_eta"):
        prev, sg = c[2], c[3]
        e2 = (cr * x - xh) / crm1
        m = math.sqrt(prev) * xh + math.sqrt(max(1.0 - prev - sg * sg, 0.0)) * e2
        return (m if z is None else m + sg * z), xh
    if kind == "dpmpp":
        m = c[2] * x + c[3] * xh
        return (m + c[4] * hist if c[4] != 0.0 else m), xh
    assert kind == "corrector", kind
    score = -c[2] * xh
    return x + (0.5 * c[3] * c[4] * score + math.sqrt(c[3] * c[4]) * z), xh


def _per_image(w, like):
    return w.double().reshape(-1, *([1] * (like.dim() - 1))) if isinstance(w, torch.Tensor) else float(w)


def sample(out, T, pred, xT, noise, *, sampler="ancestral", max_log=None, ddim_sigma=None, coefs=None, cond=None, amortized=False, none_value=-2.0,
           w=None, n_corrector=0, delta=0.1, tmin=1e-5, tmax=1.0, replacement=None, walk=None):
    """The loops in fp64 (torch).  out(net_in, k): the net's output at step k ([B, C, H, W]; [B, 2C, H, W] with max_log: prediction | variance).
    sampler: "ancestral" (T's own posterior_log_variance_clipped: fixed small or large; max_log: the learned range), "ddim" (ddim_sigma None: the
    deterministic step), "dpmpp" (coefs = (cx, c0, c1)).  cond / amortized / w: as tests.learned_variance_ref.sample.  replacement: dict(cond,
    start_fraction, noise, pad) - the paste before the predictor of step i < int(K * start_fraction).  walk: levels K..0 by +-1 (RePaint); an
    upward move L -> L + 1 is x <- sqrt(alphas[L]) x + sqrt(betas[L]) z.  -> (x0 clipped, draws used, evaluations)"""
    T = {k: np.asarray(v, np.float64) for k, v in T.items()}
    K = len(T["alphas_cumprod_prev"])
    x = xT.double().clone()
    C = x.shape[1]
    none = torch.full_like(x, none_value) if (cond is not None or amortized) and replacement is None else None
    cond64 = none if (cond is None or replacement is not None) else cond.double()
    used = n_eval = 0
    hist = None

    def net(c, k):
        nonlocal n_eval
        n_eval += 1
        return out(x if c is None else torch.cat((x, c), dim=-3), k).double()

    def draw():
        nonlocal used
        used += 1
        return noise[used - 1].double()

    dt = (tmax - tmin) / K

    def down(i):
        nonlocal x, hist
        cr, crm1 = float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i])
        sa, sb = float(T["sqrt_alphas_cumprod"][i]), float(T["sqrt_one_minus_alphas_cumprod"][i])
        if replacement is not None and i < int(K * replacement["start_fraction"]):
            c64 = replacement["cond"].double()
            noised = sa * c64 + sb * draw() if replacement["noise"] else c64
            x = torch.where(c64 == replacement["pad"], x, noised)
        oc = net(cond64, i)
        o, var = oc[:, :C], oc[:, C:]
        if w is not None:
            o = mix(o, net(none, i)[:, :C], _per_image(w, x))
        xh = x0_hat(x0_pre(pred, x, o, cr, crm1, sa, sb))
        if sampler == "dpmpp":
            cx, c0, c1 = (float(c[i]) for c in coefs)
            x = cx * x + c0 * xh + (c1 * hist if c1 != 0.0 else 0.0)
            hist = xh
            return
        if sampler == "ddim":
            prev = float(T["alphas_cumprod_prev"][i])
            sg = 0.0 if ddim_sigma is None else float(ddim_sigma[i])
            e2 = (cr * x - xh) / crm1
            x = math.sqrt(prev) * xh + math.sqrt(max(1.0 - prev - sg * sg, 0.0)) * e2
            if ddim_sigma is not None and i > 0:
                x = x + sg * draw()
            return
        mean = float(T["posterior_mean_coef1"][i]) * xh + float(T["posterior_mean_coef2"][i]) * x
        if i > 0:
            min_log = float(T["posterior_log_variance_clipped"][i])
            if max_log is not None:
                frac = (var + 1.0) * 0.5
                logvar = frac * float(max_log[i]) + (1.0 - frac) * min_log
            else:
                logvar = torch.full_like(x, min_log)
            mean = mean + torch.exp(0.5 * logvar) * draw()
        x = mean
        for _ in range(n_corrector):
            e = net(none, i)[:, :C]
            x0c = x0_hat(x0_pre(pred, x, e, cr, crm1, sa, sb))
            score = -float(T["recip_sqrt_m1_alphas_cumprod"][i]) * x0c
            x = x + (0.5 * dt * delta * score + math.sqrt(dt * delta) * draw())

    levels = list(range(K, -1, -1)) if walk is None else list(walk)
    for a, b in zip(levels, levels[1:]):
        if b < a:
            down(a - 1)
        else:
            x = math.sqrt(float(T["alphas"][a])) * x + math.sqrt(float(T["betas"][a])) * draw()
    return x.clamp(-1.0, 1.0), used, n_eval


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------------------

def vlb_terms(pred, x0, x_k, out, v, z, sc, *, sa=0.0, sb=0.0, k_is_zero, learned, cdf="exact", clip=True):
    """[B, ...] fp32 operands -> fp64 [B, 3] = vb (bits/dim), xstart_mse, mse of every image, for a net of the given kind.  sc: the scalars of
    tests.vlb_ref (c_recip, c_recipm1, coef1, coef2, true_log, model_log | min_log, max_log), rounded to fp32 as the library receives them."""
    x0, x_k, out, z = (np.asarray(t, np.float64) for t in (x0, x_k, out, z))
    c = {n: float(np.float32(sc[n])) for n in VR.SCALARS if n in sc}
    sa, sb = float(np.float32(sa)), float(np.float32(sb))
    xh = x0_pre(pred, x_k, out, c["c_recip"], c["c_recipm1"], sa, sb)
    if clip:
        xh = np.where(xh < -1.0, -1.0, np.where(xh > 1.0, 1.0, xh))
    mean_p = c["coef1"] * xh + c["coef2"] * x_k
    if learned:
        frac = (np.asarray(v, np.float64) + 1.0) / 2.0
        lp = frac * c["max_log"] + (1.0 - frac) * c["min_log"]
    else:
        lp = np.full_like(x0, c["model_log"])
    if k_is_zero:
        term = -np.log(np.maximum(VR.bin_probability(x0, mean_p, lp, cdf), 1e-12))
    else:
        term = VR.kl_normal(c["coef1"] * x0 + c["coef2"] * x_k, c["true_log"], mean_p, lp)
    target = {"eps": z, "x0": x0, "v": sa * z - sb * x0}[pred]
    B = x0.shape[0]
    red = lambda a: a.reshape(B, -1).mean(axis=1)   # noqa: E731
    return np.stack((red(term) / VR.LN2, red((xh - x0) ** 2), red((out - target) ** 2)), axis=1)


def vlb_loop(out_fn, T, logs, pred, x0, noise, *, learned, cdf="exact", clip=True):
    """The bound of one batch for a net of the given kind (an unconditional net): tests.vlb_ref.loop with this module's terms.
    -> dict of fp64 arrays: total_bpd [B], prior_bpd [B], vb, xstart_mse, mse [B, K]."""
    x0 = np.asarray(x0, np.float32)
    noise = np.asarray(noise, np.float32)
    T = {k: np.asarray(t, np.float32) for k, t in T.items()}
    logs = {k: np.asarray(t, np.float32) for k, t in logs.items()}
    K = len(T["sqrt_alphas_cumprod"])
    B, C = x0.shape[:2]
    res = {n: np.zeros((B, K)) for n in ("vb", "xstart_mse", "mse")}
    for k in reversed(range(K)):
        z = noise[K - 1 - k]
        sa, sb = T["sqrt_alphas_cumprod"][k], T["sqrt_one_minus_alphas_cumprod"][k]
        xk = VR.q_sample32(x0, z, sa, sb)
        o = np.asarray(out_fn(torch.from_numpy(xk), k).detach().cpu().numpy(), np.float32)
        sc = dict(c_recip=T["sqrt_recip_alphas_cumprod"][k], c_recipm1=T["sqrt_recipm1_alphas_cumprod"][k], coef1=T["posterior_mean_coef1"][k],
                  coef2=T["posterior_mean_coef2"][k], true_log=logs["true_log"][k])
        if learned:
            sc.update(min_log=logs["min_log"][k], max_log=logs["max_log"][k])
        else:
            sc.update(model_log=logs["model_log"][k])
        t = vlb_terms(pred, x0, xk, o[:, :C], o[:, C:2 * C] if learned else None, z, sc, sa=sa, sb=sb, k_is_zero=k == 0, learned=learned, cdf=cdf,
                      clip=clip)
        res["vb"][:, k], res["xstart_mse"][:, k], res["mse"][:, k] = t[:, 0], t[:, 1], t[:, 2]
    res["prior_bpd"] = VR.prior(x0, T["sqrt_alphas_cumprod"][K - 1], T["sqrt_one_minus_alphas_cumprod"][K - 1])
    res["total_bpd"] = res["vb"].astype(np.float32).astype(np.float64).sum(axis=1) + res["prior_bpd"].astype(np.float32).astype(np.float64)
    return res
