"""fp64 restatement of per-image x0 shaping (dynamic thresholding, Saharia et al. 2022, section 2.3; guidance rescale, Lin et al. 2023, section 3.4)
and of the DDPM samplers that carry it.  Written from the formulas, independent of the library: torch / numpy on the CPU only.

Per predictor step and per image b of per = C * H * W elements, with eps_g the plain eps or eps_u + w (eps_c - eps_u):
    sigma_c, sigma_g = population standard deviations of eps_c, eps_g over the image;  f_b = phi sigma_c / sigma_g + (1 - phi)  (1 when
    sigma_g == 0 or phi == 0);  eps' = f_b eps_g;  x0 = c_recip x - c_recipm1 eps';
    pos = p32 (per - 1) with p32 the fp32 value of the quantile, k = floor(pos), frac = float32(pos - k);  lo, hi = the k-th and
    min(k + 1, per - 1)-th smallest of |x0|;  s_raw = lo + frac (hi - lo);  s_b = min(max(s_raw, 1), s_max);  x0_hat = clamp(x0, -s_b, s_b) / s_b.
The position and frac are the library's (the quantile is an fp32 field, frac an fp32 kernel argument); everything else is fp64 here.
"""
import math

import numpy as np
import torch


def position(p, per: int):
    """-> (k, frac): torch.quantile's position p (per - 1) for the fp32 quantile, its floor and its fraction rounded to fp32."""
    pos = float(np.float32(p)) * (per - 1)
    k = min(int(math.floor(pos)), per - 1)
    return k, float(np.float32(pos - k))


def _rows(t):
    return t.reshape(t.shape[0], -1)


def _per_image(v, like):
    """A per-image vector [B] (or a scalar) shaped to broadcast over `like` [B, ...]."""
    if isinstance(v, torch.Tensor) and v.dim() > 0:
        return v.double().reshape(-1, *([1] * (like.dim() - 1)))
    return float(v)


def sigmas(eps_c, eps_g):
    """Population standard deviations per image, fp64: mean first, then the centred sum of squares."""
    out = []
    for e in (eps_c, eps_g):
        r = _rows(e.double())
        d = r - r.mean(dim=1, keepdim=True)
        out.append(torch.sqrt((d * d).sum(dim=1) / r.shape[1]))
    return out


def rescale_factor(eps_c, eps_g, phi):
    """f [B] in fp64; (1 - phi) is the fp32 difference the library's host code forms."""
    B = eps_c.shape[0]
    if not phi:
        return torch.ones(B, dtype=torch.float64)
    sc, sg = sigmas(eps_c, eps_g)
    phi32 = float(np.float32(phi))
    om = float(np.float32(1.0) - np.float32(phi))
    f = phi32 * (sc / sg) + om
    return torch.where(sg == 0, torch.ones_like(f), f)


def threshold(x0, p, s_max=None):
    """-> (s [B], s_raw [B]) in the dtype of x0 (fp64 for the restatement; fp32 in: the stated fp32 interpolation, each operation rounded).
    An image that holds a NaN gets NaN."""
    a = _rows(x0).abs()
    B, per = a.shape
    k, frac = position(p, per)
    srt, _ = torch.sort(a, dim=1)        # NaNs sort last
    lo, hi = srt[:, k], srt[:, min(k + 1, per - 1)]
    fr = torch.tensor(frac, dtype=a.dtype)
    s_raw = lo + fr * (hi - lo)
    s_raw = torch.where(torch.isnan(a).any(dim=1), torch.full_like(s_raw, float("nan")), s_raw)
    s = torch.where(torch.isnan(s_raw), s_raw, s_raw.clamp(min=1.0))
    if s_max:
        s = torch.where(torch.isnan(s), s, s.clamp(max=float(s_max)))
    return s, s_raw


def shaped_x0(x, eps_c, eps_g, c_recip, c_recipm1, shaping):
    """x0_hat in fp64 for shaping = (p or None, s_max or None, phi); None: the static clip.  -> (x0_hat, f [B], s [B])"""
    x, eps_c, eps_g = x.double(), eps_c.double(), eps_g.double()
    B = x.shape[0]
    if shaping is None:
        one = torch.ones(B, dtype=torch.float64)
        return (c_recip * x - c_recipm1 * eps_g).clamp(-1.0, 1.0), one, one
    p, s_max, phi = shaping
    f = rescale_factor(eps_c, eps_g, phi)
    x0 = c_recip * x - c_recipm1 * (_per_image(f, x) * eps_g)
    if not p:
        return x0.clamp(-1.0, 1.0), f, torch.ones(B, dtype=torch.float64)
    s, _ = threshold(x0, p, s_max)
    sv = _per_image(s, x)
    return torch.maximum(torch.minimum(x0, sv), -sv) / sv + 0.0 * sv, f, s   # + 0 s: a NaN threshold makes the whole image NaN


def apply_rows(x, eps, f, s, c_recip, c_recipm1):
    """x0_hat from given rows (f, s) [B]: clamp(c_recip x - c_recipm1 (f eps), -s, s) / s, in the dtype of the operands."""
    fv, sv = (v.reshape(-1, *([1] * (x.dim() - 1))) for v in (f, s))
    x0 = c_recip * x - c_recipm1 * (fv * eps)
    return torch.maximum(torch.minimum(x0, sv), -sv) / sv


# ---- the four predictor steps on a given x0_hat (fp64 when fed fp64) ----
def ancestral_from_x0(x0, x, z, coef1, coef2, sigma):
    mean = coef1 * x0 + coef2 * x
    return mean if z is None else mean + sigma * z


def ddim_from_x0(x0, x, z, c_recip, c_recipm1, acp_prev, sigma):
    e2 = (c_recip * x - x0) / c_recipm1
    out = math.sqrt(acp_prev) * x0 + math.sqrt(max(1.0 - acp_prev - sigma * sigma, 0.0)) * e2
    return out if z is None else out + sigma * z


def dpmpp_from_x0(x0, x, hist, cx, c0, c1):
    m = cx * x + c0 * x0
    return m + c1 * hist if c1 != 0 else m


def sample(eps, T, xT, noise, *, kind, shaping, cond=None, none_value=-2.0, w=None, ddim_sigma=None, coefs=None, log=None):
    """The DDPM loop Ns-1..0 in fp64 with shaped predictor steps.  eps(net_in, k): the net's output at sampling step k for the input net_in
    (the state, or state | condition when cond is given), any dtype in, any out.  T: the tables (name -> array).  kind: "ancestral", "ddim"
    (ddim_sigma: DDIM(eta)) or "dpmpp" (coefs = (cx, c0, c1)).  w (a float or a [B] tensor; needs cond): classifier-free guidance against the
    none_value-filled condition.  noise: the injected draws, used in order.  log (a list): receives (step, f, s) per step.
    -> (x0 clipped to [-1, 1], draws used, evaluations)"""
    T = {k: np.asarray(v, np.float64) for k, v in T.items()}
    K = len(T["alphas_cumprod_prev"])
    x = xT.double().clone()
    cond64 = None if cond is None else cond.double()
    none = None if cond is None else torch.full_like(x, none_value)
    used = n_eval = 0
    hist = None

    def net(c, k):
        nonlocal n_eval
        n_eval += 1
        return eps(x if c is None else torch.cat((x, c), dim=-3), k).double()

    def draw():
        nonlocal used
        used += 1
        return noise[used - 1].double()

    for i in reversed(range(K)):
        ec = net(cond64, i)
        eg = ec if w is None else (lambda eu: eu + _per_image(w, x) * (ec - eu))(net(none, i))
        cr, crm1 = float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i])
        x0, f, s = shaped_x0(x, ec, eg, cr, crm1, shaping)
        if log is not None:
            log.append((i, f.clone(), s.clone()))
        if kind == "dpmpp":
            cx, c0, c1 = (float(c[i]) for c in coefs)
            x, hist = dpmpp_from_x0(x0, x, hist, cx, c0, c1), x0
        elif kind == "ddim":
            sg = 0.0 if ddim_sigma is None else float(ddim_sigma[i])
            z = draw() if ddim_sigma is not None and i > 0 else None
            x = ddim_from_x0(x0, x, z, cr, crm1, float(T["alphas_cumprod_prev"][i]), sg)
        else:
            z = draw() if i > 0 else None
            x = ancestral_from_x0(x0, x, z, float(T["posterior_mean_coef1"][i]), float(T["posterior_mean_coef2"][i]),
                                  float(np.exp(0.5 * T["posterior_log_variance_clipped"][i])))
    return x.clamp(-1.0, 1.0), used, n_eval
