"""The null-space (DDNM) samplers restated in numpy, written from the formulas of the issue and the header block of mi355_ddpm_nullspace_sample, not
from the HIP code: the three row operators A with their pseudo-inverses, the rectified predictor step in both forms, the DDNM+ coefficient tables, the
loop, and an fp32 model of the step in the kernel's documented operation order (for the error budget).

An operator is a dict: {"kind": 0, "known": bool [B, C, H, W]} (mask), {"kind": 1, "hl": .., "wl": ..} (block mean), {"kind": 2, "hl": .., "wl": ..}
(bilinear taps of an integer factor).  All three have disjoint rows with equal weights inside a row, so A A^T is diagonal and A^+ r is r_q on every
tap of row q: `spread`.
"""
import numpy as np


def axis_taps(s):
    """Offsets inside a block of s pixels and their weights for the bilinear reduction by the integer factor s (align_corners = False): the source
    position of output o is s (o + 1/2) - 1/2 = s o + (s - 1) / 2 - an integer for odd s (one tap, weight 1), half-way between s o + s/2 - 1 and
    s o + s/2 for even s (two taps, weight 1/2 each)."""
    s = int(s)
    return [((s - 1) // 2, 1.0)] if s % 2 else [(s // 2 - 1, 0.5), (s // 2, 0.5)]


def _taps(op, H, W):
    sy, sx = H // op["hl"], W // op["wl"]
    if op["kind"] == 1:
        return sy, sx, [(j, 1.0 / sy) for j in range(sy)], [(j, 1.0 / sx) for j in range(sx)]
    return sy, sx, axis_taps(sy), axis_taps(sx)


def n_taps(op, H, W):
    if op["kind"] == 0:
        return 1
    _, _, ty, tx = _taps(op, H, W)
    return len(ty) * len(tx)


def apply_A(op, v):
    """A v.  Kind 0: v itself (a row per known pixel; the unknown entries are not rows and are never read by a caller).  Kind 1: the block means.
    Kind 2: the weighted tap sums."""
    if op["kind"] == 0:
        return v
    B, C, H, W = v.shape
    sy, sx, ty, tx = _taps(op, H, W)
    blocks = v.reshape(B, C, op["hl"], sy, op["wl"], sx)
    if op["kind"] == 1:
        return blocks.mean(axis=(3, 5))
    out = np.zeros((B, C, op["hl"], op["wl"]), dtype=v.dtype)
    for oy, wy in ty:
        for ox, wx in tx:
            out = out + (wy * wx) * blocks[:, :, :, oy, :, ox]
    return out


def tap_mask(op, shape):
    """True where a pixel is a tap of some row."""
    if op["kind"] == 0:
        return op["known"]
    B, C, H, W = shape
    sy, sx, ty, tx = _taps(op, H, W)
    m = np.zeros((B, C, op["hl"], sy, op["wl"], sx), dtype=bool)
    for oy, _ in ty:
        for ox, _ in tx:
            m[:, :, :, oy, :, ox] = True
    return m.reshape(shape)


def spread(op, q, shape):
    """q_row on every tap of the row, 0 elsewhere: A^+ q for these operators (A^T (A A^T)^-1 with A A^T = diag(sum of squared weights))."""
    if op["kind"] == 0:
        return np.where(op["known"], q, 0.0)
    B, C, H, W = shape
    sy, sx = H // op["hl"], W // op["wl"]
    full = np.broadcast_to(q[:, :, :, None, :, None], (B, C, op["hl"], sy, op["wl"], sx)).reshape(shape)
    return np.where(tap_mask(op, shape), full, 0.0)


def pinv(op, q, shape):
    return spread(op, q, shape)


def x0_pre(pred, x, out, cr, crm1, sa, sb):
    if pred == "x0":
        return out
    if pred == "v":
        return sa * x - sb * out
    return cr * x - crm1 * out


def clip(a):
    return np.where(np.isnan(a), a, np.clip(a, -1.0, 1.0))


def ddim_coefs(acp_prev, sigma):
    return np.sqrt(acp_prev), np.sqrt(max(1.0 - acp_prev - sigma * sigma, 0.0))


def step(op, pred, form, x, out, y, z, c, detail=False):
    """One rectified predictor step in fp64.  c: dict(cr, crm1, sa, sb, a, b, lam, sigma); form 0: a, b = coef1, coef2; form 1: a = acp_prev.
    z None: no noise (form 0 adds sigma * 0; form 1 adds nothing).  y: the measurement (kind 0: [B, C, H, W], read where known)."""
    x0 = clip(x0_pre(pred, x, out, c["cr"], c["crm1"], c["sa"], c["sb"]))
    Ax = apply_A(op, x0)
    r = Ax - y
    if op["kind"] == 0:
        r = np.where(op["known"], r, 0.0)
    t = c["lam"] * r
    x0h = np.where(tap_mask(op, x.shape), x0 - spread(op, t, x.shape), x0)
    if form == 0:
        new = (c["a"] * x0h + c["b"] * x) + c["sigma"] * (0.0 if z is None else z)
    else:
        sa, sb = ddim_coefs(c["a"], c["sigma"])
        e2 = (c["cr"] * x - x0h) / c["crm1"]
        new = sa * x0h + sb * e2
        if z is not None:
            new = new + c["sigma"] * z
    if detail:
        return new, dict(x0=x0, Ax=Ax, r=r, t=t, x0h=x0h)
    return new


def coefs64(T, sigma_y):
    """(lam, sigma) of DDNM+ in fp64 from the chain's tables (paper eq. 17-19, simplified form)."""
    a = np.asarray(T["posterior_mean_coef1"], dtype=np.float64)
    s = np.exp(0.5 * np.asarray(T["posterior_log_variance_clipped"], dtype=np.float64))
    s[0] = 0.0
    K = len(a)
    lam, sig = np.ones(K), np.zeros(K)
    for i in range(K):
        if sigma_y > 0.0 and s[i] < a[i] * sigma_y:
            lam[i] = s[i] / (a[i] * sigma_y)      # then a lam sigma_y = s: the measurement's noise is the whole posterior variance, nothing is drawn
            continue
        sig[i] = np.sqrt(max(s[i] ** 2 - (a[i] * lam[i] * sigma_y) ** 2, 0.0))
    return lam, sig


def moves(K, walk=None):
    if walk is None:
        return [(L, True) for L in range(K, 0, -1)]
    return [(a, b < a) for a, b in zip(walk, walk[1:])]


def sample(out_fn, T, op, pred, form, xT, y, noise, lam, sigma=None, ddim_sigma=None, walk=None, channels=None):
    """The loop in fp64: out_fn(x float32 tensor-like [B, C, H, W] as numpy, k) -> the network output as numpy (its first `channels` channels are read).
    T: name -> array [K].  noise: a list of draws, consumed in order.  -> (result fp64, draws used, evaluations)."""
    T = {k: np.asarray(v, dtype=np.float64) for k, v in T.items()}
    x = np.asarray(xT, dtype=np.float64).copy()
    K = len(T["alphas_cumprod_prev"])
    C = x.shape[1] if channels is None else channels
    used = n_eval = 0

    def draw():
        nonlocal used
        z = np.asarray(noise[used], dtype=np.float64)
        used += 1
        return z

    for level, down in moves(K, walk):
        if not down:
            x = np.sqrt(T["alphas"][level]) * x + np.sqrt(T["betas"][level]) * draw()
            continue
        i = level - 1
        out = np.asarray(out_fn(x.astype(np.float32), i), dtype=np.float64)[:, :C]
        n_eval += 1
        c = dict(cr=T["sqrt_recip_alphas_cumprod"][i], crm1=T["sqrt_recipm1_alphas_cumprod"][i], sa=T["sqrt_alphas_cumprod"][i],
                 sb=T["sqrt_one_minus_alphas_cumprod"][i], lam=float(lam[i]))
        if form == 0:
            c.update(a=T["posterior_mean_coef1"][i], b=T["posterior_mean_coef2"][i], sigma=float(sigma[i]))
            z = draw() if i > 0 else None
        else:
            c.update(a=T["alphas_cumprod_prev"][i], b=0.0, sigma=float(ddim_sigma[i]) if ddim_sigma is not None else 0.0)
            z = draw() if (ddim_sigma is not None and i > 0) else None
        x = step(op, pred, form, x, out, y, z, c)
    return clip(x), used, n_eval


# ---- the step in fp32 numpy, in the kernel's documented operation order -----------------------------------------------------------------------------

def step32(op, pred, form, x, out, y, z, c):
    """Every operation rounded to fp32, none contracted; the block sum of kind 1 each row left to right, then the row sums top to bottom, one division
    by (float)(sy sx); kind 2 as l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11) with absent taps entering as 0."""
    f = np.float32
    x, out = x.astype(f), out.astype(f)
    cr, crm1, sa_p, sb_p, a, b, lam, sigma = (f(c[k]) for k in ("cr", "crm1", "sa", "sb", "a", "b", "lam", "sigma"))
    with np.errstate(invalid="ignore"):
        if pred == "x0":
            pre = out
        elif pred == "v":
            pre = sa_p * x - sb_p * out
        else:
            pre = cr * x - crm1 * out
        x0 = np.where(pre < -1, f(-1), np.where(pre > 1, f(1), pre)).astype(f)
        shape = x.shape
        if op["kind"] == 0:
            r = (x0 - y.astype(f)).astype(f)
            x0h = np.where(op["known"], x0 - lam * r, x0).astype(f)
        else:
            B, C, H, W = shape
            sy, sx = H // op["hl"], W // op["wl"]
            blocks = x0.reshape(B, C, op["hl"], sy, op["wl"], sx)
            if op["kind"] == 1:
                rows = blocks[..., 0]
                for j in range(1, sx):
                    rows = (rows + blocks[..., j]).astype(f)            # [B, C, hl, sy, wl]
                s = rows[:, :, :, 0, :]
                for j in range(1, sy):
                    s = (s + rows[:, :, :, j, :]).astype(f)
                Ax = (s / f(sy * sx)).astype(f)
            else:
                ty, tx = axis_taps(sy), axis_taps(sx)
                zero = np.zeros((B, C, op["hl"], op["wl"]), dtype=f)
                v = [[blocks[:, :, :, ty[i][0], :, tx[j][0]] if (i < len(ty) and j < len(tx)) else zero for j in range(2)] for i in range(2)]
                l1y, l1x = f(0.5 if len(ty) == 2 else 0.0), f(0.5 if len(tx) == 2 else 0.0)
                l0y, l0x = f(1) - l1y, f(1) - l1x
                top = (l0x * v[0][0] + l1x * v[0][1]).astype(f)
                bot = (l0x * v[1][0] + l1x * v[1][1]).astype(f)
                Ax = (l0y * top + l1y * bot).astype(f)
            r = (Ax - y.astype(f)).astype(f)
            t = (lam * r).astype(f)
            full = np.broadcast_to(t[:, :, :, None, :, None], (B, C, op["hl"], sy, op["wl"], sx)).reshape(shape)
            x0h = np.where(tap_mask(op, shape), x0 - full, x0).astype(f)
        if form == 0:
            new = ((a * x0h + b * x) + sigma * (f(0) if z is None else z.astype(f))).astype(f)
        else:
            sa, sb = np.sqrt(a), np.sqrt(np.maximum((f(1.0) - a) - sigma * sigma, f(0.0)))
            e2 = ((cr * x - x0h) / crm1).astype(f)
            new = (sa * x0h + sb * e2).astype(f)
            if z is not None:
                new = (new + sigma * z.astype(f)).astype(f)
    return new
