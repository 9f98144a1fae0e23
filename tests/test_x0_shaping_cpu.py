"""CPU: per-image x0 shaping (DDPM.with_x0_shaping; mi355_ddpm_shaped_sample) - the fp64 restatement (tests/x0_shaping_ref.py) against
torch.quantile / clamp / std, the host validation and the views, the library's refusals through the ABI (no GPU: they come before any launch and
before the handle is looked at), the new symbols, and the rounding budgets the GPU tests hold the kernels to, each proven here on an fp32 numpy
restatement in the kernels' operation order.

Budgets (fp64 from the fp32 inputs, EPS32 = 2^-24, first-order count r, bound (r + 1) EPS32 M as tests/test_multistep_cpu.py does):
  x0_hat  : f e, c_recipm1 (f e), c_recip x, the difference, the division by s >= 1 - five roundings of values bounded by
            P = |c_recip x| + |c_recipm1 f e| (the clamp is exact and 1-Lipschitz): two more than the static clip's three.
  ancestral step  r = 8:  coef1 x0 carries x0's 5 and its own product, then two sums; coef2 x: a product and two sums; sigma z: a product and a sum.
            M = |coef1| P + |coef2 x| + |sigma z|.
  DDIM(eta) step  r = 12: tests/test_ddpm_respace_cpu.py's r = 10 on M = (sa + sb / b) P + sb |a x| / b + |sigma z| plus the two new roundings of x0.
  DPM-Solver++    r = 10: tests/test_multistep_cpu.py's R_DPMPP = 8 on M = |cx x| + |c0| P + |c1 hist| plus the same two.
  sigma   : a sum of `per` fp32 terms in the kernel's order has depth L = ceil(per / 1024) + 6 + 16 (a thread's strided serial sum, six butterfly
            levels, the sixteen waves in order): |sum error| <= L EPS32 sum|v|.  The mean adds its division; each centred term two roundings, its
            square one; the variance its division, the root its own.  |sigma error| <= (L + 1) EPS32 mean|v| + ((L + 3) / 2 + 2) EPS32 sigma, the
            first term being the mean's error passed through d -> sqrt(mean d^2) (1-Lipschitz in a constant shift of the centre).
  f       : phi (sigma_c / sigma_g) + (1 - phi): the two sigmas' relative errors, the division, the product, the fp32 (1 - phi), the sum.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import x0_shaping_ref as XR
from tests.test_ddpm_respace_cpu import EPS32, STEPS7, step_inputs
from tests.test_multistep_cpu import R_DPMPP

R_X0, R_ANCESTRAL, R_DDIM, R_DPMPP_SHAPED = 5, 8, 12, R_DPMPP + 2
XS_THREADS = 1024


def _ddpm(Ns):
    from image_diffusion.sde_diffusion import DDPM

    return DDPM(Ns)


# ---- the restatement against torch.quantile, clamp and std ---------------------------------------------------------------------------------

@pytest.mark.parametrize("per", [1, 2, 5, 64, 257, 3 * 8 * 8])
@pytest.mark.parametrize("p", [0.5, 0.9, 0.995, 1.0])
def test_restatement_is_torch_quantile(per, p):
    g = torch.Generator().manual_seed(7000 + per)
    x0 = torch.randn(3, per, generator=g, dtype=torch.float64) * 1.7
    s, s_raw = XR.threshold(x0, p)
    p32 = float(np.float32(p))
    want = torch.quantile(x0.abs(), p32, dim=1)            # interpolation="linear": lo + frac (hi - lo)
    torch.testing.assert_close(s_raw, want, rtol=1e-6, atol=0)   # frac is rounded to fp32 in the restatement (the kernel's argument): 2^-24 relative
    assert torch.equal(s, s_raw.clamp(min=1.0))
    s2, _ = XR.threshold(x0, p, s_max=1.25)
    assert torch.equal(s2, s_raw.clamp(1.0, 1.25))
    # shaped_x0 is clamp / s with that s, and std is torch.std without Bessel's correction (the ratio of two is that of any normalisation)
    x = torch.randn(3, per, generator=g, dtype=torch.float64)
    ec, eu = torch.randn(3, per, generator=g, dtype=torch.float64), torch.randn(3, per, generator=g, dtype=torch.float64)
    eg = eu + 3.0 * (ec - eu)
    got, f, s3 = XR.shaped_x0(x, ec, eg, 1.5, 1.1, (p, None, 0.7))
    sc, sg = XR.sigmas(ec, eg)
    torch.testing.assert_close(sc, ec.std(dim=1, correction=0), rtol=1e-12, atol=1e-300)
    phi32, om = float(np.float32(0.7)), float(np.float32(1.0) - np.float32(0.7))
    torch.testing.assert_close(f, torch.where(sg == 0, torch.ones_like(sg), phi32 * sc / sg + om), rtol=1e-14, atol=0)
    pre = 1.5 * x - 1.1 * (f[:, None] * eg)
    q = torch.quantile(pre.abs(), p32, dim=1).clamp(min=1.0)
    torch.testing.assert_close(got, torch.maximum(torch.minimum(pre, q[:, None]), -q[:, None]) / q[:, None], rtol=1e-6, atol=1e-9)
    if per == 1:
        assert torch.equal(f, torch.ones(3, dtype=torch.float64))     # one element: sigma_g == 0
    # s == 1 is the static clip, and shaping None is it too
    small = XR.shaped_x0(0.1 * x, ec * 0.1, ec * 0.1, 1.5, 1.1, (p, None, 0.0))
    assert torch.equal(small[0], (1.5 * (0.1 * x) - 1.1 * (ec * 0.1)).clamp(-1, 1)) and torch.equal(small[2], torch.ones(3, dtype=torch.float64))
    assert torch.equal(XR.shaped_x0(x, ec, eg, 1.5, 1.1, None)[0], (1.5 * x - 1.1 * eg).clamp(-1, 1))


def test_restatement_nan_and_position():
    x0 = torch.tensor([[0.5, float("nan"), 2.0, 3.0], [0.5, -0.0, 2.0, -3.0]], dtype=torch.float64)
    s, s_raw = XR.threshold(x0, 0.5)
    assert math.isnan(float(s[0])) and math.isnan(float(s_raw[0])) and float(s_raw[1]) == 1.25 and float(s[1]) == 1.25
    assert XR.position(1.0, 7) == (6, 0.0) and XR.position(0.5, 4) == (1, 0.5) and XR.position(0.3, 1) == (0, 0.0)
    k, frac = XR.position(0.995, 3 * 32 * 32)
    assert k == int(math.floor(float(np.float32(0.995)) * 3071)) and 0.0 <= frac < 1.0
    x = torch.tensor([[[0.5, float("nan")]], [[0.25, 4.0]]], dtype=torch.float64)
    got, _, s = XR.shaped_x0(x, torch.zeros_like(x), torch.zeros_like(x), 1.0, 0.0, (1.0, None, 0.0))
    assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1], torch.tensor([[0.0625, 1.0]], dtype=torch.float64)) and float(s[1]) == 4.0


# ---- host validation and the views ---------------------------------------------------------------------------------------------------------

def test_with_x0_shaping_validates_as_the_library_does():
    from image_diffusion.sde_diffusion import X0Shaping

    d = _ddpm(100)
    assert d.x0_shaping is None and d.respace(10).x0_shaping is None
    v = d.with_x0_shaping(dynamic_threshold=0.995, max_threshold=1.5, guidance_rescale=0.7)
    assert v.x0_shaping == X0Shaping(0.995, 1.5, 0.7) and d.x0_shaping is None
    assert d.with_x0_shaping(1, None, 0).x0_shaping == X0Shaping(1.0, None, 0.0)
    assert d.with_x0_shaping(guidance_rescale=1.0).x0_shaping == X0Shaping(None, None, 1.0)
    assert d.with_x0_shaping().x0_shaping is None and v.with_x0_shaping().x0_shaping is None       # all off: no shaping
    for kw in (dict(dynamic_threshold=0.0), dict(dynamic_threshold=-0.1), dict(dynamic_threshold=1.0001), dict(dynamic_threshold=float("nan")),
               dict(dynamic_threshold=True), dict(dynamic_threshold="0.9"), dict(dynamic_threshold=0.9, max_threshold=0.99),
               dict(dynamic_threshold=0.9, max_threshold=float("nan")), dict(max_threshold=0.0), dict(guidance_rescale=-0.01),
               dict(guidance_rescale=1.01), dict(guidance_rescale=float("nan")), dict(guidance_rescale=None)):
        with pytest.raises(ValueError):
            d.with_x0_shaping(**kw)
        with pytest.raises(ValueError):
            d.respace(5).with_x0_shaping(**kw)
    assert d.with_x0_shaping(0.9, max_threshold=float("inf")).x0_shaping.max_threshold == float("inf")


def test_views_share_tables_and_commute_with_respace():
    from image_diffusion.sampling import _sched_key
    from image_diffusion.sde_diffusion import TABLE_NAMES, RespacedDDPM

    d = _ddpm(100)
    for base in (d, d.respace(STEPS7)):
        v = base.with_x0_shaping(0.9, guidance_rescale=0.5)
        assert type(v) is type(base) and v is not base
        assert [n for n, _ in v.named_buffers()] == list(TABLE_NAMES) == [n for n, _ in base.named_buffers()]
        assert all(a is b for (_, a), (_, b) in zip(v.named_buffers(), base.named_buffers()))     # the same tensors
        assert _sched_key(v) == _sched_key(base) and v.Ns == base.Ns
        hv, hb = v.host_tables(), base.host_tables()
        assert list(hv) == list(hb) and all(torch.equal(hv[k], hb[k]) for k in hb)
        assert v.time(3) == base.time(3) and list(v.state_dict()) == list(base.state_dict())
    a, b = d.respace(STEPS7).with_x0_shaping(0.9, 2.0, 0.5), d.with_x0_shaping(0.9, 2.0, 0.5).respace(STEPS7)
    assert isinstance(a, RespacedDDPM) and isinstance(b, RespacedDDPM)
    assert a.x0_shaping == b.x0_shaping is not None and a.timesteps == b.timesteps and a.base_Ns == b.base_Ns
    assert all(torch.equal(x, y) for (_, x), (_, y) in zip(a.named_buffers(), b.named_buffers()))
    assert all(torch.equal(x, y) for x, y in zip(a.dpm_solver_coefs(2), b.dpm_solver_coefs(2)))


def test_samplers_refuse_what_shaping_cannot_do():
    """guidance_rescale on an unguided sampler: ValueError when the sampler is made (generic path) or called; ReconstructionGuidance: refused."""
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, ReconstructionGuidance, Replacement
    from image_diffusion.likelihoods import InPainting

    d = _ddpm(100).respace(5)
    lik = InPainting(patch_size=4, pad_value=-2)
    eps = lambda xi, i: torch.zeros_like(xi[:, :1])   # noqa: E731
    phi = d.with_x0_shaping(0.9, guidance_rescale=0.5)
    xT = torch.zeros(2, 1, 8, 8)
    with pytest.raises(ValueError, match="guided"):
        sampling.get_ddim_sample_fn(eps, phi)
    with pytest.raises(ValueError, match="guided"):
        sampling.get_dpm_solver_sample_fn(eps, phi)
    for fn in (sampling.get_prior_sample_fn(eps, phi, Amortized(1.0, 0, 0.1), lik),):
        with pytest.raises(ValueError, match="guided"):
            fn(xT)
    for cond in (Amortized(1.0, 0, 0.1), Replacement(0.1, 1.0, True, 0)):
        with pytest.raises(ValueError, match="guided"):
            sampling.get_conditional_sample_fn(eps, phi, cond, lik)(xT, xT)
    sampling.get_ddim_sample_fn(eps, phi, lik, guidance_scale=2.0)      # a guided sampler takes it

    class Net:
        engine = None

    tagged = sampling.make_eps_model(Net(), d)
    sampling.get_conditional_sample_fn(tagged, d, ReconstructionGuidance(1.0, 1.0, "before", 0, 0.1), lik)      # the unshaped chain is taken
    with pytest.raises(NotImplementedError, match="with_x0_shaping"):
        sampling.get_conditional_sample_fn(tagged, d.with_x0_shaping(0.9), ReconstructionGuidance(1.0, 1.0, "before", 0, 0.1), lik)


# ---- the library's refusals, through the ABI --------------------------------------------------------------------------------------------------

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
    for name in ("mi355_ddpm_shaped_workspace_bytes", "mi355_ddpm_shaped_sample", "mi355_x0_shape_stats", "mi355_x0_shaped_step"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.mi355_version() == 108
    d = _ddpm(100).respace(STEPS7)
    tb, keep = _tables_c(d)
    opt = _lib.DDPMOptionsC(_lib.DDIM, 0, 0.1, 1e-5, 1.0, 1.0, 1, -2.0, -2.0, 1, 0)
    steps = (C.c_int32 * d.Ns)(*d.timesteps)
    sd = _lib.DDPMScheduleC()
    sd.steps, sd.train_steps = C.cast(steps, C.POINTER(C.c_int32)), d.base_Ns
    cs = [c.contiguous() for c in d.dpm_solver_coefs(2)]
    ms = _lib.MultistepScheduleC()
    ms.steps, ms.train_steps = sd.steps, d.base_Ns
    ms.cx, ms.c0, ms.c1 = (C.cast(c.data_ptr(), C.POINTER(C.c_float)) for c in cs)

    def call(sh, guided=0, sched=None, msched=None):
        return L.mi355_ddpm_shaped_sample(None, None, 1, None, None, 0, guided, 2.0, None, C.byref(tb), C.byref(opt),
                                          C.byref(sched) if sched is not None else None, C.byref(msched) if msched is not None else None,
                                          C.byref(sh) if sh is not None else None, None, 0, 3, None, 0, None)

    S = _lib.X0ShapingC
    inf, nan = float("inf"), float("nan")
    cases = [(S(1.5, 0, 0), 0, b"shaping->quantile"), (S(-0.1, 0, 0), 0, b"shaping->quantile"), (S(nan, 0, 0), 0, b"shaping->quantile"),
             (S(inf, 0, 0), 0, b"shaping->quantile"), (S(0.9, 0.5, 0), 0, b"shaping->max_threshold"), (S(0.9, -2.0, 0), 0, b"shaping->max_threshold"),
             (S(0.9, nan, 0), 0, b"shaping->max_threshold"), (S(0.9, 0, 1.5), 1, b"shaping->rescale_phi"), (S(0.9, 0, -0.5), 1, b"shaping->rescale_phi"),
             (S(0.9, 0, nan), 1, b"shaping->rescale_phi"), (S(0.9, 0, 0.5), 0, b"guided != 0")]
    for sh, guided, msg in cases:
        for kw in ({}, dict(sched=sd), dict(msched=ms)):
            assert call(sh, guided, **kw) == -1 and msg in L.mi355_last_error() and b"ddpm_shaped_sample" in L.mi355_last_error(), (msg, kw)
    assert call(S(0.9, 0, 0), 0, sched=sd, msched=ms) == -1 and b"both sched and msched" in L.mi355_last_error()
    assert call(None, 0, sched=sd, msched=ms) == -1 and b"both sched and msched" in L.mi355_last_error()
    # the loops' own refusals, under this entry point's name; then, everything in order, the missing handle
    bad = _lib.DDPMScheduleC()
    bad.steps, bad.train_steps = sd.steps, 0
    assert call(S(0.9, 0, 0), 0, sched=bad) == -1 and b"ddpm_shaped_sample: train_steps" in L.mi355_last_error()
    opt.mode = _lib.DDPM_PRIOR
    assert call(S(0.9, 0, 0), 0, msched=ms) == -1 and b"ddpm_shaped_sample: opt->mode must be MI355_DDIM" in L.mi355_last_error()
    opt.mode = _lib.DDIM
    for sh in (None, S(0, 0, 0), S(0.9, 2.0, 0), S(1.0, inf, 0)):
        assert call(sh) == -1 and b"bad argument (net, x, workspace, batch)" in L.mi355_last_error()
    assert call(S(0.9, 0, 1.0), 1) == -1 and b"bad argument (net, x, workspace, batch)" in L.mi355_last_error()
    assert L.mi355_ddpm_shaped_workspace_bytes(None, 3, 0, 0) == -1
    # the statistics op refuses the same struct before it looks at a pointer
    for sh, guided, msg in cases:
        assert L.mi355_x0_shape_stats(None, None, 1.0, None, guided, 1.0, 1.0, C.byref(sh), None, None, 3, 16, None) == -1
        assert msg in L.mi355_last_error() and b"x0_shape_stats" in L.mi355_last_error()
    for args, msg in (((None, None), b"x is null"),):
        assert L.mi355_x0_shape_stats(*args, 1.0, None, 0, 1.0, 1.0, None, None, None, 3, 16, None) == -1 and msg in L.mi355_last_error()
    assert L.mi355_x0_shaped_step(7, None, None, None, None, 0, 0.0, None, 4, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, None, 8, None) == -1
    assert b"kind" in L.mi355_last_error()
    del keep


# ---- the budgets ------------------------------------------------------------------------------------------------------------------------------

def rows_for(n, per, seed):
    """fp32 rows (f, s) for n = B * per elements: f in [0.6, 1.2], s in [1, 2.5], one image with (1, 1)."""
    B = n // per
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.6, 1.2, B).astype(np.float32)
    s = rng.uniform(1.0, 2.5, B).astype(np.float32)
    f[0], s[0] = 1.0, 1.0
    return f, s


def _pre(x, eps, f, s, a, b, per):
    """fp64 x0_hat and P from the fp32 inputs."""
    a, b = float(np.float32(a)), float(np.float32(b))
    fe = np.repeat(f.astype(np.float64), per) * eps.astype(np.float64)
    sv = np.repeat(s.astype(np.float64), per)
    x64 = x.astype(np.float64)
    pre = a * x64 - b * fe
    x0 = np.where(np.isnan(pre), pre, np.clip(pre, -sv, sv)) / sv
    return x0, np.abs(a * x64) + np.abs(b * fe), x64


def shaped_budget(kind, x, eps, f, s, per, a, b, c=None, z=None, hist=None):
    """-> (fp64 step result from the fp32 inputs and rows, fp64 x0_hat, the step's bound, x0_hat's bound).  c: ancestral (coef1, coef2, sigma);
    ddim / ddim_eta (acp_prev, sigma); dpmpp (cx, c0, c1)."""
    x0, P, x64 = _pre(x, eps, f, s, a, b, per)
    a64, b64 = float(np.float32(a)), float(np.float32(b))
    c = tuple(float(np.float32(v)) for v in c)
    z64 = None if z is None else z.astype(np.float64)
    if kind == "ddpm":
        c1, c2, sg = c
        want = XR.ancestral_from_x0(x0, x64, z64, c1, c2, sg)
        M = abs(c1) * P + np.abs(c2 * x64) + (0.0 if z64 is None else np.abs(sg * z64))
        r = R_ANCESTRAL
    elif kind in ("ddim", "ddim_eta"):
        prev, sg = c
        want = XR.ddim_from_x0(x0, x64, z64, a64, b64, prev, sg)
        sa, sb = math.sqrt(prev), math.sqrt(max(1.0 - prev - sg * sg, 0.0))
        M = (sa + sb / b64) * P + sb * np.abs(a64 * x64) / b64 + (0.0 if z64 is None else np.abs(sg * z64))
        r = R_DDIM
    else:
        cx, c0, c1 = c
        h64 = hist.astype(np.float64)
        want = XR.dpmpp_from_x0(x0, x64, h64, cx, c0, c1)
        M = np.abs(cx * x64) + abs(c0) * P + np.abs(c1 * h64)
        r = R_DPMPP_SHAPED
    return want, x0, (r + 1) * EPS32 * M, (R_X0 + 1) * EPS32 * P


def shaped_fp32(kind, x, eps, f, s, per, a, b, c, z=None, hist=None, mutant=None):
    """The kernels' arithmetic in fp32 numpy, in their operation order."""
    t = np.float32
    a, b = t(a), t(b)
    c = tuple(t(v) for v in c)
    fv, sv = np.repeat(f, per), np.repeat(s, per)
    ax = a * x
    pre = ax - b * (eps if mutant == "no_f" else fv * eps)
    lo = -sv if mutant != "static" else t(-1) + 0 * sv
    hi = -lo
    x0 = np.where(pre < lo, lo, np.where(pre > hi, hi, pre))
    if mutant not in ("static", "no_div"):
        x0 = x0 / sv
    if kind == "ddpm":
        m = c[0] * x0 + c[1] * x
        out = m if z is None else m + c[2] * z
    elif kind in ("ddim", "ddim_eta"):
        prev, sg = c
        sa, sb = np.sqrt(prev), np.sqrt(np.maximum((t(1.0) - prev) - sg * sg, t(0.0)))
        m = sa * x0 + sb * ((ax - x0) / b)
        out = m if z is None else m + sg * z
    else:
        m = c[0] * x + c[1] * x0
        out = m + c[2] * hist if c[2] != 0 else m
    return out.astype(np.float32), x0.astype(np.float32)


def step_cases():
    """(kind, c_recip, c_recipm1, coefficients) on DDPM(100).respace(STEPS7) at three steps: the four kinds, eta = 0.5 for DDIM(eta)."""
    r = _ddpm(100).respace(STEPS7)
    T = r.host_tables()
    sg = r.ddim_sigma(0.5)
    cx, c0, c1 = r.dpm_solver_coefs(2)
    out = []
    for k in (1, 3, r.Ns - 2):
        a, b = float(T["sqrt_recip_alphas_cumprod"][k]), float(T["sqrt_recipm1_alphas_cumprod"][k])
        out.append(("ddpm", a, b, (float(T["posterior_mean_coef1"][k]), float(T["posterior_mean_coef2"][k]),
                                   float((0.5 * T["posterior_log_variance_clipped"][k]).exp()))))
        out.append(("ddim", a, b, (float(T["alphas_cumprod_prev"][k]), 0.0)))
        out.append(("ddim_eta", a, b, (float(T["alphas_cumprod_prev"][k]), float(sg[k]))))
        out.append(("dpmpp", a, b, (float(cx[k]), float(c0[k]), float(c1[k]))))
    return out


def step_operands(kind, n, a, b, seed):
    x, eps, z = step_inputs(n, a, b, seed)
    x, eps = (1.6 * x).astype(np.float32), (1.6 * eps).astype(np.float32)     # pre reaches +-2.4: beyond thresholds up to 2.5 only rarely, beyond 1 often
    hist = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, n).astype(np.float32)
    return x, eps, (z if kind in ("ddpm", "ddim_eta") else None), (hist if kind == "dpmpp" else None)


def test_fp32_restatement_of_the_shaped_steps_stays_inside_the_budgets():
    worst = {}
    broke = dict(no_f=0, static=0, no_div=0)
    cases = step_cases()
    for j, (kind, a, b, c) in enumerate(cases):
        for n, per in ((105, 35), (768, 256)):
            x, eps, z, hist = step_operands(kind, n, a, b, 100 * j + n)
            f, s = rows_for(n, per, 9 * j + n)
            with np.errstate(invalid="ignore"):
                want, x0, bound, bound0 = shaped_budget(kind, x, eps, f, s, per, a, b, c, z, hist)
                got, g0 = shaped_fp32(kind, x, eps, f, s, per, a, b, c, z, hist)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and nan.sum() == 1
            ratio = float((np.abs(got.astype(np.float64) - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max())
            worst[kind] = max(worst.get(kind, 0.0), ratio)
            assert ratio <= 1.0, (kind, n, ratio)
            assert (np.abs(g0.astype(np.float64) - x0)[~nan] <= bound0[~nan]).all(), (kind, n)
            # rows (1, 1) are the static clip, bit for bit
            one = np.ones_like(f)
            with np.errstate(invalid="ignore"):
                u = shaped_fp32(kind, x, eps, one, one, per, a, b, c, z, hist)[0]
                v = shaped_fp32(kind, x, eps, one, one, per, a, b, c, z, hist, mutant="static")[0]
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
            for mut in broke:
                with np.errstate(invalid="ignore"):
                    bad = shaped_fp32(kind, x, eps, f, s, per, a, b, c, z, hist, mutant=mut)[0].astype(np.float64)
                broke[mut] += bool((np.abs(bad - want)[~nan] > bound[~nan]).any())
    print(f"shaped steps, fp32 restatement: max err / budget {worst}; cases broken by each mutant: {broke} of {2 * len(cases)}")
    assert all(v == 2 * len(cases) for v in broke.values())


def sigma_budget(v):
    """v [B, per] fp32 -> (fp64 population sigma per image, its bound)."""
    v64 = v.astype(np.float64)
    per = v.shape[1]
    L = -(-per // XS_THREADS) + 6 + XS_THREADS // 64
    sig = np.sqrt(((v64 - v64.mean(axis=1, keepdims=True)) ** 2).mean(axis=1))
    return sig, (L + 1) * EPS32 * np.abs(v64).mean(axis=1) + ((L + 3) / 2 + 2) * EPS32 * sig


def factor_budget(sc, bc, sg, bg, phi):
    """-> (fp64 f, its bound) from the fp64 sigmas and their bounds."""
    phi32, om = float(np.float32(phi)), float(np.float32(1.0) - np.float32(phi))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(sg == 0, 0.0, sc / np.where(sg == 0, 1.0, sg))
        rel = np.where(sg == 0, 0.0, bc / np.maximum(sc, 1e-300) + bg / np.where(sg == 0, 1.0, sg)) + 2 * EPS32
    f = np.where(sg == 0, 1.0, phi32 * ratio + om)
    return f, 1.25 * (phi32 * ratio * rel + EPS32 * np.abs(f)) + 1e-300      # 1.25: the second-order terms of a first-order count


def sigma_fp32(v):
    """The kernel's order in fp32 numpy: thread t sums elements t, t + 1024, ...; six butterfly levels inside each wave of 64; the waves in order."""
    t = np.float32
    B, per = v.shape
    out = np.zeros(B, np.float32)
    for bi in range(B):
        def block_sum(vals):
            pad = np.zeros(-(-per // XS_THREADS) * XS_THREADS, np.float32)
            pad[:per] = vals
            acc = np.zeros(XS_THREADS, np.float32)
            for row in pad.reshape(-1, XS_THREADS):
                acc = acc + row
            w = acc.reshape(-1, 64)
            for o in (32, 16, 8, 4, 2, 1):
                w = w + w[:, np.arange(64) ^ o]
            tot = t(0)
            for i in range(w.shape[0]):
                tot = t(tot + w[i, 0])
            return tot

        m = t(block_sum(v[bi]) / t(per))
        d = (v[bi] - m).astype(np.float32)
        out[bi] = np.sqrt(t(block_sum((d * d).astype(np.float32)) / t(per)))
    return out


@pytest.mark.parametrize("per", [1, 5, 257, 3 * 32 * 32 + 3])
def test_fp32_restatement_of_sigma_and_f_stays_inside_the_budgets(per):
    rng = np.random.default_rng(5000 + per)
    ec = (rng.standard_normal((3, per)) * 1.3 + 0.4).astype(np.float32)
    eg = (ec * 2.5 + rng.standard_normal((3, per)).astype(np.float32)).astype(np.float32)
    eg[2] = 0.75                                   # a constant image: sigma_g == 0, f = 1
    sc, bc = sigma_budget(ec)
    sg, bg = sigma_budget(eg)
    gc, gg = sigma_fp32(ec), sigma_fp32(eg)
    assert (np.abs(gc - sc) <= bc).all() and (np.abs(gg - sg) <= bg).all(), (np.abs(gc - sc) / np.maximum(bc, 1e-300))
    assert gg[2] == 0.0 and sg[2] == 0.0
    t = np.float32
    phi = 0.7
    with np.errstate(divide="ignore", invalid="ignore"):
        f32 = np.where(gg == 0, t(1), t(phi) * (gc / gg) + (t(1) - t(phi)))
    f, bf = factor_budget(sc, bc, sg, bg, phi)
    assert (np.abs(f32 - f) <= bf).all() and f[2] == 1.0 and f32[2] == 1.0
    want = XR.rescale_factor(torch.from_numpy(ec), torch.from_numpy(eg), phi).numpy()
    assert np.allclose(f, want, rtol=1e-13, atol=0)
    if per > 1:   # the mutant that forgets to centre is far outside (on a sample whose mean is not by chance near 0)
        raw = np.sqrt((ec.astype(np.float64) ** 2).mean(axis=1))
        assert (np.abs(raw - sc) > 100 * bc).any()
