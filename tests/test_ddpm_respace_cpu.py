"""CPU: sampling a DDPM net on a sub-sequence of its steps - the schedule algebra of DDPM.respace against the fp64 restatement
(tests/ddpm_respace_ref.py), the step identities, the element-wise budgets of the new step kernels proven on an fp32 restatement in the
kernels' operation order, the RePaint walk, the time the net sees, the Python surface and the new symbols.

Budgets (the form of mi355_lowres_seed's test, (r + 1) 2^-24 M against fp64 from the fp32 inputs; r = roundings on the longest path):
  ddim_eta_step: r = 10, M = (sa + sb / b)(|a x| + |b e|) + sb |a x| / b + |sigma z|,  a = c_recip, b = c_recipm1
  renoise_step : r = 3,  M = |a x| + |b z|
"""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import ddpm_respace_ref as R

EPS32 = 2.0 ** -24
STEPS7 = [0, 3, 4, 17, 40, 41, 99]
PAIRS = [(100, STEPS7), (1000, 50), (1000, [999]), (25, [0, 1, 2, 24])]


def _ddpm(Ns):
    from image_diffusion.sde_diffusion import DDPM

    return DDPM(Ns)


def _steps(Ns, ts):
    return R.even_steps(Ns, ts) if isinstance(ts, int) else tuple(ts)


# ---- tables -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ns,ts", PAIRS)
def test_respaced_tables_are_the_restatement_rounded_once(Ns, ts):
    from image_diffusion.sde_diffusion import TABLE_NAMES, RespacedDDPM

    base = _ddpm(Ns)
    r = base.respace(ts)
    steps = _steps(Ns, ts)
    assert isinstance(r, RespacedDDPM) and r.Ns == len(steps) and r.timesteps == steps and r.base_Ns == Ns
    assert all(isinstance(t, int) for t in r.timesteps)
    assert [n for n, _ in r.named_buffers()] == list(TABLE_NAMES) == [n for n, _ in base.named_buffers()]
    assert (r.tmin, r.tmax) == (base.tmin, base.tmax) and r.ts is base.ts
    acp = base.alphas_cumprod.numpy()
    want = R.tables32(acp, steps)
    for name in TABLE_NAMES:
        got = getattr(r, name).numpy()
        assert got.dtype == np.float32 and np.isfinite(got).all(), name
        if name.startswith("log_") or name == "posterior_log_variance_clipped":   # libm's log against torch's: one ulp
            ulp = np.spacing(np.abs(want[name]))
            assert (np.abs(got.astype(np.float64) - want[name].astype(np.float64)) <= ulp).all(), name
        else:
            assert np.array_equal(got, want[name]), name
    assert np.array_equal(r.alphas_cumprod.numpy(), acp[list(steps)])          # the base's values, bit for bit
    assert np.array_equal(r.alphas_cumprod_prev.numpy()[1:], acp[list(steps)][:-1]) and r.alphas_cumprod_prev[0] == 1.0
    # DDIM(eta = 1): 1 - acp_prev - sigma^2 >= 0 in fp32, sigma^2 is the posterior variance
    sg = r.ddim_sigma(1.0)
    assert sg.dtype == torch.float32 and tuple(sg.shape) == (r.Ns,) and sg.device.type == "cpu"
    prev32 = r.alphas_cumprod_prev.numpy()
    assert ((np.float32(1.0) - prev32) - sg.numpy() * sg.numpy() >= 0).all()
    T = R.tables64(acp, steps)
    s64 = R.ddim_sigma64(T["alphas_cumprod"], T["alphas_cumprod_prev"], 1.0)
    assert np.array_equal(sg.numpy(), s64.astype(np.float32))
    # both sides are values below 1 formed by a handful of fp64 roundings each (two square roots and a square against two products and a
    # quotient): a few units of 2^-53, the 1e-16 these four schedules show in numpy; held to 4 * 2^-53
    assert np.abs(s64 ** 2 - T["posterior_variance"]).max() <= 4 * 2.0 ** -53
    assert np.array_equal(r.ddim_sigma(0.5).numpy(), (0.5 * s64).astype(np.float32)) and not r.ddim_sigma(0.0).any()


def test_identity_respacing_against_the_fp32_built_base():
    """respace(range(Ns)) rebuilds the base's tables in fp64 from its fp32 alphas_cumprod; the base built them in fp32 from a cumprod whose
    entries each carry up to one rounding per factor.  alphas' = acp_k / acp_{k-1} therefore differs from the base's alphas_k by at most
    the two cumprod entries' own relative errors, (2 k + 1) 2^-24 at step k: that bound is asserted, the measured figure printed."""
    for Ns in (25, 100, 1000):
        base = _ddpm(Ns)
        r = base.respace(range(Ns))
        assert r.timesteps == tuple(range(Ns)) and np.array_equal(r.alphas_cumprod.numpy(), base.alphas_cumprod.numpy())
        k = np.arange(Ns, dtype=np.float64)
        rel = np.abs(r.alphas.numpy().astype(np.float64) / base.alphas.numpy().astype(np.float64) - 1.0)
        print(f"Ns = {Ns}: max |alphas'/alphas - 1| = {rel.max():.3e} (bound at its step {((2 * k + 2) * EPS32)[rel.argmax()]:.3e})")
        assert (rel <= (2 * k + 2) * EPS32).all()


@pytest.mark.parametrize("Ns,ts", PAIRS)
def test_ddim_eta1_is_the_ancestral_step_in_fp64(Ns, ts):
    """DDIM(eta = 1)'s mean is the posterior mean and its variance the posterior variance (Song et al. 2021, section 4.1), to 1e-10."""
    T = R.tables64(_ddpm(Ns).alphas_cumprod.numpy(), _steps(Ns, ts))
    sg = R.ddim_sigma64(T["alphas_cumprod"], T["alphas_cumprod_prev"], 1.0)
    rng = np.random.default_rng(7)
    worst = 0.0
    for i in range(len(sg)):
        a, b = T["sqrt_recip_alphas_cumprod"][i], T["sqrt_recipm1_alphas_cumprod"][i]
        x0 = rng.uniform(-0.99, 0.99, 64)                # unclipped: the identity is about the unclipped predictor
        e = rng.standard_normal(64)
        x = (x0 + b * e) / a
        ddim = R.ddim_eta_step(x, e, None, a, b, T["alphas_cumprod_prev"][i], sg[i])
        post = R.ancestral_step(x, e, None, T, i)
        worst = max(worst, float(np.abs(ddim - post).max()), abs(sg[i] ** 2 - T["posterior_variance"][i]))
    print(f"Ns = {Ns}: DDIM(1) mean vs posterior mean, sigma^2 vs posterior variance: {worst:.2e}")
    assert worst <= 1e-10


# ---- the kernels' arithmetic in fp32 numpy, in the kernels' operation order, inside the budgets ------------------------------------------

def step_inputs(n, a, b, seed):
    """x, eps, z (fp32) with about a third of pre = a x - b eps outside [-1, 1], planted pre = +1 and -1 (eps = 0, x = +-1 / a) and one NaN."""
    rng = np.random.default_rng(seed)
    a32, b32 = np.float32(a), np.float32(b)
    pre = rng.uniform(-1.5, 1.5, n)
    eps = rng.standard_normal(n).astype(np.float32)
    x = ((pre + float(b32) * eps.astype(np.float64)) / float(a32)).astype(np.float32)
    z = rng.standard_normal(n).astype(np.float32)
    if n >= 8:
        x[n // 3], eps[n // 3] = np.float32(1.0) / a32, 0.0
        x[n // 2], eps[n // 2] = np.float32(-1.0) / a32, 0.0
        x[n // 5] = np.nan
    return x, eps, z


def ddim_eta_budget(x, eps, z, a, b, acp_prev, sigma):
    """-> (fp64 result from the fp32 inputs, (r + 1) 2^-24 M with r = 10)."""
    a, b, p, s = (float(np.float32(v)) for v in (a, b, acp_prev, sigma))
    x, eps = x.astype(np.float64), eps.astype(np.float64)
    zz = None if z is None else z.astype(np.float64)
    want = R.ddim_eta_step(x, eps, zz, a, b, p, s)
    sa, sb = math.sqrt(p), math.sqrt(max(1.0 - p - s * s, 0.0))
    M = (sa + sb / b) * (np.abs(a * x) + np.abs(b * eps)) + sb * np.abs(a * x) / b + (0.0 if zz is None else np.abs(s * zz))
    return want, 11 * EPS32 * M


def renoise_budget(x, z, a, b):
    a, b = float(np.float32(a)), float(np.float32(b))
    x, z = x.astype(np.float64), z.astype(np.float64)
    return R.renoise_step(x, z, a, b), 4 * EPS32 * (np.abs(a * x) + np.abs(b * z))


def _ddim_eta_fp32(x, eps, z, a, b, acp_prev, sigma):
    f = np.float32
    a, b, p, s = f(a), f(b), f(acp_prev), f(sigma)
    sa, sb = np.sqrt(p), np.sqrt(np.maximum((f(1.0) - p) - s * s, f(0.0)))
    ax = a * x
    pre = ax - b * eps
    x0 = np.where(pre < -1, f(-1), np.where(pre > 1, f(1), pre))
    e2 = (ax - x0) / b
    m = sa * x0 + sb * e2
    return m if z is None else m + s * z


def coefficient_cases():
    r = _ddpm(100).respace(STEPS7)
    T = r.host_tables()
    sg = r.ddim_sigma(1.0)
    out = []
    for k in (0, 3, r.Ns - 1):
        for eta in (0.0, 0.5, 1.0):
            out.append((k, eta, float(T["sqrt_recip_alphas_cumprod"][k]), float(T["sqrt_recipm1_alphas_cumprod"][k]),
                        float(T["alphas_cumprod_prev"][k]), float(np.float32(eta) * sg[k]), float(T["alphas"][k].sqrt()), float(T["betas"][k].sqrt())))
    return out


def test_fp32_restatements_stay_inside_the_budgets():
    for k, eta, a, b, prev, sigma, ra, rb in coefficient_cases():
        for n in (105, 768):
            x, eps, z = step_inputs(n, a, b, 100 * k + n)
            with np.errstate(invalid="ignore"):
                want, bound = ddim_eta_budget(x, eps, z, a, b, prev, sigma)
                got = _ddim_eta_fp32(x, eps, z, a, b, prev, sigma).astype(np.float64)
                pre = float(np.float32(a)) * x.astype(np.float64) - float(np.float32(b)) * eps.astype(np.float64)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and nan.sum() == 1
            frac = float((np.abs(pre[~nan]) > 1).mean())
            assert 0.2 <= frac <= 0.5, frac
            ratio = float((np.abs(got - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max())
            assert ratio <= 1.0, (k, eta, n, ratio)
            want, bound = renoise_budget(x, z, ra, rb)
            got = (np.float32(ra) * x + np.float32(rb) * z).astype(np.float64)
            nan = np.isnan(want)
            assert (np.abs(got - want)[~nan] <= bound[~nan]).all(), (k, n)


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,j,r", [(6, 2, 2), (7, 3, 3), (25, 5, 2), (4, 1, 4), (5, 10, 3), (1, 1, 1), (8, 2, 1)])
def test_repaint_walk(K, j, r):
    from image_diffusion.conditioning import repaint_walk

    w = repaint_walk(K, j, r)
    assert w == R.repaint_levels(K, j, r)
    assert w[0] == K and w[-1] == 0 and all(abs(b - a) == 1 for a, b in zip(w, w[1:])) and all(0 <= v <= K for v in w)
    down = sum(b < a for a, b in zip(w, w[1:]))
    up = len(w) - 1 - down
    n_jumps = len(range(0, K - j, j)) * (r - 1)
    assert up == n_jumps * j and down == K + up
    if r == 1:
        assert w == list(range(K, -1, -1))
    if (K, j, r) == (6, 2, 2):
        assert w == [6, 5, 4, 3, 4, 5, 4, 3, 2, 1, 2, 3, 2, 1, 0] and down == 10
    for bad in ((0, 1, 1), (4, 0, 1), (4, 1, 0)):
        with pytest.raises(ValueError):
            repaint_walk(*bad)


# ---- the time the net sees, the tags, the surface ------------------------------------------------------------------------------------------

def test_eps_model_feeds_the_training_time():
    from image_diffusion import sampling

    base = _ddpm(100)
    r = base.respace(STEPS7)
    seen = []
    net = lambda x, t: seen.append(t) or x   # noqa: E731
    eps = sampling.make_eps_model(net, r)
    x = torch.zeros(3, 1, 4, 4)
    for k in range(r.Ns):
        want = np.float32(STEPS7[k]) / np.float32(100)
        assert np.float32(r.time(k)) == want and r.time(k) == float(want)
        eps(x, k)
        eps(x, torch.full((3,), k, dtype=torch.long))
        assert float(seen[-2]) == float(want)
        assert seen[-1].dtype == torch.float32 and tuple(seen[-1].shape) == (3,) and (seen[-1].numpy() == want).all()
    for i in (0, 33, 99):   # the unrespaced chain: as before, and DDPM.time is the samplers' rounding of it
        assert np.float32(base.time(i)) == np.float32(i) / np.float32(100)
        sampling.make_eps_model(net, base)(x, torch.full((3,), i, dtype=torch.long))
        assert (seen[-1].numpy() == np.float32(i) / np.float32(100)).all()
    # the fused path is for an eps_model built for this very schedule
    assert sampling._same_schedule(eps, r) and not sampling._same_schedule(eps, base)
    assert not sampling._same_schedule(eps, base.respace([0, 3, 4, 17, 40, 42, 99]))
    assert not sampling._same_schedule(sampling.make_eps_model(net, _ddpm(7)), r)       # the same Ns, another schedule
    assert sampling._same_schedule(sampling.make_eps_model(net, base), base)
    hand = lambda x, i: x   # noqa: E731
    hand._mi355_network, hand._mi355_Ns = net, 100   # tagged with a step count alone, as before: the unrespaced chain
    assert sampling._same_schedule(hand, base) and not sampling._same_schedule(hand, _ddpm(1000).respace(100))


def test_respace_refusals():
    base = _ddpm(100)
    for bad in (1, 0, -3, 101, [], [3, 3], [5, 4], [-1, 2], [0, 100], [0.0, 1.0], [0, 2.5], "ab", None, True, 3.0, [True, 2]):
        with pytest.raises(ValueError):
            base.respace(bad)
    with pytest.raises(ValueError, match="finite and positive"):
        _ddpm(20).respace([0, 5, 19])        # the Ns <= 20 quirk is reproduced, not respaced
    assert _ddpm(20).respace([0, 5]).Ns == 2   # ... where the kept steps are finite it is an ordinary chain
    assert base.respace(2).timesteps == (0, 99) and base.respace(np.int64(4)).timesteps == (0, 33, 66, 99)
    assert base.respace(np.array([1, 50])).timesteps == (1, 50) and base.respace([7]).Ns == 1
    rr = base.respace(STEPS7).respace([1, 4, 6])   # a respacing of a respacing still points at training time
    assert rr.timesteps == (3, 40, 99) and rr.base_Ns == 100
    assert np.array_equal(rr.alphas_cumprod.numpy(), base.alphas_cumprod.numpy()[[3, 40, 99]])


def test_new_keywords_are_trailing_with_todays_defaults():
    from image_diffusion import sampling
    from mi355.engine import UNetEngine

    p = inspect.signature(UNetEngine.ddpm_sample).parameters
    assert list(p)[-4:] == ["timesteps", "train_steps", "ddim_sigma", "walk"] and all(p[k].default is None for k in list(p)[-4:])
    assert list(p)[-6:-4] == ["y", "null_label"]
    p = inspect.signature(sampling.get_ddim_sample_fn).parameters
    assert list(p) == ["eps_model", "ddpm", "likelihood", "guidance_scale", "eta"] and p["eta"].default == 0.0
    with pytest.raises(ValueError, match="eta"):
        sampling.get_ddim_sample_fn(lambda x, i: x, _ddpm(25), eta=-0.5)
    with pytest.raises(ValueError, match="scheduled call"):
        UNetEngine._ddpm_schedule({}, None, None, [0.1], None)
    with pytest.raises(ValueError, match="go together"):
        UNetEngine._ddpm_schedule({}, (0, 1), None, None, None)


def test_repaint_conditioning_type():
    from image_diffusion.conditioning import RePaint, Replacement, get_conditioning

    assert get_conditioning("repaint") is RePaint and RePaint.KEY == "repaint" and issubclass(RePaint, Replacement)
    assert RePaint.PARAMS == Replacement.PARAMS + ("jump_length", "n_resample")
    c = RePaint(0.1, 0.5, True, 0, 2, 3)
    assert (c.delta, c.start_fraction, c.noise, c.n_corrector, c.jump_length, c.n_resample) == (0.1, 0.5, True, 0, 2, 3)
    assert get_conditioning("replacement") is Replacement
    for bad in (dict(jump_length=0), dict(n_resample=0), dict(jump_length=1.5)):
        with pytest.raises(ValueError):
            RePaint(**dict(dict(delta=0.1, start_fraction=1.0, noise=True, n_corrector=0, jump_length=2, n_resample=2), **bad))


class _RecOps:
    """The step ops in eager torch on the CPU, recording what the generic samplers ask for."""

    def __init__(self):
        self.log = []

    def ddpm_step_(self, x, eps, z, *a, philox=None):
        self.log.append(("down", z is not None))
        return x

    def replace_mask_(self, x, cond, z, *a):
        self.log.append(("paste", z is not None))
        return x

    def renoise_(self, x, z, a, b, philox=None):
        self.log.append(("up", round(a * a + b * b, 5)))
        return x

    def ddim_step_(self, x, eps, *a):
        self.log.append(("ddim", False))
        return x

    def ddim_eta_step_(self, x, eps, z, cr, cm, prev, sigma, philox=None):
        self.log.append(("ddim_eta", z is not None, sigma > 0))
        return x

    def clip_(self, x, lo=-1.0, hi=1.0):
        return x.clip_(lo, hi)


def test_generic_loops_host_logic():
    """The RePaint walk and DDIM(eta) on a recording op table: the moves, the steps the net is asked for, the draws."""
    from image_diffusion import sampling
    from image_diffusion.conditioning import RePaint, Replacement, repaint_walk
    from image_diffusion.likelihoods import InPainting

    r = _ddpm(100).respace(6)
    lik = InPainting(patch_size=3, pad_value=-2)
    asked = []
    eps_model = lambda xi, i: asked.append(int(i[0])) or xi   # noqa: E731
    xT = torch.zeros(2, 1, 8, 8)
    cond = torch.full_like(xT, 0.5)
    walk = repaint_walk(6, 2, 2)
    n_draws = 10 + 9 + 4   # 10 pastes (start_fraction 1), 10 predictor steps of which one ends at level 0, 4 moves up
    rec = _RecOps()
    with sampling.use_ops(rec), sampling.injected_noise([torch.zeros_like(xT)] * n_draws):
        sampling.get_conditional_sample_fn(eps_model, r, RePaint(0.1, 1.0, True, 0, 2, 2), lik)(xT, cond)
    assert asked == [a - 1 for a, b in zip(walk, walk[1:]) if b < a] and len(asked) == 10
    assert [e[0] for e in rec.log if e[0] != "paste"] == ["down" if b < a else "up" for a, b in zip(walk, walk[1:])]
    assert all(e[1] == 1.0 for e in rec.log if e[0] == "up")                  # a^2 + b^2 = alphas + betas = 1
    assert [e for e in rec.log if e[0] == "down"][-1] == ("down", False)
    with sampling.use_ops(rec), sampling.injected_noise([torch.zeros_like(xT)] * (n_draws - 1)), pytest.raises(RuntimeError, match="exhausted"):
        sampling.get_conditional_sample_fn(eps_model, r, RePaint(0.1, 1.0, True, 0, 2, 2), lik)(xT, cond)
    # n_resample = 1: the calls of Replacement
    logs = []
    for c in (RePaint(0.1, 0.5, True, 0, 2, 1), Replacement(0.1, 0.5, True, 0)):
        rec.log.clear()
        with sampling.use_ops(rec), sampling.injected_noise([torch.zeros_like(xT)] * 8):
            sampling.get_conditional_sample_fn(eps_model, r, c, lik)(xT, cond)
        logs.append(list(rec.log))
    assert logs[0] == logs[1] and len(logs[0]) == 6 + 3
    # DDIM: eta = 0 is the deterministic kernel and draws nothing; eta > 0 draws on every step but the last
    for eta, want in ((0.0, [("ddim", False)] * 6), (0.5, [("ddim_eta", True, True)] * 5 + [("ddim_eta", False, False)])):
        rec.log.clear()
        asked.clear()
        with sampling.use_ops(rec), sampling.injected_noise([torch.zeros_like(xT)] * 5):
            sampling.get_ddim_sample_fn(eps_model, r, eta=eta)(xT)
        assert rec.log == want and asked == [5, 4, 3, 2, 1, 0]


# ---- the library ---------------------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("mi355_ddim_eta_step", "mi355_ddim_eta_cfg_step", "mi355_renoise_step", "mi355_ddpm_sample_sched", "mi355_ddpm_cfg_sample_sched")


def test_library_exports_the_new_symbols():
    import os
    import re

    import __graft_entry__ as ge
    from tests.conftest import REPO

    ge.build()
    from mi355 import _lib

    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "mi355_sampler.h")).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(L, name) and name in declared, name
    assert "mi355_ddpm_schedule" not in declared and "typedef struct mi355_ddpm_schedule" in header
    assert L.mi355_version() == 108   # additive: new symbols only
    assert [f for f, _ in _lib.DDPMScheduleC._fields_] == ["steps", "train_steps", "ddim_sigma", "walk", "n_walk", "renoise_a", "renoise_b"]
    # a null handle is refused before anything else; a negative sigma and a bad Philox offset before any launch (n = 0: nothing would run)
    assert L.mi355_ddpm_sample_sched(None, None, 1, None, None, None, None, None, 0, 1, None, 0, None) < 0
    assert L.mi355_ddpm_cfg_sample_sched(None, None, 1, None, None, 0, 1.0, None, None, None, None, None, 0, 1, None, 0, None) < 0
    assert L.mi355_ddim_eta_step(None, None, None, 1.0, 1.0, 0.5, -0.1, 0, 0, 0, 0, None) == -1 and b"sigma" in L.mi355_last_error()
    assert L.mi355_ddim_eta_step(None, None, None, 1.0, 1.0, 0.5, float("nan"), 0, 0, 0, 0, None) == -1
    assert L.mi355_ddim_eta_step(None, None, None, 1.0, 1.0, 0.5, float("inf"), 0, 0, 0, 0, None) == -1
    assert L.mi355_renoise_step(None, None, 1.0, 1.0, 1, 0, 6, 0, None) == -1 and b"multiple of 4" in L.mi355_last_error()
    assert L.mi355_ddim_eta_step(None, None, None, 1.0, 1.0, 0.5, 0.1, 0, 0, 0, 0, None) == 0       # n = 0: nothing to do
