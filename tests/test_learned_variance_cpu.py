"""CPU: learned-variance DDPM nets (DDPM.with_learned_variance, DDPM.from_betas; mi355_ddpm_lv_sample) - the tables of a chain built from its
betas against an independent numpy evaluation, the times and schedule keys under a time_scale, the views, every refusal that needs no GPU (the
Python ones by message, the library's through the ABI: they come before any launch and before the handle is looked at), and the rounding
budget the GPU test holds mi355_ddpm_lv_step to, proven here on an fp32 numpy restatement of the stated operation sequence.

Budget of one learned-variance step (fp64 from the fp32 inputs, EPS32 = 2^-24, first-order count r, bound (r + 1) EPS32 M as
tests/test_x0_shaping_cpu.py does):
  mean    r = 6: x0 = clip(c_recip x - c_recipm1 eps) has three roundings of values bounded by P = |c_recip x| + |c_recipm1 eps| (the clip is exact
          and 1-Lipschitz); coef1 x0 adds its product, then the two sums; coef2 x: a product and two sums.  M = |coef1| P + |coef2 x| + |sigma z|
          (the last sum rounds the whole result).
  logvar  frac = (v + 1) * 0.5: one rounding (the halving is exact), |d frac| <= EPS32 |frac|; 1 - frac: |d| <= EPS32 (|frac| + |1 - frac|);
          frac max_log: (1 + 1) EPS32 |frac| |max_log|; (1 - frac) min_log: EPS32 (|frac| + 2 |1 - frac|) |min_log|; their sum rounds once more:
          |d logvar| <= EPS32 (3 |frac| |max_log| + (|frac| + 3 |1 - frac|) |min_log|).
  sigma   = exp(0.5 logvar): the halving is exact, the exponential passes 0.5 |d logvar| on as a relative error and adds its own, at most one
          fp32 ulp = 2 EPS32 (the device's expf and numpy's alike); sigma z: one product.  Relative to |sigma z|:
          0.5 |d logvar| + (2 + 1 + 1) EPS32, the last 1 being the (r + 1) of the convention.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import learned_variance_ref as LR
from tests.test_ddpm_respace_cpu import EPS32, STEPS7, step_inputs

R_MEAN = 6
PERS = [1, 5, 257, 3 * 32 * 32 + 3]
B = 3


def _ddpm(Ns):
    from image_diffusion.sde_diffusion import DDPM

    return DDPM(Ns)


def _ulps(got32, want64):
    """|got - want| in units of the fp32 spacing at want (got fp32 tensor / array, want fp64 array)."""
    got = np.asarray(got32, np.float32).astype(np.float64)
    want = np.asarray(want64, np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want.astype(np.float32)).astype(np.float32)).astype(np.float64)


# ---- tables of from_betas, linear_betas, cosine_betas ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,T", [("linear", 1000), ("linear", 100), ("cosine", 1000), ("cosine", 100), ("cosine", 7)])
def test_tables_from_betas_are_the_fp64_values_rounded_once(name, T):
    from image_diffusion import sde_diffusion as SD

    betas = getattr(SD, name + "_betas")(T)
    want_b = getattr(LR, name + "_betas")(T)
    assert betas.dtype == np.float64 and betas.shape == (T,)
    np.testing.assert_allclose(betas, want_b, rtol=4e-16 * 8, atol=0)     # a few fp64 ulps: linspace and libm differ by that
    d = SD.DDPM.from_betas(betas, time_scale=T)
    assert d.Ns == T and [n for n, _ in d.named_buffers()] == list(SD.TABLE_NAMES)
    ref = LR.tables_from_betas(betas)
    for n in SD.TABLE_NAMES:
        got = getattr(d, n)
        assert got.dtype == torch.float32 and got.shape == (T,)
        u = _ulps(got.numpy(), ref[n])
        assert float(u.max()) <= 1.0, (n, float(u.max()))
    u = _ulps(d.max_log().numpy(), np.log(betas))
    assert float(u.max()) <= 1.0
    assert d.host_tables()["betas"].dtype == torch.float32
    if name == "linear":
        assert betas[0] == pytest.approx(1e-4 * 1000 / T, rel=1e-15) and betas[-1] == pytest.approx(0.02 * 1000 / T, rel=1e-15)
    else:
        assert float(betas.max()) <= 0.999 and (T < 100 or float(betas.max()) == 0.999)


def test_from_betas_of_a_chains_own_betas_gives_them_back():
    from image_diffusion.sde_diffusion import DDPM

    d = _ddpm(100)
    e = DDPM.from_betas(d.betas.double())
    assert torch.equal(e.betas.view(torch.int32), d.betas.view(torch.int32)) and e.time_scale == 1.0
    assert [e.time(k) for k in range(100)] == [d.time(k) for k in range(100)]
    assert e.tmin == d.tmin and e.tmax == d.tmax and torch.equal(e.ts, d.ts)
    # the other tables: the fp32-built chain against the fp64-built one, a few fp32 ulps apart where the formula is well conditioned
    np.testing.assert_allclose(e.alphas_cumprod.numpy(), d.alphas_cumprod.numpy(), rtol=1e-5)
    f = DDPM.from_betas(list(d.betas.double().numpy()))
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(e.named_buffers(), f.named_buffers()))


def test_from_betas_refusals():
    from image_diffusion import sde_diffusion as SD

    for bad in ([0.1, 1.0], [0.1, 1.5], [0.0, 0.1], [-0.1, 0.1], [0.1, float("nan")], [0.1, float("inf")], []):
        with pytest.raises(ValueError):
            SD.DDPM.from_betas(bad)
    for ts in (0.0, -1.0, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="time_scale"):
            SD.DDPM.from_betas([0.1, 0.2], time_scale=ts)
    for T in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            SD.linear_betas(T)
        with pytest.raises(ValueError):
            SD.cosine_betas(T)


# ---- times and keys ----------------------------------------------------------------------------------------------------------------------------

def test_times_and_schedule_keys_under_a_time_scale():
    from image_diffusion import sde_diffusion as SD
    from image_diffusion.sampling import _sched_key, make_eps_model

    T = 100
    betas = SD.cosine_betas(T)
    keys = set()
    for scale in (1, T, 1000):
        d = SD.DDPM.from_betas(betas, time_scale=scale)
        r = d.respace(STEPS7)
        rr = r.respace([1, 4, 6])
        assert r.time_scale == float(scale) == rr.time_scale and r.base_Ns == T
        f32 = np.float32
        for k in (0, 1, 57, 99):
            assert d.time(k) == float(f32(k) * f32(scale) / f32(T))
        for k, tau in enumerate(STEPS7):
            assert r.time(k) == float(f32(tau) * f32(scale) / f32(T))
        assert [rr.time(k) for k in range(3)] == [r.time(k) for k in (1, 4, 6)]
        if scale == T:     # the integer step itself
            assert [r.time(k) for k in range(r.Ns)] == [float(t) for t in STEPS7]
        keys |= {_sched_key(d), _sched_key(r)}
        assert _sched_key(d.with_learned_variance()) == _sched_key(d)
        # eps_model feeds those times, for an int and for the samplers' long tensor
        seen = []
        em = make_eps_model(lambda x, t: seen.append(t) or x, r)
        em(torch.zeros(2, 1), 3)
        em(torch.zeros(2, 1), torch.tensor([3, 5]))
        assert seen[0] == r.time(3) and seen[1].tolist() == [r.time(3), r.time(5)]
        if scale != 1:   # (time_scale 1 on all steps: the expression the unscheduled chain always fed)
            em2 = make_eps_model(lambda x, t: seen.append(t) or x, d)
            em2(torch.zeros(2, 1), torch.tensor([7, 99]))
            assert seen[2].tolist() == [d.time(7), d.time(99)]
    assert len(keys) == 6
    # a chain without a time_scale keeps the key it had
    p = _ddpm(100)
    assert _sched_key(p) == (100, None) and _sched_key(p.respace(STEPS7)) == (100, tuple(STEPS7))
    assert _sched_key(SD.DDPM.from_betas(betas)) == (100, None)


# ---- views ---------------------------------------------------------------------------------------------------------------------------------------

def test_learned_variance_views_commute_with_respace_and_shaping():
    from image_diffusion.sde_diffusion import TABLE_NAMES, RespacedDDPM

    d = _ddpm(100)
    assert d.learned_variance is False and d.respace(5).learned_variance is False
    v = d.with_learned_variance()
    assert v.learned_variance is True and d.learned_variance is False and type(v) is type(d) and v is not d
    assert all(a is b for (_, a), (_, b) in zip(v.named_buffers(), d.named_buffers())) and list(v.state_dict()) == list(d.state_dict())
    assert v.with_learned_variance(False).learned_variance is False
    a, b = d.respace(STEPS7).with_learned_variance(), d.with_learned_variance().respace(STEPS7)
    assert isinstance(a, RespacedDDPM) and isinstance(b, RespacedDDPM) and a.learned_variance and b.learned_variance
    assert a.timesteps == b.timesteps and all(torch.equal(x, y) for (_, x), (_, y) in zip(a.named_buffers(), b.named_buffers()))
    assert torch.equal(a.max_log(), b.max_log())
    s1, s2 = v.with_x0_shaping(0.9).respace(STEPS7), d.with_x0_shaping(0.9).respace(STEPS7).with_learned_variance()
    assert s1.learned_variance and s2.learned_variance and s1.x0_shaping == s2.x0_shaping is not None
    assert [n for n, _ in a.named_buffers()] == list(TABLE_NAMES)
    # max_log of the respaced chain: log of its own betas, 1 - acp'_k / acp'_{k-1}, in fp64, rounded once
    acp = d.alphas_cumprod.double().numpy()[STEPS7]
    prev = np.concatenate(([1.0], acp[:-1]))
    want = np.log(1.0 - acp / prev)
    ml = a.max_log()
    assert ml.dtype == torch.float32 and ml.device.type == "cpu"
    assert np.array_equal(ml.numpy(), want.astype(np.float32))
    # and of the base: log of its fp32 betas
    assert np.array_equal(v.max_log().numpy(), np.log(d.betas.double().numpy()).astype(np.float32))
    # min_log <= max_log wherever the posterior variance is not clipped: the range is a range
    assert bool((a.host_tables()["posterior_log_variance_clipped"][1:] <= ml[1:]).all())


# ---- Python refusals -------------------------------------------------------------------------------------------------------------------------------

def test_samplers_refuse_what_a_learned_variance_chain_cannot_do():
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance, ReconstructionGuidance, Replacement
    from image_diffusion.likelihoods import InPainting

    d = _ddpm(100).respace(5)
    lv = d.with_learned_variance()
    lik = InPainting(patch_size=4, pad_value=-2)
    wide = lambda xi, i: torch.zeros(xi.shape[0], 2, 8, 8)   # noqa: E731   a learned-variance net of a one-channel state
    narrow = lambda xi, i: torch.zeros(xi.shape[0], 1, 8, 8)   # noqa: E731
    xT = torch.zeros(2, 1, 8, 8)
    am, cfg, rep = Amortized(1.0, 0, 0.1), ClassifierFreeGuidance(1.0, 0, 0.1, 2.0), Replacement(0.1, 1.0, True, 0)

    class Net:
        engine = None

    tagged = sampling.make_eps_model(Net(), lv)
    with pytest.raises(NotImplementedError, match="ReconstructionGuidance.*learned-variance"):
        sampling.get_conditional_sample_fn(tagged, lv, ReconstructionGuidance(1.0, 1.0, "before", 0, 0.1), lik)
    sampling.get_conditional_sample_fn(sampling.make_eps_model(Net(), d), d, ReconstructionGuidance(1.0, 1.0, "before", 0, 0.1), lik)
    for what, chain in (("tiling", lv.with_tiling(sampling.Tiling(stride=4))), ("feature_cache", lv.with_feature_cache(sampling.FeatureCache(interval=2)))):
        for make in (lambda c: sampling.get_prior_sample_fn(wide, c, am, lik), lambda c: sampling.get_conditional_sample_fn(wide, c, am, lik),
                     lambda c: sampling.get_conditional_sample_fn(wide, c, rep, lik), lambda c: sampling.get_ddim_sample_fn(wide, c)):
            with pytest.raises(NotImplementedError, match=what + ".*learned-variance"):
                make(chain)
    for make in (lambda t: sampling.get_prior_sample_fn(wide, lv, am, lik, tiling=t), lambda t: sampling.get_conditional_sample_fn(wide, lv, am, lik, tiling=t)):
        with pytest.raises(NotImplementedError, match="tiling.*learned-variance"):
            make(sampling.Tiling(stride=4))
    with pytest.raises(NotImplementedError, match="feature_cache.*learned-variance"):
        sampling.get_prior_sample_fn(wide, lv, am, lik, feature_cache=sampling.FeatureCache(interval=2))
    shaped = lv.with_x0_shaping(0.9)
    with pytest.raises(NotImplementedError, match="x0_shaping.*learned-variance"):
        sampling.get_dpm_solver_sample_fn(wide, shaped)
    with pytest.raises(NotImplementedError, match="x0_shaping.*learned-variance"):
        sampling.get_ddim_sample_fn(wide, shaped)
    for make, args in ((lambda: sampling.get_prior_sample_fn(wide, shaped, am, lik), (xT,)),
                       (lambda: sampling.get_conditional_sample_fn(wide, shaped, am, lik), (xT, xT)),
                       (lambda: sampling.get_conditional_sample_fn(wide, shaped, cfg, lik), (xT, xT)),
                       (lambda: sampling.get_conditional_sample_fn(wide, shaped, rep, lik), (xT, xT))):
        with pytest.raises(NotImplementedError, match="x0_shaping.*learned-variance"):
            make()(*args)
    # the net's width against the chain, both ways
    for fn, args in ((sampling.get_prior_sample_fn(narrow, lv, am, lik), (xT,)), (sampling.get_conditional_sample_fn(narrow, lv, cfg, lik), (xT, xT)),
                     (sampling.get_ddim_sample_fn(narrow, lv), (xT,)), (sampling.get_dpm_solver_sample_fn(narrow, lv), (xT,))):
        with pytest.raises(ValueError, match="twice the state's channels"):
            fn(*args)

    class Eng:
        out_channels = 2

    with pytest.raises(ValueError, match="with_learned_variance"):
        sampling._check_engine_width(Eng(), xT, None)
    with pytest.raises(ValueError, match="twice the state's channels"):
        sampling._check_engine_width(type("E", (), dict(out_channels=1))(), xT, lv.max_log())
    sampling._check_engine_width(Eng(), xT, lv.max_log())
    sampling._check_engine_width(type("E", (), dict(out_channels=1))(), xT, None)


def test_generic_loops_pass_the_wide_output_whole():
    """The host loops on a learned-variance chain: one ddpm_lv_step_ per step with i > 0 (the 2C output itself, nothing sliced), the plain step
    at i = 0 and the corrector through strided_step_; draws numbered as on a plain chain."""
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance
    from image_diffusion.likelihoods import InPainting

    class Rec:
        def __init__(self):
            self.calls = []

        def ddpm_lv_step_(self, x, out, z, cr, crm1, c1, c2, min_log, max_log, philox=None, w=None):
            self.calls.append(("lv", tuple(x.shape), tuple(out.shape), z is not None or philox is not None, min_log, max_log, w))
            return x

        def strided_step_(self, kind, x, out, cr, crm1, a, b=0.0, c=0.0, sigma=0.0, z=None, philox=None, hist=None, w=None):
            self.calls.append((kind, tuple(x.shape), tuple(out.shape), z is not None or philox is not None, hist is not None, w))
            return x

        def clip_(self, x, lo, hi):
            return x

    lv = _ddpm(100).respace(STEPS7).with_learned_variance()
    T, ml = lv.host_tables(), lv.max_log()
    lik = InPainting(patch_size=4, pad_value=-2)
    wide = lambda xi, i: torch.zeros(xi.shape[0], 2, 8, 8)   # noqa: E731
    xT = torch.zeros(2, 1, 8, 8)
    rec = Rec()
    with sampling.use_ops(rec):
        sampling.get_conditional_sample_fn(wide, lv, Amortized(1.0, 1, 0.1), lik)(xT, xT)
    kinds = [c[0] for c in rec.calls]
    assert kinds == ["lv", "corrector"] * 6 + ["ddpm", "corrector"]
    assert all(c[1] == (2, 1, 8, 8) and c[2] == (2, 2, 8, 8) for c in rec.calls)
    lvs = [c for c in rec.calls if c[0] == "lv"]
    assert [c[4] for c in lvs] == [float(T["posterior_log_variance_clipped"][i]) for i in range(6, 0, -1)]
    assert [c[5] for c in lvs] == [float(ml[i]) for i in range(6, 0, -1)] and all(c[3] and c[6] is None for c in lvs)
    assert rec.calls[-2][3] is False      # step 0 draws nothing
    rec = Rec()
    with sampling.use_ops(rec):
        sampling.get_conditional_sample_fn(wide, lv, ClassifierFreeGuidance(1.0, 0, 0.1, 3.0), lik)(xT, xT)
    assert [c[0] for c in rec.calls] == ["lv"] * 6 + ["ddpm"] and all(c[1] == (4, 1, 8, 8) and c[2] == (4, 2, 8, 8) and c[-1] == 3.0 for c in rec.calls)
    rec = Rec()
    with sampling.use_ops(rec):
        sampling.get_ddim_sample_fn(wide, lv)(xT)
        sampling.get_ddim_sample_fn(wide, lv, eta=0.5)(xT)
        sampling.get_dpm_solver_sample_fn(wide, lv)(xT)
        sampling.get_ddim_sample_fn(wide, lv, lik, guidance_scale=2.0)(xT, xT)
    assert [c[0] for c in rec.calls] == ["ddim"] * 7 + ["ddim_eta"] * 7 + ["dpmpp"] * 7 + ["ddim"] * 7
    assert [c[3] for c in rec.calls[7:14]] == [True] * 6 + [False] and all(c[4] for c in rec.calls[14:21])
    assert all(c[2][1] == 2 for c in rec.calls) and all(c[1] == (4, 1, 8, 8) and c[-1] == 2.0 for c in rec.calls[21:])


# ---- the library's refusals, through the ABI -------------------------------------------------------------------------------------------------------

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
    for name in ("mi355_ddpm_lv_workspace_bytes", "mi355_ddpm_lv_sample", "mi355_ddpm_lv_step", "mi355_strided_step"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.mi355_version() == 108
    d = _ddpm(100).respace(STEPS7)
    tb, keep = _tables_c(d)
    opt = _lib.DDPMOptionsC(_lib.DDPM_PRIOR, 0, 0.1, 1e-5, 1.0, 1.0, 1, -2.0, -2.0, 1, 0)
    steps = (C.c_int32 * d.Ns)(*d.timesteps)
    sd = _lib.DDPMScheduleC()
    sd.steps, sd.train_steps = C.cast(steps, C.POINTER(C.c_int32)), d.base_Ns
    cs = [c.contiguous() for c in d.dpm_solver_coefs(2)]
    ms = _lib.MultistepScheduleC()
    ms.steps, ms.train_steps = sd.steps, d.base_Ns
    ms.cx, ms.c0, ms.c1 = (C.cast(c.data_ptr(), C.POINTER(C.c_float)) for c in cs)
    fp = C.POINTER(C.c_float)

    def var(learned, max_log, times):
        v = _lib.DDPMVarianceC(learned, None, None)
        v._keep = [None if a is None else torch.tensor(a, dtype=torch.float32) for a in (max_log, times)]
        v.max_log, v.times = (None if t is None else C.cast(t.data_ptr(), fp) for t in v._keep)
        return v

    def call(v, guided=0, sched=None, msched=None, noise=None):
        return L.mi355_ddpm_lv_sample(None, None, 1, None, None, 0, guided, 2.0, None, C.byref(tb), C.byref(opt),
                                      C.byref(sched) if sched is not None else None, C.byref(msched) if msched is not None else None,
                                      C.byref(v) if v is not None else None, noise, 0, 3, None, 0, None)

    ml = d.with_learned_variance().max_log().tolist()
    good_t = [d.time(k) for k in range(d.Ns)]
    inf, nan = float("inf"), float("nan")
    cases = [(var(2, ml, None), b"var->learned"), (var(-1, ml, None), b"var->learned"), (var(1, None, None), b"var->max_log"),
             (var(1, ml[:3] + [nan] + ml[4:], None), b"var->max_log"), (var(1, ml[:6] + [-inf], None), b"var->max_log"),
             (var(1, [inf] + ml[1:], None), b"var->max_log"), (var(0, None, good_t[:2] + [nan] + good_t[3:]), b"var->times"),
             (var(1, ml, [inf] + good_t[1:]), b"var->times")]
    for v, msg in cases:
        for kw in ({}, dict(sched=sd)):
            assert call(v, **kw) == -1 and msg in L.mi355_last_error() and b"ddpm_lv_sample" in L.mi355_last_error(), (msg, kw)
    # a non-finite max_log where the variance is not learned is not read
    assert call(var(0, [nan] * d.Ns, None)) == -1 and b"bad argument (net, x, workspace, batch)" in L.mi355_last_error()
    assert call(None, sched=sd, msched=ms) == -1 and b"both sched and msched" in L.mi355_last_error()
    # the loops' own refusals, under this entry point's name; then, everything in order, the missing handle
    bad = _lib.DDPMScheduleC()
    bad.steps, bad.train_steps = sd.steps, 0
    assert call(var(1, ml, None), sched=bad) == -1 and b"ddpm_lv_sample: train_steps" in L.mi355_last_error()
    assert call(var(1, ml, None), msched=ms) == -1 and b"ddpm_lv_sample: opt->mode must be MI355_DDIM" in L.mi355_last_error()
    opt.mode = _lib.DDIM
    one = torch.zeros(1)
    assert call(None, msched=ms, noise=C.c_void_p(one.data_ptr())) == -1 and b"ddpm_lv_sample: noise given with msched" in L.mi355_last_error()
    for v in (None, var(0, None, None), var(1, ml, None), var(1, ml, good_t), var(0, None, good_t)):
        for kw in ({}, dict(sched=sd), dict(msched=ms)):
            assert call(v, **kw) == -1 and b"ddpm_lv_sample: bad argument (net, x, workspace, batch)" in L.mi355_last_error()
    assert L.mi355_ddpm_lv_sample(None, None, 1, None, None, 0, 0, 2.0, None, None, C.byref(opt), None, None, None, None, 0, 3, None, 0, None) == -1
    assert b"tables or opt is null" in L.mi355_last_error()
    assert L.mi355_ddpm_lv_workspace_bytes(None, 3, 0, 0) == -1 and b"ddpm_lv_workspace_bytes" in L.mi355_last_error()
    # the step ops refuse before they look at a pointer
    assert L.mi355_ddpm_lv_step(None, None, None, 0.0, None, 0, 0, 1.0, 1.0, 0.5, 0.5, -3.0, -1.0, 0, 0, 0, 3, None) == -1
    assert b"elems_per_image" in L.mi355_last_error()
    for mn, mx in ((nan, -1.0), (-3.0, inf)):      # (an empty batch: the pointers are not asked for)
        assert L.mi355_ddpm_lv_step(None, None, None, 0.0, None, 0, 16, 1.0, 1.0, 0.5, 0.5, mn, mx, 0, 0, 0, 0, None) == -1
        assert b"ddpm_lv_step: min_log and max_log must be finite" in L.mi355_last_error()
    assert L.mi355_ddpm_lv_step(None, None, None, 0.0, None, 0, 16, 1.0, 1.0, 0.5, 0.5, -3.0, -1.0, 0, 0, 0, 3, None) == -1
    assert b"ddpm_lv_step: null argument" in L.mi355_last_error()
    assert L.mi355_ddpm_lv_step(None, None, None, 0.0, None, 0, 16, 1.0, 1.0, 0.5, 0.5, -3.0, -1.0, 1, 0, 6, 3, None) == -1
    assert b"ddpm_lv_step: the Philox offset" in L.mi355_last_error()
    assert L.mi355_ddpm_lv_step(None, None, None, 0.0, None, 1, 16, 1.0, 1.0, 0.5, 0.5, -3.0, -1.0, 0, 0, 0, 3, None) == -1
    assert b"ddpm_lv_cfg_step: null argument" in L.mi355_last_error()
    sstep = lambda kind, stride, per, n, guided=0: L.mi355_strided_step(kind, None, None, stride, None, None, guided, 0.0, None, per, 1.0, 1.0, 0.5, 0.5, 0.0,  # noqa: E731
                                                                        0.0, 0, 0, 0, n, None)
    assert sstep(5, 32, 16, 48) == -1 and b"strided_step: kind" in L.mi355_last_error()
    assert sstep(0, 32, 16, 50) == -1 and b"whole images" in L.mi355_last_error()
    assert sstep(0, 8, 16, 48) == -1 and b"eps_stride" in L.mi355_last_error()
    assert sstep(4, 32, 16, 48, guided=1) == -1 and b"no guided form" in L.mi355_last_error()
    assert sstep(1, 32, 16, 48) == -1 and b"ddim_step: null argument" in L.mi355_last_error()
    assert sstep(4, 32, 16, 48) == -1 and b"null argument" in L.mi355_last_error()
    del keep


def test_engine_and_ops_signatures():
    import inspect

    from mi355.engine import UNetEngine
    from mi355.ops import Ops

    p = inspect.signature(UNetEngine.ddpm_learned).parameters
    assert list(p)[:4] == ["self", "x", "tables", "max_log"] and p["times"].default is None and p["coefs"].default is None
    q = inspect.signature(UNetEngine.ddpm_shaped).parameters      # the entry point it is patterned on keeps its arguments
    assert set(q) - {"shaping"} == set(p) - {"max_log", "times"}
    assert list(inspect.signature(Ops.ddpm_lv_step_).parameters)[:10] == ["self", "x", "out", "z", "c_recip", "c_recipm1", "coef1", "coef2", "min_log", "max_log"]


# ---- the budget -------------------------------------------------------------------------------------------------------------------------------------

def lv_cases():
    """(c_recip, c_recipm1, coef1, coef2, min_log, max_log) on DDPM(100) at 7 logSNR-even steps, at every step that draws noise."""
    d = _ddpm(100)
    r = d.respace(d.logsnr_steps(7)).with_learned_variance()
    T, ml = r.host_tables(), r.max_log()
    return [tuple(float(T[n][k]) for n in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
                                           "posterior_log_variance_clipped")) + (float(ml[k]),) for k in range(1, r.Ns)]


def lv_operands(per, a, b, seed, batch=B):
    """fp32 x [batch * per], eps and v [batch, per], z: step_inputs' state and eps (a third of x0 clipped, the planted +-1, one NaN), v uniform in
    [-3, 3] with a different offset per image (a cross-image mix-up moves sigma by far more than the budget)."""
    n = batch * per
    x, eps, z = step_inputs(n, a, b, seed)
    rng = np.random.default_rng(seed + 17)
    v = rng.uniform(-1.0, 1.0, (batch, per)) + np.linspace(-2.0, 2.0, batch)[:, None]
    return x, eps.reshape(batch, per), v.astype(np.float32), z


def lv_budget(x, eps, v, z, c):
    """-> (fp64 step result from the fp32 inputs, its bound)."""
    a, b, c1, c2, mn, mx = (float(np.float32(t)) for t in c)
    x64, e64, v64, z64 = x.astype(np.float64), eps.reshape(-1).astype(np.float64), v.reshape(-1).astype(np.float64), z.astype(np.float64)
    t = torch.from_numpy
    want = LR.lv_step(t(x64), t(e64), t(v64), t(z64), a, b, c1, c2, mn, mx).numpy()
    P = np.abs(a * x64) + np.abs(b * e64)
    frac = (v64 + 1.0) * 0.5
    dlog = EPS32 * (3 * np.abs(frac) * abs(mx) + (np.abs(frac) + 3 * np.abs(1.0 - frac)) * abs(mn))
    sz = np.abs(np.exp(0.5 * (frac * mx + (1.0 - frac) * mn)) * z64)
    return want, (R_MEAN + 1) * EPS32 * (abs(c1) * P + np.abs(c2 * x64) + sz) + sz * (0.5 * dlog + 4 * EPS32)


def lv_fp32(x, eps, v, z, c, mutant=None):
    """The stated operation sequence in fp32 numpy, every operation rounded."""
    f = np.float32
    a, b, c1, c2, mn, mx = (f(t) for t in c)
    e, vv = eps.reshape(-1), v.reshape(-1)
    if mutant == "next_image":
        vv = np.roll(v, 1, axis=0).reshape(-1)
    if mutant == "clamped":
        vv = np.clip(vv, f(-1), f(1))
    frac = (vv + f(1)) * f(0.5)
    logvar = frac * mx + (f(1) - frac) * mn
    if mutant == "swapped":
        logvar = frac * mn + (f(1) - frac) * mx
    pre = a * x - b * e
    x0 = np.where(pre < -1, f(-1), np.where(pre > 1, f(1), pre))
    mean = c1 * x0 + c2 * x
    return (mean + np.exp(f(0.5) * logvar).astype(f) * z).astype(f)


@pytest.mark.parametrize("per", PERS)
def test_fp32_restatement_of_the_learned_variance_step_stays_inside_the_budget(per):
    worst = 0.0
    broke = dict(next_image=0, clamped=0, swapped=0)
    cases = lv_cases()
    for j, c in enumerate(cases):
        x, eps, v, z = lv_operands(per, c[0], c[1], 300 * j + per)
        with np.errstate(invalid="ignore"):
            want, bound = lv_budget(x, eps, v, z, c)
            got = lv_fp32(x, eps, v, z, c)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and nan.sum() == (1 if B * per >= 8 else 0)
        worst = max(worst, float((np.abs(got.astype(np.float64) - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max()))
        for mut in broke:
            with np.errstate(invalid="ignore"):
                bad = lv_fp32(x, eps, v, z, c, mutant=mut).astype(np.float64)
            broke[mut] += bool((np.abs(bad - want)[~nan] > bound[~nan]).any())
    print(f"per = {per}: learned-variance step, fp32 restatement: max err / budget {worst:.3f}; cases broken by each mutant: {broke} of {len(cases)}")
    assert worst <= 1.0
    assert all(n == len(cases) for n in broke.values())
    assert len(cases) == 6 and all(math.isfinite(t) for c in cases for t in c)
