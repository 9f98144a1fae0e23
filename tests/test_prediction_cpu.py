"""CPU: x0- and v-prediction DDPM nets (DDPM.with_prediction, DDPM.with_fixed_variance; mi355_ddpm_pred_sample, mi355_ddpm_vlb_pred, mi355_pred_step,
mi355_pred_shape_stats, mi355_vlb_terms_pred) - the views, the fixed large variance, every refusal that needs no GPU (the Python ones by message,
the library's through the ABI: they come before any launch and before the handle is looked at), the host loops on a recording op double, and the
rounding budget the GPU test holds mi355_pred_step to, proven here on an fp32 numpy restatement of the stated operation sequence.

Budget of one step (fp64 from the fp32 inputs, EPS32 = 2^-24, first-order rounding count r, bound (r + 1) EPS32 M, as tests/test_x0_shaping_cpu.py
and tests/test_learned_variance_cpu.py derive theirs).  The data prediction x0_hat carries r_pre roundings of values bounded by P:
  eps   x0_pre = fl(fl(c_recip x) - fl(c_recipm1 out)): r_pre = 3, P = |c_recip x| + |c_recipm1 out|         (today's count)
  v     x0_pre = fl(fl(sa x) - fl(sb out)):             r_pre = 3, P = |sa x| + |sb out|                      (sa, sb in place of c_recip, c_recipm1)
  x0    x0_pre = out:                                   r_pre = 0, P = |out|                                  (the three roundings are gone)
  shaped (rows f, s): out is f out (one rounding more) and the clipped value is divided by s >= 1 (one more): r_pre + 2 on the same P with f out.
The clip is exact and 1-Lipschitz.  Behind x0_hat the counts are those of the existing budgets less their own x0_hat share:
  ancestral     r = r_pre + 3: coef1 x0_hat adds its product, then the two sums; coef2 x: a product and two sums; sigma z: a product and a sum.
                M = |coef1| P + |coef2 x| + |sigma z|                                                        (eps unshaped: 6, shaped: 8, as today)
  learned var.  the mean as the ancestral step; sigma = exp(0.5 logvar) with tests/test_learned_variance_cpu.py's |d logvar| and 4 EPS32 on |sigma z|
  DDIM(eta)     r = r_pre + 7 on M = (sa' + sb' / c_recipm1) P + sb' |c_recip x| / c_recipm1 + |sigma z|, sa' = sqrt(prev), sb' = sqrt(max(1 - prev -
                sigma^2, 0)): c_recip x, the difference (bounded by |c_recip x| + P since |x0_hat| <= P), the division, two products, the sum, and the
                noise term's product and sum (eps unshaped: 10, shaped: 12, as today)
  DPM-Solver++  r = r_pre + 5 on M = |cx x| + |c0| P + |c1 hist|                                              (eps unshaped: 8, shaped: 10, as today)
  corrector     x + (kd (-rsm1 x0_hat) + kn z), kd = fl(fl(0.5 dt) delta), kn = sqrt(fl(dt delta)): the x0_hat term carries r_pre, kd's one rounding
                (the halving is exact), the score's product, kd's product and the two sums: r = r_pre + 5; the noise term kn's two roundings, a
                product and two sums (5 <= r for every kind once the last sum is shared); M = |x| + |kd rsm1| P + |kn z|.  r = r_pre + 6 covers both.
A kind that is confused with eps, sa and sb swapped, a + for the -, or the variance channel read as the prediction each leave the budget.
"""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

from tests import prediction_ref as PR
from tests.test_ddpm_respace_cpu import EPS32, STEPS7, step_inputs
from tests.test_x0_shaping_cpu import rows_for

PERS = [1, 5, 257, 3 * 32 * 32 + 3]
B = 3
PREDS = ("eps", "x0", "v")
STEP_KINDS = ("ddpm", "ddim", "ddim_eta", "dpmpp", "corrector", "ddpm_lv")
R_PRE = {"eps": 3, "x0": 0, "v": 3}
R_STEP = {"ddpm": 3, "ddpm_lv": 3, "ddim": 7, "ddim_eta": 7, "dpmpp": 5, "corrector": 6}


def _ddpm(Ns):
    from image_diffusion.sde_diffusion import DDPM

    return DDPM(Ns)


# ---- views -------------------------------------------------------------------------------------------------------------------------------------------

def test_prediction_views_commute_and_leave_the_tables_alone():
    from image_diffusion.sampling import _sched_key
    from image_diffusion.sde_diffusion import DDPM, TABLE_NAMES, RespacedDDPM, cosine_betas

    d = _ddpm(100)
    assert d.prediction == "eps" and d.fixed_variance == "small" and d.respace(5).prediction == "eps"
    for kind in PREDS:
        v = d.with_prediction(kind)
        assert v.prediction == kind and d.prediction == "eps" and type(v) is type(d) and v is not d
        assert all(a is b for (_, a), (_, b) in zip(v.named_buffers(), d.named_buffers())) and list(v.state_dict()) == list(d.state_dict())
        hv, hb = v.host_tables(), d.host_tables()
        assert list(hv) == list(hb) and all(torch.equal(hv[k], hb[k]) for k in hb)
        assert _sched_key(v) == _sched_key(d) and v.time(3) == d.time(3)
        assert v.with_prediction("eps").prediction == "eps"
    for bad in ("xstart", "V", None, 1):
        with pytest.raises(ValueError, match="prediction"):
            d.with_prediction(bad)
    for bad in ("fixed_large", "LARGE", None, True):
        with pytest.raises(ValueError, match="variance"):
            d.with_fixed_variance(bad)
    a = d.respace(STEPS7).with_prediction("v").with_fixed_variance("large").with_learned_variance().with_x0_shaping(0.9)
    b = d.with_x0_shaping(0.9).with_learned_variance().with_fixed_variance("large").with_prediction("v").respace(STEPS7)
    c = d.with_fixed_variance("large").respace(STEPS7).with_x0_shaping(0.9).with_prediction("v").with_learned_variance()
    for r in (a, b, c):
        assert isinstance(r, RespacedDDPM) and r.prediction == "v" and r.fixed_variance == "large" and r.learned_variance
        assert r.x0_shaping == a.x0_shaping is not None and r.timesteps == tuple(STEPS7) and [n for n, _ in r.named_buffers()] == list(TABLE_NAMES)
        assert all(torch.equal(x, y) for (_, x), (_, y) in zip(r.named_buffers(), a.named_buffers()))
        assert all(torch.equal(r.host_tables()[k], a.host_tables()[k]) for k in a.host_tables())
    # a from_betas chain keeps its time_scale under the views, respaced or not
    e = DDPM.from_betas(cosine_betas(100), time_scale=100).with_prediction("x0").with_fixed_variance("large")
    assert e.time_scale == 100.0 and e.prediction == "x0" and e.time(40) == 40.0
    er = e.respace(STEPS7)
    assert er.time_scale == 100.0 and er.prediction == "x0" and er.fixed_variance == "large" and er.time(4) == 40.0
    assert _sched_key(er) == _sched_key(DDPM.from_betas(cosine_betas(100), time_scale=100).respace(STEPS7))


@pytest.mark.parametrize("chain", ["plain", "cosine", "respaced", "respaced_cosine"])
def test_fixed_large_variance_is_max_log_from_step_one(chain):
    from image_diffusion.sde_diffusion import DDPM, cosine_betas

    base = _ddpm(100) if "cosine" not in chain else DDPM.from_betas(cosine_betas(100))
    d = base.respace(STEPS7) if chain.startswith("respaced") else base
    small = {k: v.clone() for k, v in d.host_tables().items()}
    big = d.with_fixed_variance("large")
    T = big.host_tables()
    name = "posterior_log_variance_clipped"
    assert T[name].dtype == torch.float32 and torch.equal(T[name][1:], d.max_log()[1:])
    assert torch.equal(T[name][:1], small[name][:1])                       # entry 0 is left alone: step 0 draws no noise
    assert all(torch.equal(T[k], small[k]) for k in small if k != name)
    assert all(torch.equal(d.host_tables()[k], small[k]) for k in small)   # the chain itself is untouched
    assert all(torch.equal(big.with_fixed_variance("small").host_tables()[k], small[k]) for k in small)
    # log(betas[k]) of the chain's own betas, in fp64, rounded once
    if chain.startswith("respaced"):
        acp = base.alphas_cumprod.double().numpy()[STEPS7]
        betas = 1.0 - acp / np.concatenate(([1.0], acp[:-1]))
    else:
        betas = base._betas64.numpy() if base._betas64 is not None else base.betas.double().numpy()
    assert np.array_equal(T[name][1:].numpy(), np.log(betas).astype(np.float32)[1:])
    assert bool((T[name][1:] >= small[name][1:]).all()) and bool((T[name][1:] > small[name][1:]).any())   # beta_k >= the posterior variance
    # the views commute
    other = (base.with_fixed_variance("large").respace(STEPS7) if chain.startswith("respaced") else base.with_prediction("v").with_fixed_variance("large"))
    assert torch.equal(other.host_tables()[name], T[name])
    moved = big.to(torch.float32)    # nn.Module._apply drops the cached tables
    assert torch.equal(moved.host_tables()[name], T[name])


def test_get_vlb_fn_reads_the_variance_and_the_kind_from_the_chain():
    from image_diffusion import bound

    d = _ddpm(100).respace(STEPS7)
    seen = []

    class Eng:
        out_channels = 1

        def ddpm_vlb(self, x, tables, logs, **kw):
            seen.append((logs, kw))
            return torch.zeros(x.shape[0], 7, 3), torch.zeros(x.shape[0], 2)

    from image_diffusion import sampling
    x0 = torch.zeros(2, 1, 8, 8)
    for chain, variance, pred in ((d, "fixed_small", None), (d.with_fixed_variance("large"), "fixed_large", None),
                                  (d.with_prediction("v"), "fixed_small", "v"), (d.with_prediction("x0").with_fixed_variance("large"), "fixed_large", "x0"),
                                  (d.with_prediction("eps"), "fixed_small", None)):
        seen.clear()
        fn = bound.get_vlb_fn(lambda xi, i: xi, chain)
        orig = sampling._fast_engine
        sampling._fast_engine = lambda *a: Eng()
        try:
            fn(x0)
        finally:
            sampling._fast_engine = orig
        logs, kw = seen[0]
        want = chain.vlb_log_variances(variance)
        assert set(logs) == set(want) and all(torch.equal(logs[k], want[k]) for k in want)
        assert kw.get("prediction") == pred and kw["learned"] is False


# ---- Python refusals ------------------------------------------------------------------------------------------------------------------------------------

def test_samplers_refuse_what_a_prediction_chain_cannot_do():
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, ReconstructionGuidance, Replacement
    from image_diffusion.likelihoods import InPainting

    d = _ddpm(100).respace(5)
    lik = InPainting(patch_size=4, pad_value=-2)
    net = lambda xi, i: torch.zeros(xi.shape[0], 1, 8, 8)   # noqa: E731
    am, rep = Amortized(1.0, 0, 0.1), Replacement(0.1, 1.0, True, 0)

    class Net:
        engine = None

    for kind in ("x0", "v"):
        p = d.with_prediction(kind)
        with pytest.raises(NotImplementedError, match="ReconstructionGuidance.*prediction"):
            sampling.get_conditional_sample_fn(sampling.make_eps_model(Net(), p), p, ReconstructionGuidance(1.0, 1.0, "before", 0, 0.1), lik)
        for what, chain in (("tiling", p.with_tiling(sampling.Tiling(stride=4))), ("feature_cache", p.with_feature_cache(sampling.FeatureCache(interval=2)))):
            for make in (lambda c: sampling.get_prior_sample_fn(net, c, am, lik), lambda c: sampling.get_conditional_sample_fn(net, c, am, lik),
                         lambda c: sampling.get_conditional_sample_fn(net, c, rep, lik), lambda c: sampling.get_ddim_sample_fn(net, c)):
                with pytest.raises(NotImplementedError, match=what + ".*prediction"):
                    make(chain)
        with pytest.raises(NotImplementedError, match="tiling.*prediction"):
            sampling.get_prior_sample_fn(net, p, am, lik, tiling=sampling.Tiling(stride=4))
        with pytest.raises(NotImplementedError, match="feature_cache.*prediction"):
            sampling.get_conditional_sample_fn(net, p, am, lik, feature_cache=sampling.FeatureCache(interval=2))
    # the eps view is the chain itself: everything above is taken
    e = d.with_prediction("eps")
    sampling.get_conditional_sample_fn(sampling.make_eps_model(Net(), e), e, ReconstructionGuidance(1.0, 1.0, "before", 0, 0.1), lik)
    sampling.get_prior_sample_fn(net, e.with_tiling(sampling.Tiling(stride=4)), am, lik)
    # one variance per chain
    both = d.with_learned_variance().with_fixed_variance("large")
    with pytest.raises(NotImplementedError, match="fixed variance.*learned-variance"):
        sampling.get_prior_sample_fn(net, both, am, lik)
    with pytest.raises(NotImplementedError, match="fixed variance.*learned-variance"):
        sampling.get_ddim_sample_fn(net, both)
    # the engine: tiling and the cache by name, a kind that is none
    from mi355 import _lib
    from mi355.engine import UNetEngine

    x = torch.zeros(2, 1, 8, 8)
    for kw in (dict(tiling=object()), dict(cache_interval=2), dict(cache_schedule=[1, 0]), dict(cache_branch=1)):
        with pytest.raises(NotImplementedError, match=next(iter(kw)) + ".*prediction"):
            UNetEngine.ddpm_sample(None, x, {}, mode=_lib.DDPM_PRIOR, prediction="v", **kw)
    with pytest.raises(ValueError, match="prediction must be one of"):
        UNetEngine.ddpm_sample(None, x, {}, mode=_lib.DDPM_PRIOR, prediction="xstart")
    with pytest.raises(ValueError, match="prediction must be one of"):
        UNetEngine.ddpm_vlb(None, x, {}, {}, learned=False, prediction="w")


def test_engine_and_ops_signatures():
    from mi355.engine import UNetEngine
    from mi355.ops import Ops

    p = inspect.signature(UNetEngine.ddpm_pred).parameters
    assert list(p)[:4] == ["self", "x", "tables", "prediction"] and all(p[k].default is None for k in ("shaping", "max_log", "times", "coefs"))
    q = inspect.signature(UNetEngine.ddpm_learned).parameters
    assert set(p) - {"prediction", "shaping"} == set(q)
    for fn in (UNetEngine.ddpm_sample, UNetEngine.ddpm_vlb):
        k = inspect.signature(fn).parameters["prediction"]
        assert k.default is None and k.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(Ops.pred_step_).parameters)[:7] == ["self", "kind", "prediction", "x", "out", "c_recip", "c_recipm1"]
    assert list(inspect.signature(Ops.pred_shape_stats).parameters)[:7] == ["self", "prediction", "x", "out", "c_recip", "c_recipm1", "shaping"]
    assert inspect.signature(Ops.vlb_terms).parameters["prediction"].default is None


# ---- the library's refusals, through the ABI --------------------------------------------------------------------------------------------------------------

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
    for name in ("mi355_ddpm_pred_workspace_bytes", "mi355_ddpm_pred_sample", "mi355_ddpm_vlb_pred", "mi355_pred_step", "mi355_pred_shape_stats",
                 "mi355_vlb_terms_pred"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.mi355_version() == 108   # additive: new symbols and one struct only
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
    ml = d.max_log().contiguous()
    var = _lib.DDPMVarianceC(1, C.cast(ml.data_ptr(), fp), None)

    def call(kind, v=None, sh=None, guided=0, sched=None, msched=None, tables=tb):
        pr = _lib.DDPMPredictionC(kind) if kind is not None else None
        return L.mi355_ddpm_pred_sample(None, None, 1, None, None, 0, guided, 2.0, None, C.byref(tables), C.byref(opt),
                                        C.byref(sched) if sched is not None else None, C.byref(msched) if msched is not None else None,
                                        C.byref(v) if v is not None else None, C.byref(sh) if sh is not None else None,
                                        C.byref(pr) if pr is not None else None, None, 0, 3, None, 0, None)

    err = L.mi355_last_error
    for kind in (-1, 3, 7):
        for kw in ({}, dict(sched=sd), dict(v=var)):
            assert call(kind, **kw) == -1 and b"ddpm_pred_sample: pred->kind must be" in err(), (kind, kw)
    # v needs the two tables it reads
    bare = _lib.DDPMTablesC()
    C.memmove(C.byref(bare), C.byref(tb), C.sizeof(tb))
    bare.sqrt_one_minus_alphas_cumprod = None
    assert call(2, tables=bare) == -1 and b"pred->kind 2 (v) needs tables->sqrt_alphas_cumprod" in err()
    assert call(1, tables=bare) == -1 and b"bad argument (net, x, workspace, batch)" in err()
    # the learned range together with shaping stays refused, whatever the kind; shaping switched off is no shaping
    on, off = _lib.X0ShapingC(0.9, 0.0, 0.0), _lib.X0ShapingC(0.0, 0.0, 0.0)
    for kind in (None, 0, 1, 2):
        assert call(kind, v=var, sh=on) == -1 and b"ddpm_pred_sample: var->learned together with shaping" in err()
        assert call(kind, v=var, sh=off) == -1 and b"bad argument (net, x, workspace, batch)" in err()
    # everything the underlying loops refuse, under this entry point's name; then, everything in order, the missing handle
    assert call(1, sh=_lib.X0ShapingC(2.0, 0.0, 0.0)) == -1 and b"ddpm_pred_sample: shaping->quantile" in err()
    assert call(1, sh=_lib.X0ShapingC(0.0, 0.0, 0.5)) == -1 and b"ddpm_pred_sample: shaping->rescale_phi > 0 needs guided" in err()
    assert call(2, v=_lib.DDPMVarianceC(2, None, None)) == -1 and b"ddpm_pred_sample: var->learned must be" in err()
    assert call(2, sched=sd, msched=ms) == -1 and b"ddpm_pred_sample: both sched and msched" in err()
    bad = _lib.DDPMScheduleC()
    bad.steps, bad.train_steps = sd.steps, 0
    assert call(2, sched=bad) == -1 and b"ddpm_pred_sample: train_steps" in err()
    assert call(1, msched=ms) == -1 and b"ddpm_pred_sample: opt->mode must be MI355_DDIM" in err()
    for kind in (None, 0, 1, 2):
        for kw in ({}, dict(sched=sd), dict(v=var), dict(sh=on), dict(sh=_lib.X0ShapingC(0.9, 0.0, 0.5), guided=1)):
            assert call(kind, **kw) == -1 and b"ddpm_pred_sample: bad argument (net, x, workspace, batch)" in err(), (kind, kw)
    assert L.mi355_ddpm_pred_workspace_bytes(None, 3, 0, 0) == -1 and b"ddpm_pred_workspace_bytes" in err()
    # the bound
    for kind in (-1, 3):
        pr = _lib.DDPMPredictionC(kind)
        assert L.mi355_ddpm_vlb_pred(None, None, 1, None, None, C.byref(tb), None, C.byref(pr), None, 0, None, None, 3, None, 0, None) == -1
        assert b"ddpm_vlb_pred: pred->kind must be" in err()
    pr = _lib.DDPMPredictionC(2)
    assert L.mi355_ddpm_vlb_pred(None, None, 1, None, None, C.byref(tb), None, C.byref(pr), None, 0, None, None, 3, None, 0, None) == -1
    assert b"ddpm_vlb: opt is null" in err()
    # the step op refuses before it looks at a pointer
    def pstep(kind, pk, per=16, n=48, stride=0, guided=0, shape=None, off=0, mn=-3.0, mx=-1.0):
        return L.mi355_pred_step(kind, pk, None, None, stride, None, None, guided, 0.0, None, per, 1.0, 1.0, 0.8, 0.6, 0.5, 0.5, 0.0, 0.0, mn, mx, 1, 7, off,
                                 shape, n, None)

    one = torch.zeros(8)
    assert pstep(6, 0) == -1 and b"pred_step: kind must be" in err()
    assert pstep(-1, 0) == -1 and b"pred_step: kind must be" in err()
    for pk in (-1, 3):
        for kind in range(6):
            assert pstep(kind, pk) == -1 and b"pred_step: pred_kind must be" in err()
    assert pstep(0, 1, n=50) == -1 and b"whole images" in err()
    assert pstep(0, 1, per=0) == -1 and b"whole images" in err()
    assert pstep(1, 2, stride=8) == -1 and b"pred_step: out_stride" in err()
    assert pstep(4, 2, guided=1) == -1 and b"no guided form" in err()
    assert pstep(4, 1, shape=C.c_void_p(one.data_ptr())) == -1 and b"the corrector keeps the static clip" in err()
    assert pstep(4, 1) == -1 and b"pred_step: null argument" in err()
    assert pstep(0, 2, off=2) == -1 and b"ddpm_step: the Philox offset" in err()
    assert pstep(1, 1) == -1 and b"ddim_step: null argument" in err()
    assert pstep(3, 2, guided=1) == -1 and b"dpmpp_cfg_step: null argument" in err()
    # (an empty state: the pointers are not asked for)
    assert pstep(5, 1, stride=16, n=0) == -1 and b"ddpm_lv_step: the variance channels sit behind" in err()
    assert pstep(5, 1, stride=32, n=0, mn=float("nan")) == -1 and b"ddpm_lv_step: min_log and max_log must be finite" in err()
    assert pstep(5, 2, stride=32, n=0, shape=C.c_void_p(one.data_ptr())) == -1 and b"not built for" in err()
    assert pstep(0, 1, stride=32, n=0, shape=C.c_void_p(one.data_ptr())) == -1 and b"not built for a strided eps" in err()
    assert pstep(5, 2, stride=32, n=0) == 0 and pstep(2, 1, n=0) == 0
    # the statistics op and the terms op
    sh = _lib.X0ShapingC(0.9, 0.0, 0.0)
    for pk in (-1, 3):
        assert L.mi355_pred_shape_stats(pk, None, None, 0.0, None, 0, 1.0, 1.0, 0.8, 0.6, C.byref(sh), None, None, 3, 16, None) == -1
        assert b"x0_shape_stats: the prediction kind must be" in err()
    assert L.mi355_pred_shape_stats(2, None, None, 0.0, None, 0, 1.0, 1.0, 0.8, 0.6, C.byref(sh), None, None, 3, 16, None) == -1 and b"x is null" in err()
    assert L.mi355_pred_shape_stats(1, None, None, 0.0, None, 0, 1.0, 1.0, 0.8, 0.6, C.byref(sh), None, None, 3, 16, None) == -1 and b"eps is null" in err()
    sc = (1.0, 1.0, 0.5, 0.5, -3.0, -3.0, -3.0, -1.0)

    def terms(pk, sa=0.8, sb=0.6, batch=0):
        return L.mi355_vlb_terms_pred(None, None, None, 16, None, 1, 0, 0, *sc, 0, 0, 0, 1, pk, sa, sb, None, 3, batch, 16, None)

    for pk in (-1, 3):
        assert terms(pk) == -1 and b"vlb_terms: the prediction kind must be" in err()
    assert terms(2, sa=float("nan")) == -1 and b"vlb_terms: sa and sb must be finite" in err()
    assert terms(1, sa=float("nan")) == 0 and terms(2) == 0      # an empty batch: nothing launched
    assert terms(2, batch=3) == -1 and b"vlb_terms: null argument" in err()
    del keep


# ---- the host loops on a recording op double -----------------------------------------------------------------------------------------------------------------

class _Rec:
    """Records every step op; the ops of a plain chain and the one step op of a prediction chain alike."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _draw(z):
        return None if z is None else float(z.reshape(-1)[0])

    def pred_step_(self, kind, prediction, x, out, cr, crm1, a, b=0.0, c=0.0, sigma=0.0, *, sa=0.0, sb=0.0, min_log=0.0, max_log=0.0, z=None,
                   philox=None, hist=None, w=None, shape=None):
        self.calls.append(dict(kind=kind, pred=prediction, x=tuple(x.shape), out=out, draw=self._draw(z), sa=sa, sb=sb, w=w, shape=shape, hist=hist is not None,
                               cr=cr, min_log=min_log, max_log=max_log))
        return x

    def pred_shape_stats(self, prediction, x, out, cr, crm1, shaping, *, sa=0.0, sb=0.0, w=None, detail=False):
        self.calls.append(dict(kind="stats", pred=prediction, x=tuple(x.shape), out=out, sa=sa, sb=sb, w=w))
        return "rows"

    def ddpm_step_(self, x, eps, z, cr, crm1, c1, c2, sigma, philox=None):
        self.calls.append(dict(kind="ddpm", pred=None, draw=self._draw(z)))
        return x

    def corrector_step_(self, x, eps, z, cr, crm1, rsm1, dt, delta, philox=None):
        self.calls.append(dict(kind="corrector", pred=None, draw=self._draw(z)))
        return x

    def ddim_eta_step_(self, x, eps, z, cr, crm1, prev, sigma, philox=None):
        self.calls.append(dict(kind="ddim_eta", pred=None, draw=self._draw(z)))
        return x

    def replace_mask_(self, x, cond, z, pad, noisy, sa, sb, philox=None):
        self.calls.append(dict(kind="paste", pred=None, draw=self._draw(z)))
        return x

    def renoise_(self, x, z, a, b, philox=None):
        self.calls.append(dict(kind="renoise", pred=None, draw=self._draw(z)))
        return x

    def clip_(self, x, lo, hi):
        return x


def test_generic_loops_issue_one_step_op_per_step_with_the_raw_output():
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance, RePaint, Replacement
    from image_diffusion.likelihoods import InPainting

    base = _ddpm(100).respace(STEPS7)
    lik = InPainting(patch_size=4, pad_value=-2)
    xT = torch.zeros(2, 1, 8, 8)
    draws = [torch.full((2, 1, 8, 8), float(j)) for j in range(60)]
    raw = {}

    def net_of(width):
        def net(xi, i):
            raw["last"] = torch.full((xi.shape[0], width, 8, 8), float(int(i[0])))
            return raw["last"]
        return net

    def run(chain, make, *args, width=1):
        rec = _Rec()
        with sampling.use_ops(rec), sampling.injected_noise(draws):
            make(net_of(width), chain)(*args)
        return rec.calls

    T = base.host_tables()
    for kind in ("x0", "v"):
        p = base.with_prediction(kind)
        # amortized with a corrector: one pred_step_ per predictor and per corrector; the draws numbered as on the plain chain
        mk = lambda n, c: sampling.get_conditional_sample_fn(n, c, Amortized(1.0, 1, 0.1), lik)   # noqa: E731
        got, plain = run(p, mk, xT, xT), run(base, mk, xT, xT)
        assert [c["kind"] for c in got] == ["ddpm", "corrector"] * 7 == [c["kind"] for c in plain]
        assert all(c["pred"] == kind for c in got) and all(c["pred"] is None for c in plain)
        assert [c["draw"] for c in got] == [c["draw"] for c in plain] and got[-2]["draw"] is None and got[0]["draw"] == 0.0
        steps = [i for i in range(6, -1, -1) for _ in range(2)]
        assert all(c["out"].shape == (2, 1, 8, 8) and float(c["out"][0, 0, 0, 0]) == i for c, i in zip(got, steps))     # the model's own output, whole
        assert [c["sa"] for c in got] == [float(T["sqrt_alphas_cumprod"][i]) for i in steps]
        assert [c["sb"] for c in got] == [float(T["sqrt_one_minus_alphas_cumprod"][i]) for i in steps]
        # replacement with a corrector, and one RePaint walk: the paste and the re-noising stay the loops' own
        for cond in (Replacement(0.1, 0.8, True, 1), RePaint(0.1, 0.8, True, 0, 2, 2)):
            mk = lambda n, c, cond=cond: sampling.get_conditional_sample_fn(n, c, cond, lik)   # noqa: E731
            got, plain = run(p, mk, xT, xT), run(base, mk, xT, xT)
            assert [(c["kind"], c["draw"]) for c in got] == [(c["kind"], c["draw"]) for c in plain]
            assert all(c["pred"] == kind for c in got if c["kind"] in ("ddpm", "corrector"))
            assert any(c["kind"] == "renoise" for c in got) == isinstance(cond, RePaint) and any(c["kind"] == "paste" for c in got)
        # DDIM(eta): one op per step, the draws as on the plain chain
        mk = lambda n, c: sampling.get_ddim_sample_fn(n, c, eta=0.5)   # noqa: E731
        got, plain = run(p, mk, xT), run(base, mk, xT)
        assert [(c["kind"], c["draw"]) for c in got] == [("ddim_eta", float(j)) for j in range(6)] + [("ddim_eta", None)] == \
            [(c["kind"], c["draw"]) for c in plain]
        got = run(p, lambda n, c: sampling.get_ddim_sample_fn(n, c), xT)
        assert [c["kind"] for c in got] == ["ddim"] * 7 and all(c["pred"] == kind and c["draw"] is None for c in got)
        # DPM-Solver++: the history goes with every step
        got = run(p, lambda n, c: sampling.get_dpm_solver_sample_fn(n, c), xT)
        assert [c["kind"] for c in got] == ["dpmpp"] * 7 and all(c["pred"] == kind and c["hist"] for c in got)
        # guided: the pair [2B] passed raw with the scale, on the duplicated state; shaped: the statistics op of the kind in front of each step
        mk = lambda n, c: sampling.get_conditional_sample_fn(n, c, ClassifierFreeGuidance(1.0, 0, 0.1, 3.0), lik)   # noqa: E731
        got = run(p, mk, xT, xT)
        assert [c["kind"] for c in got] == ["ddpm"] * 7 and all(c["x"] == (4, 1, 8, 8) and c["out"].shape == (4, 1, 8, 8) and c["w"] == 3.0 for c in got)
        got = run(p.with_x0_shaping(0.9, guidance_rescale=0.5), mk, xT, xT)
        assert [c["kind"] for c in got] == ["stats", "ddpm"] * 7 and all(c["pred"] == kind and c["w"] == 3.0 for c in got)
        assert all(c["x"] == (2, 1, 8, 8) and c["out"].shape == (4, 1, 8, 8) for c in got[0::2]) and all(c["shape"] == "rows" for c in got[1::2])
        got = run(p.with_x0_shaping(0.9), lambda n, c: sampling.get_dpm_solver_sample_fn(n, c, lik, guidance_scale=2.0), xT, xT)
        assert [c["kind"] for c in got] == ["stats", "dpmpp"] * 7 and all(c["shape"] == "rows" and c["hist"] and c["x"] == (4, 1, 8, 8) for c in got[1::2])
        # a learned variance range: [prediction | variance] passed whole to the learned-variance step, step 0 through the plain one
        lv = p.with_learned_variance()
        got = run(lv, lambda n, c: sampling.get_prior_sample_fn(n, c, Replacement(0.1, 1.0, True, 0), lik), xT, width=2)
        assert [c["kind"] for c in got] == ["ddpm_lv"] * 6 + ["ddpm"] and all(c["out"].shape == (2, 2, 8, 8) and c["pred"] == kind for c in got)
        assert [c["max_log"] for c in got[:6]] == [float(lv.max_log()[i]) for i in range(6, 0, -1)]
        assert [c["min_log"] for c in got[:6]] == [float(T["posterior_log_variance_clipped"][i]) for i in range(6, 0, -1)]
    # the fixed large variance reaches the plain ops as their sigma: nothing else changes
    rec = _Rec()
    sig = []
    rec.ddpm_step_ = lambda x, eps, z, cr, crm1, c1, c2, sigma, philox=None: sig.append(sigma) or x
    with sampling.use_ops(rec), sampling.injected_noise(draws):
        sampling.get_prior_sample_fn(net_of(1), base.with_fixed_variance("large"), Replacement(0.1, 1.0, True, 0), lik)(xT)
    ml = base.max_log()
    assert sig[:6] == [float((0.5 * ml[i]).exp()) for i in range(6, 0, -1)]


# ---- the budget --------------------------------------------------------------------------------------------------------------------------------------------

def pred_cases():
    """Per step k in (1, 3, Ns - 2) of DDPM(100).respace(STEPS7): the scalars every step kind reads there."""
    r = _ddpm(100).respace(STEPS7)
    T, ml = r.host_tables(), r.max_log()
    sg = r.ddim_sigma(0.5)
    cx, c0, c1 = r.dpm_solver_coefs(2)
    dt = (r.tmax - r.tmin) / r.Ns
    out = []
    for k in (1, 3, r.Ns - 2):
        g = lambda n: float(T[n][k])   # noqa: E731
        cr, crm1 = g("sqrt_recip_alphas_cumprod"), g("sqrt_recipm1_alphas_cumprod")
        out.append(dict(sa=g("sqrt_alphas_cumprod"), sb=g("sqrt_one_minus_alphas_cumprod"), c={
            "ddpm": (cr, crm1, g("posterior_mean_coef1"), g("posterior_mean_coef2"), float((0.5 * T["posterior_log_variance_clipped"][k]).exp())),
            "ddpm_lv": (cr, crm1, g("posterior_mean_coef1"), g("posterior_mean_coef2"), g("posterior_log_variance_clipped"), float(ml[k])),
            "ddim": (cr, crm1, g("alphas_cumprod_prev"), 0.0), "ddim_eta": (cr, crm1, g("alphas_cumprod_prev"), float(sg[k])),
            "dpmpp": (cr, crm1, float(cx[k]), float(c0[k]), float(c1[k])), "corrector": (cr, crm1, g("recip_sqrt_m1_alphas_cumprod"), dt, 0.1)}))
    return out


def pred_operands(kind, pred, per, case, seed, shaped=False, batch=B):
    """fp32 x [n], out [n] (the raw output of a net of the kind), z, hist, var [n] (each None where the step kind does not read it): about a third
    of x0_pre outside [-1, 1], the planted +-1 and one NaN in x (tests.test_ddpm_respace_cpu.step_inputs); shaped: scaled as step_operands does."""
    n = batch * per
    c = case["c"][kind]
    if pred == "v":
        x, out, z = step_inputs(n, case["sa"], case["sb"], seed)
    else:
        x, out, z = step_inputs(n, c[0], c[1], seed)
        if pred == "x0":      # the output is the data prediction itself
            out = np.random.default_rng(seed + 5).uniform(-1.5, 1.5, n).astype(np.float32)
    if shaped:
        x, out = (1.6 * x).astype(np.float32), (1.6 * out).astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    hist = rng.uniform(-1.0, 1.0, n).astype(np.float32) if kind == "dpmpp" else None
    var = None
    if kind == "ddpm_lv":
        var = (rng.uniform(-1.0, 1.0, (batch, per)) + np.linspace(-2.0, 2.0, batch)[:, None]).astype(np.float32).reshape(-1)
    return x, out, (z if kind in ("ddpm", "ddim_eta", "corrector", "ddpm_lv") else None), hist, var


def pred_budget(kind, pred, x, o, case, *, z=None, hist=None, var=None, f=None, s=None, per=None):
    """o: the (guided: mixed) fp32 output.  f, s: fp32 rows [B] (None: unshaped).  -> (fp64 step result from the fp32 inputs, fp64 x0_hat, the step's bound, x0_hat's bound (r_pre + 1) EPS32 P)."""
    c = tuple(float(np.float32(v)) for v in case["c"][kind])
    sa, sb = float(np.float32(case["sa"])), float(np.float32(case["sb"]))
    x64, o64 = x.astype(np.float64), o.astype(np.float64)
    z64, h64, v64 = (None if t is None else t.astype(np.float64) for t in (z, hist, var))
    shaped = f is not None
    fe = f64 = s64 = None
    if shaped:
        f64, s64 = np.repeat(f.astype(np.float64), per), np.repeat(s.astype(np.float64), per)
    want, xh = PR.step(kind, pred, x64, o64, c, sa=sa, sb=sb, z=z64, hist=h64, var=v64, f=f64, s=s64)
    fe = np.abs(o64 if not shaped else f64 * o64)
    P = {"eps": np.abs(c[0] * x64) + c[1] * fe, "v": np.abs(sa * x64) + sb * fe, "x0": fe}[pred]
    r = R_PRE[pred] + (2 if shaped else 0) + R_STEP[kind]
    noise = 0.0
    extra = 0.0
    if kind == "ddpm":
        noise = 0.0 if z64 is None else np.abs(c[4] * z64)
        M = abs(c[2]) * P + np.abs(c[3] * x64) + noise
    elif kind == "ddpm_lv":
        frac = (v64 + 1.0) * 0.5
        dlog = EPS32 * (3 * np.abs(frac) * abs(c[5]) + (np.abs(frac) + 3 * np.abs(1.0 - frac)) * abs(c[4]))
        sz = np.abs(np.exp(0.5 * (frac * c[5] + (1.0 - frac) * c[4])) * z64)
        M = abs(c[2]) * P + np.abs(c[3] * x64) + sz
        extra = sz * (0.5 * dlog + 4 * EPS32)
    elif kind in ("ddim", "ddim_eta"):
        prev, sg = c[2], c[3]
        sa2, sb2 = math.sqrt(prev), math.sqrt(max(1.0 - prev - sg * sg, 0.0))
        M = (sa2 + sb2 / c[1]) * P + sb2 * np.abs(c[0] * x64) / c[1] + (0.0 if z64 is None else np.abs(sg * z64))
    elif kind == "dpmpp":
        M = np.abs(c[2] * x64) + abs(c[3]) * P + np.abs(c[4] * h64)
    else:
        kd, kn = 0.5 * c[3] * c[4], math.sqrt(c[3] * c[4])
        M = np.abs(x64) + abs(kd * c[2]) * P + np.abs(kn * z64)
    return want, xh, (r + 1) * EPS32 * M + extra, (R_PRE[pred] + (2 if shaped else 0) + 1) * EPS32 * P


def pred_fp32(kind, pred, x, o, case, *, z=None, hist=None, var=None, f=None, s=None, per=None, mutant=None):
    """The stated operation sequence in fp32 numpy, every operation rounded.  mutant: "as_eps" (the kind confused with eps), "swap" (sa and sb
    swapped), "plus" (+ for the -), "var_as_pred" (the variance channel read as the prediction)."""
    t = np.float32
    c = tuple(t(v) for v in case["c"][kind])
    sa, sb = t(case["sa"]), t(case["sb"])
    if mutant == "swap":
        sa, sb = sb, sa
    if mutant == "var_as_pred":
        o = var
    fe = o if f is None else np.repeat(f, per) * o
    use = "eps" if mutant == "as_eps" else pred
    if use == "x0":
        pre = fe
    else:
        p, q = (c[0] * x, c[1] * fe) if use == "eps" else (sa * x, sb * fe)
        pre = p + q if mutant == "plus" else p - q
    sv = t(1) if s is None else np.repeat(s, per)
    with np.errstate(invalid="ignore"):
        xh = np.where(pre < -sv, -sv, np.where(pre > sv, sv, pre)).astype(t)
    if s is not None:
        xh = xh / sv
    if kind == "ddpm":
        m = c[2] * xh + c[3] * x
        out = m if z is None else m + c[4] * z
    elif kind == "ddpm_lv":
        frac = (var + t(1)) * t(0.5)
        logvar = frac * c[5] + (t(1) - frac) * c[4]
        out = (c[2] * xh + c[3] * x) + np.exp(t(0.5) * logvar).astype(t) * z
    elif kind in ("ddim", "ddim_eta"):
        prev, sg = c[2], c[3]
        sa2, sb2 = np.sqrt(prev), np.sqrt(np.maximum((t(1) - prev) - sg * sg, t(0)))
        m = sa2 * xh + sb2 * ((c[0] * x - xh) / c[1])
        out = m if z is None else m + sg * z
    elif kind == "dpmpp":
        m = c[2] * x + c[3] * xh
        out = m + c[4] * hist if c[4] != 0 else m
    else:
        kd, kn = t(0.5) * c[3] * c[4], np.sqrt(c[3] * c[4])
        out = x + (kd * (-c[2] * xh) + kn * z)
    return out.astype(t), xh.astype(t)


MUTANTS = {"eps": ("plus",), "x0": ("as_eps",), "v": ("as_eps", "swap", "plus")}


@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("pred", PREDS)
def test_fp32_restatement_of_the_steps_stays_inside_the_budget(per, pred):
    worst = {}
    broke, tried = {}, {}
    cases = pred_cases()
    n = B * per
    for j, case in enumerate(cases):
        for kind in STEP_KINDS:
            for shaped in ((False, True) if kind in ("ddpm", "ddim", "ddim_eta", "dpmpp") else (False,)):
                x, o, z, hist, var = pred_operands(kind, pred, per, case, 1000 * j + 37 * STEP_KINDS.index(kind) + per, shaped)
                # the reference inputs alone keep the planted NaN: exactly one non-finite element, in x, wherever step_inputs plants it
                assert int((~np.isfinite(x)).sum()) == (1 if n >= 8 else 0) and np.isfinite(o).all()
                assert all(np.isfinite(a).all() for a in (z, hist, var) if a is not None)
                f, s = rows_for(n, per, 9 * j + n) if shaped else (None, None)
                kw = dict(z=z, hist=hist, var=var, f=f, s=s, per=per)
                with np.errstate(invalid="ignore"):
                    want, xh, bound, bound0 = pred_budget(kind, pred, x, o, case, **kw)
                    got, g0 = pred_fp32(kind, pred, x, o, case, **kw)
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(got), nan) and nan.sum() == (1 if n >= 8 else 0), (kind, shaped)
                ratio = float((np.abs(got.astype(np.float64) - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max())
                key = kind + ("_shaped" if shaped else "")
                worst[key] = max(worst.get(key, 0.0), ratio)
                assert ratio <= 1.0, (kind, shaped, j, ratio)
                fin0 = np.isfinite(xh)
                assert (np.abs(g0.astype(np.float64) - xh)[fin0] <= bound0[fin0]).all(), (kind, shaped)
                if pred == "x0" and not shaped:      # no arithmetic: the clipped output itself
                    fin = np.isfinite(xh)
                    assert np.array_equal(g0[fin].view(np.uint32), np.clip(o, -1, 1)[fin].view(np.uint32))
                muts = MUTANTS[pred] + (("var_as_pred",) if kind == "ddpm_lv" else ())
                for mut in muts:
                    with np.errstate(invalid="ignore", over="ignore"):
                        bad = pred_fp32(kind, pred, x, o, case, mutant=mut, **kw)[0].astype(np.float64)
                    tried[mut] = tried.get(mut, 0) + 1
                    broke[mut] = broke.get(mut, 0) + bool((np.abs(bad - want)[~nan] > bound[~nan]).any())
    print(f"per = {per}, {pred}: fp32 restatement, max err / budget {({k: round(v, 3) for k, v in worst.items()})}; broken by each mutant: {broke} of {tried}")
    assert len(worst) == 10
    # every mutant leaves the budget in every case; with three elements in all (per = 1) one that moves only unclipped values may hide in a case
    assert set(tried) == set(MUTANTS[pred]) | {"var_as_pred"}
    assert broke == tried if n >= 8 else all(broke[m] >= tried[m] - 2 and broke[m] >= 1 for m in tried), (broke, tried)
    assert len(cases) == 3 and all(math.isfinite(v) for case in cases for c in case["c"].values() for v in c)
