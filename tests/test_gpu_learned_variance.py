"""GPU: learned-variance DDPM nets (mi355_ddpm_lv_sample, mi355_ddpm_lv_step, mi355_strided_step; DDPM.with_learned_variance, DDPM.from_betas).
  1. the step kernels on a strided eps are the contiguous kernels, bit for bit, and never read the variance channels;
  2. mi355_ddpm_lv_step against fp64 inside the budget tests/test_learned_variance_cpu.py derives, plain and guided, injected and Philox noise;
  3. mi355_ddpm_lv_sample without a variance struct is each of the six existing entry points, bit for bit;
  4. learned-variance sampling, plain and guided, with a corrector, on a respaced chain: fused vs the host loop, vs the fp64 restatement driven
     by the same fp32 network, and away from the fixed-variance result;
  5. DDIM, DDIM(eta) and DPM-Solver++ on the 2C-output net: fused vs the host loop;
  6. a from_betas chain with time_scale = T feeds the net the integer step;
  7. the public path is one library call per batch;
  8. the refusals that need a handle.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mi355.synth import randn
from tests import learned_variance_ref as LR
from tests.test_gpu_ddpm_respace import _banded, _bits, _report, _unband
from tests.test_learned_variance_cpu import PERS, lv_budget, lv_cases, lv_operands
from tests.test_x0_shaping_cpu import step_cases, step_operands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STOL = dict(rtol=2e-3, atol=1e-3)      # SAMPLER_TOL: the fused samplers against an fp64 restatement (tests/test_gpu_ddpm_respace.py)
B, S = 3, 16
W = 4.0
V_GAIN = 3.0                            # the out conv's variance rows are scaled by this: v spreads over a few units instead of sitting near 0
_CACHE = {}


# ---- 1. strided eps is the same arithmetic ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", PERS)
def test_strided_steps_are_the_contiguous_steps(per):
    from mi355.ops import default_ops as ops

    n = B * per
    wt = torch.tensor([1.75, 0.5, 3.0], device=DEV)
    seen = set()
    cases = step_cases()[4:8] + [("corrector", 1.3, 0.8, (1.2, 0.01, 0.1))]
    for j, (kind, a, b, c) in enumerate(cases):
        x, eps, z, hist = step_operands(kind if kind != "corrector" else "ddpm", n, a, b, 500 * j + per)
        eu = randn(9900 + j, n).numpy()
        for guided, w in ((False, None), (True, 2.5), (True, wt)):
            if guided and kind == "corrector":
                continue
            lead = 2 * B if guided else B
            e = torch.from_numpy(np.concatenate((eps, eu)) if guided else eps).view(lead, 1, per)
            wide = torch.cat((e, torch.full_like(e, float("nan"))), dim=1)       # [lead, 2, per]: eps | NaN
            res = {}
            for form in ("strided", "contiguous"):
                tx = torch.from_numpy(x).view(B, 1, per)
                bx, vx = _banded(torch.cat((tx, tx + 3.0)) if guided else tx, 1)
                assert vx.data_ptr() % 16 == 4
                bh, vh = _banded(torch.from_numpy(hist).view(B, 1, per), 1) if hist is not None else (None, None)
                zt = torch.from_numpy(z).to(DEV).view(B, 1, per) if z is not None else None
                if kind == "corrector":
                    if form == "strided":
                        ops.strided_step_("corrector", vx, wide.to(DEV), a, b, *c, z=zt)
                    else:
                        ops.corrector_step_(vx, e.to(DEV).contiguous(), zt, a, b, *c)
                else:
                    abc = dict(ddpm=(c[0], c[1]), ddim=(c[0],), ddim_eta=(c[0],), dpmpp=c)[kind]
                    kw = dict(sigma=c[-1] if kind in ("ddpm", "ddim_eta") else 0.0, z=zt, hist=vh, w=w)
                    if form == "strided":
                        ops.strided_step_(kind, vx, wide.to(DEV), a, b, *abc, **kw)
                    else:
                        ops.x0_shaped_step_(kind, vx, e.to(DEV).contiguous(), None, a, b, *abc, **kw)
                torch.cuda.synchronize()
                both = _unband(bx, vx.numel(), 1)
                if guided:
                    assert torch.equal(_bits(both[:n]), _bits(both[n:])), "the two halves differ"
                res[form] = (both[:n].clone(), _unband(bh, n, 1).clone() if bh is not None else None)
            got, want = res["strided"], res["contiguous"]
            assert torch.equal(_bits(got[0]), _bits(want[0])), (kind, guided)
            assert int(torch.isnan(got[0]).sum()) == (1 if n >= 8 else 0), "a variance channel (NaN) was read"
            assert not torch.equal(_bits(got[0]), _bits(torch.from_numpy(x))), "the step did nothing"
            if hist is not None:
                assert torch.equal(_bits(got[1]), _bits(want[1]))
            seen.add((kind, guided, isinstance(w, torch.Tensor)))
    assert len(seen) == 4 * 3 + 1


# ---- 2. the learned-variance step against fp64 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("philox", [False, True])
def test_lv_step_vs_fp64(per, philox):
    from mi355.ops import default_ops as ops

    n = B * per
    worst = {}
    wt = torch.tensor([1.75, 0.5, 3.0])
    for j, c in enumerate(lv_cases()):
        x, eps, v, z = lv_operands(per, c[0], c[1], 300 * j + per)
        ph = None
        if philox:
            ph = (4321 + j, 4 * j)
            z = ops.randn((n,), DEV, *ph).cpu().numpy()
        eu = randn(9800 + j, B, per).numpy()
        for guided, w in ((False, None), (True, 2.5), (True, wt)):
            if guided:
                wv = w[:, None] if isinstance(w, torch.Tensor) else w
                ec_d, eu_d = torch.from_numpy(eps).to(DEV), torch.from_numpy(eu).to(DEV)
                e_in = (eu_d + (ec_d - eu_d) * (wv.to(DEV) if isinstance(wv, torch.Tensor) else wv)).cpu().numpy()   # difference, product, sum: cfg_mix
                out = torch.cat((torch.stack((torch.from_numpy(eps), torch.from_numpy(v)), 1),
                                 torch.stack((torch.from_numpy(eu), torch.full((B, per), float("nan"))), 1)))          # [2B, 2, per]
            else:
                e_in = eps
                out = torch.stack((torch.from_numpy(eps), torch.from_numpy(v)), 1)                                          # [B, 2, per]
            with np.errstate(invalid="ignore"):
                want, bound = lv_budget(x, e_in, v, z, c)
            runs = []
            for _ in range(2):
                tx = torch.from_numpy(x).view(B, 1, per)
                bx, vx = _banded(torch.cat((tx, tx + 3.0)) if guided else tx, 1)
                _, vo = _banded(out, 1)
                zt = torch.from_numpy(z).to(DEV).view(B, 1, per) if ph is None else None
                ops.ddpm_lv_step_(vx, vo, zt, c[0], c[1], c[2], c[3], c[4], c[5], philox=ph, w=(w.to(DEV) if isinstance(w, torch.Tensor) else w))
                torch.cuda.synchronize()
                both = _unband(bx, vx.numel(), 1)
                if guided:
                    assert torch.equal(_bits(both[:n]), _bits(both[n:])), "the two halves differ"
                runs.append(both[:n].clone())
            assert torch.equal(_bits(runs[0]), _bits(runs[1])), "two runs differ"
            got = runs[0].double().numpy()
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and nan.sum() == (1 if n >= 8 else 0)
            key = "guided_w_dev" if isinstance(w, torch.Tensor) else ("guided" if guided else "plain")
            worst[key] = max(worst.get(key, 0.0), float((np.abs(got - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max()))
    print(f"per = {per}, philox = {philox}: ddpm_lv_step max err / budget {({k: round(t, 3) for k, t in worst.items()})}")
    assert len(worst) == 3 and max(worst.values()) <= 1.0, worst


# ---- nets, inputs -------------------------------------------------------------------------------------------------------------------------------

def _lv_net(in_ch, C, seed):
    """A tiny fp32 net with 2C outputs whose variance rows (the out conv's last C) are scaled by V_GAIN -> (cfg, net, state dict)."""
    from tests.test_gpu_unet import _tiny

    cfg, net, sd = _tiny(in_ch, 2 * C, seed, "fp32")
    sd = {k: t.clone() for k, t in sd.items()}
    sd["out.2.weight"][C:] *= V_GAIN
    sd["out.2.bias"][C:] *= V_GAIN
    net.load_state_dict(sd)
    return cfg, net.to(DEV), sd


@pytest.fixture(scope="module")
def nets():
    from tests.test_gpu_unet import _tiny

    return {(1, 1): _tiny(1, 1, 1001, "fp32"), (2, 1): _tiny(2, 1, 1002, "fp32"),            # (in_channels, out_channels) -> (cfg, net, sd)
            (1, 2): _lv_net(1, 1, 1011), (2, 2): _lv_net(2, 1, 1012), (3, 6): _lv_net(3, 3, 1013)}


def _inputs(C=1):
    xT = randn(8801, B, C, S, S)
    cond = (randn(8802, B, C, S, S) * 0.5).clamp(-1, 1)
    cond[:, :, 4:10, 5:11] = -2.0
    return xT, cond


def _chain():
    from image_diffusion.sde_diffusion import DDPM

    if "chain" not in _CACHE:
        d = DDPM(100)
        _CACHE["chain"] = d.respace(d.logsnr_steps(7))
    return _CACHE["chain"]


def _draws(C=1, n=40):
    return randn(8900 + C, n, B, C, S, S)


def _net_out(net, ddpm):
    """out(net_in, k) from the fp32 HIP network itself: the restatement's arithmetic is fp64, its network outputs the sampler's own."""
    def out(net_in, k):
        t = torch.full((net_in.shape[0],), ddpm.time(k), dtype=torch.float32, device=DEV)
        return net(net_in.float().to(DEV).contiguous(), t).cpu()

    return out


# ---- 3. no variance struct: the existing entry points ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loop", ["prior", "amortized_corrector", "repaint_corrector", "guided", "guided_ddim_eta", "dpm", "dpm_guided"])
def test_without_a_variance_struct_it_is_the_existing_entry_point(nets, loop):
    from image_diffusion.conditioning import repaint_walk
    from mi355 import _lib

    r = _chain()
    T = r.host_tables()
    xT, cond = (t.to(DEV) for t in _inputs())
    noise = _draws().to(DEV)
    sched = dict(timesteps=r.timesteps, train_steps=r.base_Ns)
    coefs = r.dpm_solver_coefs(2)
    cin, kw = {"prior": (1, dict(mode=_lib.DDPM_PRIOR, noise=noise)),                                                     # mi355_ddpm_sample
               "amortized_corrector": (2, dict(mode=_lib.DDPM_AMORTIZED, cond=cond, noise=noise, n_corrector=1, **sched)),   # _sched
               "repaint_corrector": (1, dict(mode=_lib.DDPM_REPLACEMENT, cond=cond, noise=noise, start_fraction=0.8, n_corrector=1,
                                             walk=repaint_walk(r.Ns, 2, 2), **sched)),
               "guided": (2, dict(mode=_lib.DDPM_AMORTIZED, cond=cond, noise=noise, guidance_scale=W, n_corrector=1)),   # _cfg_sample
               "guided_ddim_eta": (2, dict(mode=_lib.DDIM, cond=cond, noise=noise, guidance_scale=W, ddim_sigma=r.ddim_sigma(0.5), **sched)),
               "dpm": (1, dict(**sched)), "dpm_guided": (2, dict(cond=cond, guidance_scale=W, **sched))}[loop]
    eng = nets[(cin, 1)][1].engine(DEV)
    if loop.startswith("dpm"):
        want = eng.ddpm_multistep(xT.clone(), T, coefs, **kw)
        got = eng.ddpm_learned(xT.clone(), T, None, mode=_lib.DDIM, coefs=coefs, **kw)
    else:
        want = eng.ddpm_sample(xT.clone(), T, **kw)
        got = eng.ddpm_learned(xT.clone(), T, None, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)) and (want - xT).abs().max() > 1e-2
    eng.check()


# ---- 4. learned variance: fused, host loop, fp64 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["plain_corrector", "guided_corrector", "guided_per_image_w", "prior_rgb"])
def test_learned_variance_samplers(nets, case):
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance, Replacement
    from image_diffusion.likelihoods import InPainting

    base = _chain()
    r = base.with_learned_variance()
    assert r.learned_variance and r.timesteps == base.timesteps
    lik = InPainting(patch_size=6, pad_value=-2)
    Cs = 3 if case == "prior_rgb" else 1
    xT, cond = _inputs(Cs)
    noise = _draws(Cs)
    guided = case.startswith("guided")
    w = torch.tensor([4.0, 2.5, 5.5]) if case.endswith("per_image_w") else (W if guided else None)
    net = nets[(3, 6) if case == "prior_rgb" else (2, 2)][1]
    ncorr = 0 if case == "prior_rgb" else 1

    def make(eps_model):
        if case == "prior_rgb":
            return sampling.get_prior_sample_fn(eps_model, r, Replacement(0.1, 1.0, True, 0), lik)
        if not guided:
            return sampling.get_conditional_sample_fn(eps_model, r, Amortized(1.0, 1, 0.1), lik)
        return sampling.get_conditional_sample_fn(eps_model, r, ClassifierFreeGuidance(1.0, 1, 0.1, w.to(DEV) if isinstance(w, torch.Tensor) else w), lik)

    args = (xT.to(DEV),) if case == "prior_rgb" else (xT.to(DEV), cond.to(DEV))
    fast = sampling.make_eps_model(net, r)
    generic = lambda xi, i: fast(xi, i)   # noqa: E731  (untagged: the host loop over ddpm_lv_step_ and strided_step_)
    if isinstance(w, torch.Tensor):       # a per-image scale reaches the loops as the engine's guidance_scale
        eng = net.engine(DEV)
        with sampling.injected_noise(list(noise)):
            got = sampling._run_fast(eng, r, args[0], 1, args[1], n_corrector=1, delta=0.1, none_value=-2.0, guidance_scale=w.to(DEV)).cpu()
            gen = sampling._run_generic_cfg(generic, r, args[0], cond=args[1], none=lik.none_like(args[0]), guidance_scale=w.to(DEV), n_corrector=1,
                                            delta=0.1).cpu()
    else:
        with sampling.injected_noise(list(noise)):
            got = make(fast)(*args).cpu()
            gen = make(generic)(*args).cpu()
    kw = dict(cond=None if case == "prior_rgb" else cond, none_value=-2.0, w=w, n_corrector=ncorr, delta=0.1, tmin=r.tmin, tmax=r.tmax)
    out = _net_out(net, r)
    vs = []
    ref, used, n_eval = LR.sample(lambda a, k: (lambda o: vs.append(o[:B, Cs:]) or o)(out(a, k)), r.host_tables(), r.max_log(), xT, noise, **kw)
    fixed, _, _ = LR.sample(out, r.host_tables(), r.max_log(), xT, noise, learned=False, **kw)
    assert used == (r.Ns - 1) + ncorr * r.Ns and n_eval == r.Ns * ((2 if guided else 1) + ncorr)
    vall = torch.stack(vs)
    print(f"{case}: v in [{float(vall.min()):.3f}, {float(vall.max()):.3f}], std {float(vall.std()):.3f}")
    e1 = _report(f"{case}: fused vs fp64 restatement", got, ref)
    e2 = _report(f"{case}: fused vs host loop", got, gen)
    margin = 5 * (STOL["atol"] + STOL["rtol"] * float(fixed.abs().max()))
    e3 = _report(f"{case}: fp64 learned vs fp64 fixed variance (margin {margin:.3e})", ref, fixed)
    e4 = _report(f"{case}: fused vs fp64 fixed variance", got, fixed)
    assert float(got.abs().max()) <= 1.0 and bool(torch.isfinite(got).all())
    wmax = float(w.abs().max()) if isinstance(w, torch.Tensor) else (abs(w) if w is not None else 0.0)
    gb = 1e-4 * (1 + 2 * wmax) if guided else 1e-4
    torch.testing.assert_close(got, gen, rtol=gb, atol=gb)
    torch.testing.assert_close(got.double(), ref, **STOL)
    assert e3 > margin, "the restatement's learned variance does not move the result: the test shows nothing"
    assert e4 > margin
    assert np.isfinite(e1) and np.isfinite(e2)
    net.engine(DEV).check()


# ---- 5. the deterministic and DDIM(eta) samplers read the eps channels ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["ddim", "ddim_eta0.5", "dpm", "guided_ddim_eta0.5", "guided_dpm"])
def test_other_samplers_on_the_wide_net(nets, case):
    from image_diffusion import sampling
    from image_diffusion.likelihoods import InPainting

    r = _chain().with_learned_variance()
    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond = _inputs()
    noise = _draws()
    guided = case.startswith("guided")
    net = nets[(2, 2)][1]

    def make(eps_model):
        gs = W if guided else None
        if case.endswith("dpm"):
            return sampling.get_dpm_solver_sample_fn(eps_model, r, lik, guidance_scale=gs, order=2)
        return sampling.get_ddim_sample_fn(eps_model, r, lik, guidance_scale=gs, eta=0.5 if "eta" in case else 0.0)

    fast = sampling.make_eps_model(net, r)
    generic = lambda xi, i: fast(xi, i)   # noqa: E731
    with sampling.injected_noise(list(noise)):
        got = make(fast)(xT.to(DEV), cond.to(DEV)).cpu()
        gen = make(generic)(xT.to(DEV), cond.to(DEV)).cpu()
    _report(f"{case}: fused vs host loop", got, gen)
    gb = 1e-4 * (1 + 2 * W) if guided else 1e-4
    torch.testing.assert_close(got, gen, rtol=gb, atol=gb)
    assert float(got.abs().max()) <= 1.0 and bool(torch.isfinite(got).all()) and (got - xT).abs().max() > 1e-2
    # the variance channels are not read: the same sampler on the eps channels alone (a host loop around the sliced output) gives the host loop's bits
    base = _chain()
    sliced = lambda xi, i: fast(xi, i)[:, :1].contiguous()   # noqa: E731
    with sampling.injected_noise(list(noise)):
        if case.endswith("dpm"):
            narrow = sampling.get_dpm_solver_sample_fn(sliced, base, lik, guidance_scale=W if guided else None, order=2)(xT.to(DEV), cond.to(DEV)).cpu()
        else:
            narrow = sampling.get_ddim_sample_fn(sliced, base, lik, guidance_scale=W if guided else None, eta=0.5 if "eta" in case else 0.0)(
                xT.to(DEV), cond.to(DEV)).cpu()
    _report(f"{case}: host loop on the 2C output vs host loop on its eps channels", gen, narrow)
    torch.testing.assert_close(gen, narrow, rtol=gb, atol=gb)
    net.engine(DEV).check()


@pytest.mark.parametrize("case", ["replacement_corrector", "repaint"])
def test_replacement_and_repaint_on_the_wide_net(nets, case):
    """The paste and the RePaint walk are the loops' own; the predictor between them is the learned-variance step: fused vs the host loop."""
    from image_diffusion import sampling
    from image_diffusion.conditioning import RePaint, Replacement
    from image_diffusion.likelihoods import InPainting

    r = _chain().with_learned_variance()
    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond = (t.to(DEV) for t in _inputs())
    noise = _draws(n=80)
    net = nets[(1, 2)][1]
    conditioning = Replacement(0.1, 0.8, True, 1) if case == "replacement_corrector" else RePaint(0.1, 0.8, True, 0, 2, 2)
    fast = sampling.make_eps_model(net, r)
    with sampling.injected_noise(list(noise)):
        got = sampling.get_conditional_sample_fn(fast, r, conditioning, lik)(xT, cond).cpu()
        gen = sampling.get_conditional_sample_fn(lambda xi, i: fast(xi, i), r, conditioning, lik)(xT, cond).cpu()
        fixed = sampling.get_conditional_sample_fn(lambda xi, i: fast(xi, i)[:, :1].contiguous(), _chain(), conditioning, lik)(xT, cond).cpu()
    _report(f"{case}: fused vs host loop", got, gen)
    e = _report(f"{case}: learned vs fixed variance (host loop on the eps channels)", got, fixed)
    torch.testing.assert_close(got, gen, rtol=1e-4, atol=1e-4)
    assert float(got.abs().max()) <= 1.0 and bool(torch.isfinite(got).all()) and e > 5 * (STOL["atol"] + STOL["rtol"])
    net.engine(DEV).check()


# ---- 6. a chain built from betas feeds the integer step ------------------------------------------------------------------------------------------------

def test_from_betas_chain_feeds_the_integer_time(nets):
    from image_diffusion import sampling
    from image_diffusion.conditioning import Replacement
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM, cosine_betas

    lik = InPainting(patch_size=6, pad_value=-2)
    c = DDPM.from_betas(cosine_betas(100), time_scale=100)
    tau = 40
    one = c.respace([tau])                       # one step: the result is the clipped mean of the first (and only) evaluation
    assert one.time(0) == float(tau)
    net = nets[(1, 1)][1]
    eng = net.engine(DEV)
    xT = (0.4 * _inputs()[0]).to(DEV)
    got = sampling.get_prior_sample_fn(sampling.make_eps_model(net, one), one, Replacement(0.1, 1.0, True, 0), lik)(xT).cpu().double()
    T = {k: v.double() for k, v in one.host_tables().items()}

    def expect(t):
        eps = eng.forward(xT, float(t)).cpu().double()            # mi355_unet_forward_t
        x0 = (T["sqrt_recip_alphas_cumprod"][0] * xT.cpu().double() - T["sqrt_recipm1_alphas_cumprod"][0] * eps).clamp(-1, 1)
        return (T["posterior_mean_coef1"][0] * x0 + T["posterior_mean_coef2"][0] * xT.cpu().double()).clamp(-1, 1)

    at_int, at_unit = expect(tau), expect(tau / 100.0)
    d_int, d_unit = _report("one step at t = 40: sampler vs forward_t(40)", got, at_int), _report("... vs forward_t(0.4)", got, at_unit)
    assert d_int <= 1e-5 and d_unit > 1e-3, (d_int, d_unit)
    # and a learned-variance sampler on such a chain: fused (the times go in with the variance struct) vs the host loop (eps_model's times)
    r = c.respace([0, 5, 15, 30, 50, 70, 90]).with_learned_variance()
    assert [r.time(k) for k in range(r.Ns)] == [0.0, 5.0, 15.0, 30.0, 50.0, 70.0, 90.0]
    wide = nets[(1, 2)][1]
    fast = sampling.make_eps_model(wide, r)
    noise = _draws()
    x7 = _inputs()[0].to(DEV)
    with sampling.injected_noise(list(noise)):
        a = sampling.get_prior_sample_fn(fast, r, Replacement(0.1, 1.0, True, 0), lik)(x7).cpu()
        b = sampling.get_prior_sample_fn(lambda xi, i: fast(xi, i), r, Replacement(0.1, 1.0, True, 0), lik)(x7).cpu()
    ref, _, _ = LR.sample(_net_out(wide, r), r.host_tables(), r.max_log(), x7.cpu(), noise)
    _report("from_betas, learned variance: fused vs host loop", a, b)
    _report("from_betas, learned variance: fused vs fp64 restatement", a, ref)
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(a.double(), ref, **STOL)
    eng.check()
    wide.engine(DEV).check()


# ---- 7. the public path ------------------------------------------------------------------------------------------------------------------------------------

def test_public_path_is_one_library_call(nets, monkeypatch):
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib

    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond = (t.to(DEV) for t in _inputs())
    d = DDPM(25)
    # the launches of one evaluation of the same topology with a C-channel out conv: what the existing loops leave behind
    twin = nets[(2, 1)][1].engine(DEV)
    twin.ddpm_sample(xT.clone(), d.host_tables(), mode=_lib.DDPM_PRIOR)
    n_plain = twin.stats(B)["launches"]
    twin.ddpm_sample(xT.clone(), d.host_tables(), mode=_lib.DDPM_AMORTIZED, cond=cond, guidance_scale=W)
    n_guided = twin.stats(B)["launches"]
    net = nets[(2, 2)][1]
    eng = net.engine(DEV)
    calls = []
    real = eng.ddpm_learned
    monkeypatch.setattr(eng, "ddpm_learned", lambda *a, **k: calls.append(k.get("mode")) or real(*a, **k))
    for name in ("ddpm_sample", "ddpm_shaped", "ddpm_multistep"):
        monkeypatch.setattr(eng, name, lambda *a, **k: pytest.fail("an entry point without the variance struct ran"))
    r = d.with_learned_variance().respace(10)
    assert r.learned_variance
    em = sampling.make_eps_model(net, r)
    runs = [(sampling.get_prior_sample_fn(em, r, Amortized(1.0, 0, 0.1), lik), (xT,), n_plain),
            (sampling.get_conditional_sample_fn(em, r, ClassifierFreeGuidance(1.0, 0, 0.1, W), lik), (xT, cond), n_guided),
            (sampling.get_conditional_sample_fn(em, r, Amortized(1.0, 0, 0.1), lik), (xT, cond), n_plain),
            (sampling.get_ddim_sample_fn(em, r, lik, guidance_scale=W, eta=0.5), (xT, cond), n_guided),
            (sampling.get_dpm_solver_sample_fn(em, r, lik, guidance_scale=W), (xT, cond), n_guided)]
    for fn, args, n0 in runs:
        calls.clear()
        out = fn(*args)
        assert len(calls) == 1 and eng.stats(B)["launches"] == n0 + 1 and n0 > 0, (len(calls), eng.stats(B)["launches"], n0)
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0 and (out - xT).abs().max() > 1e-2
    eng.check()
    # the widths against the chain, both ways, before any call
    with pytest.raises(ValueError, match="with_learned_variance"):
        sampling.get_prior_sample_fn(sampling.make_eps_model(net, d), d, Amortized(1.0, 0, 0.1), lik)(xT)
    narrow = nets[(2, 1)][1]
    with pytest.raises(ValueError, match="twice the state's channels"):
        sampling.get_prior_sample_fn(sampling.make_eps_model(narrow, r), r, Amortized(1.0, 0, 0.1), lik)(xT)


# ---- 8. the refusals that need a handle --------------------------------------------------------------------------------------------------------------------

def test_refusals_that_need_a_handle(nets):
    from mi355 import _lib
    from mi355._lib import MI355BackendError

    r = _chain().with_learned_variance()
    T, ml = r.host_tables(), r.max_log()
    xT, cond = (t.to(DEV) for t in _inputs())
    sched = dict(timesteps=r.timesteps, train_steps=r.base_Ns)
    L = _lib.lib()
    narrow, wide = nets[(2, 1)][1].engine(DEV), nets[(2, 2)][1].engine(DEV)
    for kw in (dict(mode=_lib.DDPM_PRIOR), dict(mode=_lib.DDPM_AMORTIZED, cond=cond, guidance_scale=W), dict(mode=_lib.DDIM, coefs=r.dpm_solver_coefs(2))):
        with pytest.raises(MI355BackendError, match="ddpm_lv_sample: var->learned needs a net whose out_channels == 2 \\* channels"):
            narrow.ddpm_learned(xT.clone(), T, ml, **kw, **sched)
        assert b"var->learned" in L.mi355_last_error()
        with pytest.raises(MI355BackendError, match="ddpm_lv_sample: eps model must output the state's channel count"):
            wide.ddpm_learned(xT.clone(), T, None, **kw, **sched)
    with pytest.raises(MI355BackendError, match="ddpm_lv_sample: replacement needs an unconditional net"):
        wide.ddpm_learned(xT.clone(), T, ml, mode=_lib.DDPM_REPLACEMENT, cond=cond, **sched)
    with pytest.raises(MI355BackendError, match="ddpm_lv_sample: injected noise exhausted"):
        wide.ddpm_learned(xT.clone(), T, ml, mode=_lib.DDPM_PRIOR, noise=_draws(n=2).to(DEV), **sched)
    with pytest.raises(MI355BackendError, match="ddpm_lv_sample: workspace too small"):
        ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
        tb, keep = narrow._ddpm_tables(T)
        opt = _lib.DDPMOptionsC(_lib.DDPM_PRIOR, 0, 0.1, 1e-5, 1.0, 1.0, 1, -2.0, -2.0, 1, 0)
        _lib.check(L.mi355_ddpm_lv_sample(narrow.handle,C.c_void_p(xT.data_ptr()), 1, None, None, 0, 0, 0.0, None, C.byref(tb), C.byref(opt), None, None,
                                          None, None, 0, B, C.c_void_p(ws.data_ptr()), 4096, None), "mi355_ddpm_lv_sample")
    with pytest.raises(ValueError, match="max_log must have one entry per row"):
        wide.ddpm_learned(xT.clone(), T, ml[:3], mode=_lib.DDPM_PRIOR, **sched)
    with pytest.raises(ValueError, match="times must have one entry per row"):
        wide.ddpm_learned(xT.clone(), T, ml, times=[0.5], mode=_lib.DDPM_PRIOR, **sched)
    # the workspace of the loop chosen: what the existing entry points ask for on a C-output net, and enough for the wide net's guided tail
    h = narrow.handle
    assert L.mi355_ddpm_lv_workspace_bytes(h, B, 0, 0) == L.mi355_unet_workspace_bytes(h, B)
    assert L.mi355_ddpm_lv_workspace_bytes(h, B, 1, 0) == L.mi355_ddpm_cfg_workspace_bytes(h, B)
    assert L.mi355_ddpm_lv_workspace_bytes(h, B, 0, 1) == L.mi355_ddpm_multistep_workspace_bytes(h, B, 0)
    assert L.mi355_ddpm_lv_workspace_bytes(h, B, 1, 1) == L.mi355_ddpm_multistep_workspace_bytes(h, B, 1)
    assert L.mi355_ddpm_lv_workspace_bytes(wide.handle, B, 1, 0) >= L.mi355_ddpm_cfg_workspace_bytes(wide.handle, B) + 2 * B * S * S * 4
    # the step ops on device tensors
    from mi355.ops import default_ops as ops
    x, out = torch.zeros(B, 1, 8, device=DEV), torch.zeros(B, 3, 8, device=DEV)
    with pytest.raises(ValueError, match="twice the state's channels"):
        ops.ddpm_lv_step_(x, out, None, 1.0, 1.0, 0.5, 0.5, -3.0, -1.0)
    with pytest.raises(ValueError, match="at least as many channels"):
        ops.strided_step_("ddim", out, x, 1.0, 1.0, 0.5)
    with pytest.raises(MI355BackendError, match="strided_step: the corrector has no guided form"):
        ops.strided_step_("corrector", torch.zeros(2 * B, 1, 8, device=DEV), torch.zeros(2 * B, 2, 8, device=DEV), 1.0, 1.0, 0.5, 0.1, 0.1, w=2.0)
    narrow.check()
    wide.check()
